"""GPU: FOC's tinycudann network on the fused kernels (focnerf_amd/network_tcnn.py): one sigma hidden layer in the whole-field kernels, and
column 47 of the 48-wide object-conditioned colour input held at the pad value (1.0 for tcnn's layout) through the *_pad entry points.

  * foc_field_forward_train_pad at (1, 2) / (1, 3) is bit for bit foc_ffmlp_forward_planar(num_layers = 1) + foc_color_head_forward_pad;
  * the colour head with pad 1.0, forward and backward, is bit for bit the plain fused MLP on the materialised 48-wide input with column
    47 = 1.0 (integer-valued data: every sum is exact, so the order of summation cannot show; zeros of the weight gradient may differ in
    sign); with pad 0 the twins are the old entry points;
  * foc_nerf_field_inference_pad at (1, 2) / (1, 3), with and without the pad, against the oracle chain;
  * the network, run(fused=True), against FOC's network on the drop-in (op by op) with the same parameters, in training and inference, trains;
  * checkpoints written from drop-in-built objects render through load_objects -> the combiner as the drop-in objects do op by op.
Nothing here reads the reference tree."""
import math

import numpy as np
import pytest
import torch

import oracle
from oracle import torch_cpu_nerf
from util import assert_half_close, to_np

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -10
LOSS_SCALE = 4096.0


def _ints(g, shape, lo, hi, scale=1.0):
    return (torch.randint(lo, hi + 1, shape, generator=g, device="cuda").float() * scale).half()


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("nlc", [2, 3])
@pytest.mark.parametrize("B", [1, 31, 32, 4097, 1 << 21])
@pytest.mark.parametrize("mode", ["pad", "obj", "plain"])
def test_field_forward_one_hidden_layer_is_bitwise_the_two_calls(nlc, B, mode):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    g = torch.Generator(device="cuda").manual_seed(10 * nlc + B)
    T = 7
    n_rays = (B + T - 1) // T
    planes = ((torch.rand(16, B, 2, generator=g, device="cuda") - 0.5) * 2).half()
    w_s = (torch.randn(64 * (32 + 16), generator=g, device="cuda") * 0.25).half()
    ld0 = 32 if mode == "plain" else 48
    w_c = (torch.randn(64 * (ld0 + 64 * (nlc - 1) + 16), generator=g, device="cuda") * 0.25).half()
    ray_sh = (torch.randn(n_rays, 16, generator=g, device="cuda") * 0.5).half()
    obj = None if mode == "plain" else (torch.randn(16, generator=g, device="cuda") * 0.8).half()
    pad = 1.0 if mode == "pad" else 0.0
    st = stream_of(planes)
    h1 = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    c1 = torch.empty(B, 4, dtype=torch.float16, device="cuda")
    check(lib.foc_ffmlp_forward_planar(ptr(planes), ptr(w_s), B, 32, 16, 64, 1, 0, 6, ptr(h1), st), "sigma forward")
    check(lib.foc_color_head_forward_pad(ptr(h1), ptr(ray_sh), T, ptr(w_c), B, 64, nlc, 0, ptr(c1), 4, ptr(obj), pad, st), "colour forward")
    h2 = torch.full((B + 8, 16), 5.0, dtype=torch.float16, device="cuda")
    c2 = torch.full((B + 8, 4), 5.0, dtype=torch.float16, device="cuda")
    check(lib.foc_field_forward_train_pad(ptr(planes), ptr(w_s), 1, ptr(ray_sh), T, ptr(w_c), nlc, 64, 0, B, ptr(h2), ptr(c2), 4, ptr(obj), pad, st),
          "fused forward")
    torch.cuda.synchronize()
    assert torch.all(h2[B:] == 5.0) and torch.all(c2[B:] == 5.0), "rows past B were written"
    assert torch.equal(h2[:B].view(torch.int16), h1.view(torch.int16)), "h differs from foc_ffmlp_forward_planar"
    assert torch.equal(c2[:B].view(torch.int16), c1.view(torch.int16)), "colour logits differ from foc_color_head_forward_pad"
    if mode != "pad":                                   # pad 0: the old entry point gives the same bits
        c3 = torch.empty(B, 4, dtype=torch.float16, device="cuda")
        check(lib.foc_field_forward_train(ptr(planes), ptr(w_s), 1, ptr(ray_sh), T, ptr(w_c), nlc, 64, 0, B, ptr(h2), ptr(c3), 4, ptr(obj), st), "old")
        torch.cuda.synchronize()
        assert torch.equal(c3.view(torch.int16), c1.view(torch.int16))
    if B > 1000:
        assert h1.float().abs().max() > 0.5 and c1.float().abs().max() > 0.1, "degenerate test data"


def _colour_head(lib, fn_fwd, fn_bwd, h, ray_sh, T, W, B, layers, grad, obj, pad):
    from focnerf_amd._lib import ptr, stream_of, check
    st = stream_of(h)
    n_w = W.numel()
    out = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    extra = () if pad is None else (pad,)
    check(getattr(lib, fn_fwd)(ptr(h), ptr(ray_sh), T, ptr(W), B, 64, layers, 0, ptr(out), 16, ptr(obj), *extra, st), "fwd")
    grad_h = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    g_w = torch.empty(n_w, dtype=torch.float16, device="cuda")
    g_obj = torch.empty(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.foc_ffmlp_backward_workspace_bytes(48, 64, layers), dtype=torch.uint8, device="cuda")
    check(getattr(lib, fn_bwd)(ptr(grad), ptr(h), ptr(ray_sh), T, None, ptr(W), B, 64, layers, 0, ptr(grad_h), ptr(g_w), ptr(ws), ws.numel(), 16,
                               ptr(obj), ptr(g_obj), *extra, st), "bwd")
    torch.cuda.synchronize()
    return out, grad_h, g_w, g_obj


@pytest.mark.parametrize("layers,T,N", [(2, 64, 37), (3, 1, 700), (2, 512, 9)])
def test_colour_head_with_pad_is_the_plain_mlp_on_the_materialised_input(layers, T, N):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    g = torch.Generator(device="cuda").manual_seed(layers * 1000 + T)
    B = N * T
    # integers in {-1, 0, 1}: every activation, delta and product is an integer and every fp32 sum stays below 2^24, so it is exact
    h = _ints(g, (B, 16), -1, 1)
    ray_sh = _ints(g, (N, 16), -1, 1)
    obj = _ints(g, (16,), -1, 1)
    n_w = 64 * (48 + 64 * (layers - 1) + 16)
    W = _ints(g, (n_w,), -1, 1)
    grad = torch.zeros(B, 16, dtype=torch.float16, device="cuda")
    grad[:, :3] = _ints(g, (B, 3), -1, 1)
    out, grad_h, g_w, g_obj = _colour_head(lib, "foc_color_head_forward_pad", "foc_color_head_backward_pad", h, ray_sh, T, W, B, layers, grad, obj, 1.0)

    # the plain fused MLP on [SH16 | h[:,1:16] | obj | 1.0]
    cin = torch.cat([ray_sh.repeat_interleave(T, 0), h[:, 1:], obj.expand(B, 16), torch.ones(B, 1, dtype=torch.float16, device="cuda")], 1).contiguous()
    st = stream_of(h)
    ref = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    check(lib.foc_ffmlp_forward(ptr(cin), ptr(W), B, 48, 16, 64, layers, 0, 6, None, ptr(ref), st), "plain fwd")
    g_in = torch.empty(B, 48, dtype=torch.float16, device="cuda")
    g_w_ref = torch.empty(n_w, dtype=torch.float16, device="cuda")
    ws = torch.empty(lib.foc_ffmlp_backward_workspace_bytes(48, 64, layers), dtype=torch.uint8, device="cuda")
    check(lib.foc_ffmlp_backward(ptr(grad), ptr(cin), ptr(W), None, B, 48, 16, 64, layers, 0, 6, 1, None, ptr(g_in), ptr(g_w_ref), ptr(ws), ws.numel(), st),
          "plain bwd")
    torch.cuda.synchronize()
    assert out.float().abs().max() >= 1 and torch.isfinite(out.float()).all() and out.float().abs().max() < 2048, "degenerate test data"
    assert torch.isfinite(g_w.float()).all() and torch.isfinite(g_in.float()).all()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), "logits"
    assert torch.equal(grad_h[:, 1:].view(torch.int16), g_in[:, 16:31].view(torch.int16)), "grad_h"
    assert torch.all(grad_h[:, 0] == 0)
    dW0 = g_w.view(-1)[:64 * 48].view(64, 48)
    assert dW0[:, 47].float().abs().max() > 0, "the pad column's gradient is there"
    # equal values; the sign of a zero may differ: the head writes dW0[:, 31 + j] = colsum * obj[j], -0 where obj[j] = 0 and colsum < 0
    assert torch.equal(g_w, g_w_ref), "weight gradient (dW0[:, 47] included)"
    nz = g_w_ref != 0
    assert torch.equal(g_w[nz].view(torch.int16), g_w_ref[nz].view(torch.int16))
    # grad_obj = W0[:, 31:47]^T colsum(delta_0): the object columns' input gradient summed over the batch
    # (g_in is rounded to half per row: a loose bound)
    want = g_in[:, 31:47].float().sum(0)
    assert torch.allclose(g_obj, want, rtol=1e-2, atol=1e-2 * float(want.abs().max()))

    # pad 0: the twins are the old entry points, bit for bit (random data)
    W = (torch.randn(n_w, generator=g, device="cuda") * 0.2).half()
    h = (torch.randn(B, 16, generator=g, device="cuda") * 0.7).half()
    obj = (torch.randn(16, generator=g, device="cuda") * 0.8).half()
    a = _colour_head(lib, "foc_color_head_forward_pad", "foc_color_head_backward_pad", h, ray_sh, T, W, B, layers, grad, obj, 0.0)
    b = _colour_head(lib, "foc_color_head_forward", "foc_color_head_backward", h, ray_sh, T, W, B, layers, grad, obj, None)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16),
                           y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16))


def _sh16(dirs):
    return torch_cpu_nerf.sh_encode_deg4(dirs.detach().cpu().float()).numpy().astype(np.float16)


@pytest.mark.parametrize("num_layers_color", [3, 4])
@pytest.mark.parametrize("pad", [1.0, 0.0])
@pytest.mark.parametrize("blocked", [False, True])
def test_field_inference_one_hidden_layer_vs_oracle_chain(num_layers_color, pad, blocked):
    """k_nerf_infer<1, NLC, ..., OBJ> through field_infer: grid_encode_forward -> ffmlp_forward(32 -> 64 -> 16) -> [SH | geo | obj | pad] ->
    ffmlp_forward(48 -> 64 (-> 64) -> 16) -> sigmoid."""
    from focnerf_amd import _lib
    from focnerf_amd.field import field_infer
    from focnerf_amd.network_tcnn import NeRFNetwork
    torch.manual_seed(3)
    m = NeRFNetwork(bound=1, num_layers_color=num_layers_color).cuda().eval()
    m.colour_input_pad = pad
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-0.5, 0.5)
        m.color_net.weights.mul_(1.5)
    nl_c = num_layers_color - 1
    obj = torch.randn(16, device="cuda") * 0.8
    T = 8
    N = 200 if blocked else 1000
    B = (-(-N // 64) * 64 * T) if blocked else N
    xn = torch.rand(B, 3, device="cuda")
    d = torch.nn.functional.normalize(torch.randn(N, 3, device="cuda"), dim=-1)
    calls = []
    orig = _lib.lib.foc_nerf_field_inference_pad
    _lib.lib.foc_nerf_field_inference_pad = lambda *a: calls.append(1) or orig(*a)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            sigma, rgb = field_infer(m, xn, d, dir_div=T if blocked else 1, dir_block=64 if blocked else 0, obj_feat=obj)
    finally:
        _lib.lib.foc_nerf_field_inference_pad = orig
    assert len(calls) == (1 if pad else 0)
    S = float(np.log2(m.encoder.per_level_scale))
    enc = oracle.grid_encode_forward(to_np(xn), to_np(m.encoder.embeddings).astype(np.float16), to_np(m.encoder.offsets), 3, 2, 16, S, 16)
    enc = np.ascontiguousarray(np.transpose(enc, (1, 0, 2)).reshape(B, 32))
    h = oracle.ffmlp_forward(enc, to_np(m.sigma_net.weights).astype(np.float16), 32, 64, 1, 0, training=False)
    ray = np.minimum((np.arange(B) // (64 * T)) * 64 + np.arange(B) % 64, N - 1) if blocked else np.arange(B)
    cin = np.concatenate([_sh16(d)[ray], h[:, 1:], np.broadcast_to(to_np(obj.half())[None], (B, 16)), np.full((B, 1), pad, np.float16)],
                         1).astype(np.float16)
    c = oracle.ffmlp_forward(cin, to_np(m.color_net.weights).astype(np.float16), 48, 64, nl_c, 0, training=False)[:, :3]
    h0_gpu = np.log(to_np(sigma))
    assert_half_close(h0_gpu, h[:, 0], ulps=2.0, atol=1e-4, what="density logit")
    assert (np.abs(h0_gpu - h[:, 0].astype(np.float32)) <= 3e-6 * np.maximum(1, np.abs(h[:, 0].astype(np.float32)))).mean() > 0.97
    rgb_ref = (1.0 / (1.0 + np.exp(-c.astype(np.float32)))).astype(np.float16).astype(np.float32)
    assert_half_close(to_np(rgb), rgb_ref, ulps=2.0, atol=1e-6, what="rgb")
    assert (to_np(rgb) == rgb_ref).mean() > 0.97
    if pad:                                             # the pad is part of the result
        cin[:, 47] = 0
        c0 = oracle.ffmlp_forward(cin, to_np(m.color_net.weights).astype(np.float16), 48, 64, nl_c, 0, training=False)[:, :3]
        assert np.abs(c0.astype(np.float32) - c.astype(np.float32)).max() > 1e-2


# ---------------------------------------------------------------- the network against FOC's network on the drop-in
HASH = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16}
SH = {"otype": "SphericalHarmonics", "degree": 4}


def _mlp(hidden, layers):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": hidden, "n_hidden_layers": layers}


def _foc_network(bound):
    """FOC's tcnn network (nerf/network_tcnn.py: sigma 32 -> 64 -> 16, SH((d + 1) / 2), object feature 144 -> 16 -> 16, colour 47 -> 64 -> 64
    -> 3) on the drop-in's modules, op by op through NeRFRenderer.run — written here on focnerf_amd.renderer.NeRFRenderer (as in
    tests/test_gpu_tcnn.py), not copied."""
    from focnerf_amd import tcnn
    from focnerf_amd.activation import trunc_exp
    from focnerf_amd.renderer import NeRFRenderer

    class FocTcnnNetwork(NeRFRenderer):
        def __init__(self):
            super().__init__(bound, cuda_ray=False, density_scale=1, min_near=0.05)
            self.encoder = tcnn.Encoding(3, dict(HASH, per_level_scale=float(np.exp2(np.log2(2048 * bound / 16) / 15))))
            self.sigma_net = tcnn.Network(32, 16, _mlp(64, 1))
            self.yolo_feat_encoder = tcnn.Network(144, 16, _mlp(16, 1))
            self.encoder_dir = tcnn.Encoding(3, SH)
            self.color_net = tcnn.Network(47, 3, _mlp(64, 2))

        def density(self, x, yolo_details=None):
            h = self.sigma_net(self.encoder((x + self.bound) / (2 * self.bound)))
            return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

        def color(self, x, d, yolo_details=None, mask=None, geo_feat=None, **kwargs):
            obj = self.yolo_feat_encoder(torch.as_tensor(yolo_details[2], device=x.device).unsqueeze(0))
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
            h = torch.cat([self.encoder_dir((d + 1) / 2), geo_feat, obj.squeeze(0).repeat(d.shape[0], 1)], dim=-1)
            rgbs[mask] = torch.sigmoid(self.color_net(h)).to(rgbs.dtype)
            return rgbs

    return FocTcnnNetwork()


def _grads(model):
    """Parameter gradients under tcnn's names and layout."""
    from focnerf_amd.network_tcnn import NeRFNetwork
    if isinstance(model, NeRFNetwork):
        return {"encoder": model.encoder.embeddings.grad.reshape(-1), "sigma_net": model.sigma_net.weights.grad,
                "color_net": model.color_net.weights.grad, "yolo_feat_encoder": model.yolo_feat_encoder.params.grad}
    return {k: getattr(model, k).params.grad for k in ("encoder", "sigma_net", "color_net", "yolo_feat_encoder")}


def _count_calls(monkeypatch, names):
    from focnerf_amd import _lib
    calls = {n: 0 for n in names}
    for n in names:
        orig = getattr(_lib.lib, n)

        def wrap(*a, n=n, orig=orig):
            calls[n] += 1
            return orig(*a)
        monkeypatch.setattr(_lib.lib, n, wrap)
    return calls


def test_network_fused_against_the_dropin_network_and_training(monkeypatch):
    """4096 rays x 512 samples, the same parameters in both: the image within 16 eps, every parameter gradient within 32 eps relative (the
    bounds of tests/test_gpu_tcnn.py::test_foc_topology_run_against_fp32_and_training); the fused entry points ran. Inference agrees within
    the same bound. Twenty Adam steps lower the loss by 10 % at least and stay finite."""
    from focnerf_amd import synthetic
    from focnerf_amd.field import field_plan
    from focnerf_amd.network_tcnn import NeRFNetwork
    torch.manual_seed(0)
    bound = 1
    ref = _foc_network(bound).cuda()
    with torch.no_grad():
        ref.encoder.params.uniform_(-0.5, 0.5)
    net = NeRFNetwork(bound=bound, cuda_ray=False, density_scale=1, min_near=0.05).cuda()
    net.load_state_dict(ref.state_dict(), strict=True)
    plan = field_plan(net)
    assert plan.field and plan.tail and plan.train_forward and plan.infer and plan.colour_input_pad == 1.0
    rays_o, rays_d = synthetic.make_view_rays(64, 64, bound, 1, seed=0, device="cuda")
    rays_o, rays_d = rays_o[0].contiguous(), rays_d[0].contiguous()
    n, T = rays_o.shape[0], 512
    assert n == 4096
    gen = torch.Generator(device="cuda").manual_seed(1)
    feat = torch.rand(144, device="cuda", generator=gen)
    mask = torch.rand(1, n, T, device="cuda", generator=gen) < 0.9
    yolo = (mask, None, feat)
    target = 0.5 + 0.4 * torch.sin(3 * rays_d)
    kw = dict(num_steps=T, upsample_steps=0, bg_color=1.0, perturb=False)

    def step(m, fused):
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.run(rays_o, rays_d, yolo, fused=True, **kw) if fused else m.run(rays_o, rays_d, yolo, **kw)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        (loss * LOSS_SCALE).backward()
        return out["image"].detach().float(), {k: g.detach().float() / LOSS_SCALE for k, g in _grads(m).items()}

    calls = _count_calls(monkeypatch, ["foc_field_forward_train_pad", "foc_color_head_backward_pad", "foc_color_head_forward_pad",
                                       "foc_nerf_field_inference_pad"])
    img_ref, g_ref = step(ref, False)
    img, g = step(net, True)
    assert calls["foc_field_forward_train_pad"] == 1 and calls["foc_color_head_backward_pad"] == 1, calls
    diff = float((img - img_ref).abs().max())
    assert diff <= 16 * FP16_EPS, f"image: max |fused - drop-in| = {diff:.3g}"
    assert float(img_ref.std()) > 1e-2, "degenerate scene"
    for k in g_ref:
        rel = float((g[k] - g_ref[k]).norm() / g_ref[k].norm().clamp_min(1e-30))
        assert float(g_ref[k].norm()) > 0 and rel <= 32 * FP16_EPS, f"{k}: relative gradient error {rel:.3g}"

    # inference
    net.eval()
    ref.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = net.run(rays_o, rays_d, yolo, fused=True, **kw)["image"].float()
        b = ref.run(rays_o, rays_d, yolo, **kw)["image"].float()
    assert calls["foc_nerf_field_inference_pad"] == 1, calls
    diff = float((a - b).abs().max())
    assert diff <= 16 * FP16_EPS, f"inference image: max |fused - drop-in| = {diff:.3g}"

    net.train()
    opt = torch.optim.Adam(net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.run(rays_o, rays_d, yolo, fused=True, num_steps=T, upsample_steps=0, bg_color=1.0, perturb=True)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses) and all(torch.isfinite(p).all() for p in net.parameters())
    assert losses[-1] < 0.9 * losses[0], f"loss {losses[0]:.4g} -> {losses[-1]:.4g}"


def test_dropin_checkpoints_through_load_objects_and_the_combiner(tmp_path):
    """K objects built on the drop-in, saved, loaded with load_objects into the fused class and rendered by the combiner (render_field4: the
    whole-field kernel with the pad) against the drop-in objects' own op-by-op fields under the same select + composite."""
    from focnerf_amd import raymarching as rm
    from focnerf_amd.checkpoint import load_objects, save_checkpoint
    from focnerf_amd.combine import ObjectCombiner, pack_field4
    from focnerf_amd.field import half_cache_scope
    from focnerf_amd.fixedstep import render_field4
    from focnerf_amd.network_tcnn import NeRFNetwork
    from focnerf_amd import synthetic
    K, T = 3, 128
    srcs, paths, feats = [], [], []
    for k in range(K):
        torch.manual_seed(20 + k)
        m = _foc_network(1).cuda()
        with torch.no_grad():
            m.encoder.params.uniform_(-0.5, 0.5)
            m.color_net.params.mul_(1.5)
        p = str(tmp_path / f"obj{k}.pth")
        save_checkpoint(m, p)
        srcs.append(m.eval())
        paths.append(p)
        feats.append(torch.rand(144, device="cuda", generator=torch.Generator(device="cuda").manual_seed(k)))
    objs = load_objects(paths, lambda: NeRFNetwork(bound=1, cuda_ray=False, density_scale=1, min_near=0.05), torch.device("cuda"))
    ro, rd = synthetic.make_view_rays(32, 32, 1, 1, seed=4, device="cuda")
    vo, vd = ro[0].contiguous(), rd[0].contiguous()
    vn, vf = rm.near_far_from_aabb(vo, vd, objs[0].aabb_infer, objs[0].min_near)

    def dropin_field(m, f, lo, hi, out):
        with torch.autocast("cuda", dtype=torch.float16):
            res = m.run(vo[lo:hi][None], vd[lo:hi][None], (None, None, f), num_steps=T, upsample_steps=0, perturb=False, return_fields=True)
        f4 = pack_field4(res['densities'].view(hi - lo, T), res['rgbs'].view(hi - lo, T, 3))
        return f4 if out is None else out.copy_(f4)

    fused = [(lambda lo, hi, out, m=m, f=f: render_field4(m, vo[lo:hi], vd[lo:hi], num_steps=T, yolo_details=(None, None, f), out=out))
             for m, f in zip(objs, feats)]
    ops = [(lambda lo, hi, out, m=m, f=f: dropin_field(m, f, lo, hi, out)) for m, f in zip(srcs, feats)]
    with torch.no_grad(), half_cache_scope():
        img, dep = ObjectCombiner(rank=0, world_size=1).render_view(fused, vo.shape[0], vn, vf, T, max_ray_batch=256)
        img, dep = img.clone(), dep.clone()
        img_ref, dep_ref = ObjectCombiner(rank=0, world_size=1).render_view(ops, vo.shape[0], vn, vf, T, max_ray_batch=256)
    assert float(img_ref.std()) > 1e-2, "degenerate scene"
    diff = float((img - img_ref).abs().max())
    assert diff <= 16 * FP16_EPS, f"combined image: max |fused - drop-in| = {diff:.3g}"
