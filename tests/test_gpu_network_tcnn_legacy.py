"""GPU: torch-ngp's tinycudann network on the fused kernels (focnerf_amd/network_tcnn_legacy.py): column 31 of the 32-wide colour input held
at the pad value (1.0 for tcnn's layout) through the *_pad31 entry points, on the fixed-step path and on the occupancy grid.

  * the colour head with pad 1.0, forward and backward, is bit for bit the plain fused MLP on the materialised 32-wide input with column
    31 = 1.0 (integer-valued data: every sum is exact, so the order of summation cannot show); with pad 0 the twins are the old entry points;
  * foc_field_forward_train_pad31 is bit for bit foc_ffmlp_forward_planar + foc_color_head_forward_pad31 at every layer pair;
  * foc_nerf_field_inference_pad31 against the chain of separate kernels, and with pad 0 bit for bit the old entry point;
  * the occupancy training node against FOC_FUSED_OCC=0 (march, the network's forward, composite_rays_train); its twins with pad 0 are the
    old node; the native inference loop is bit for bit the Python loop;
  * the network against the legacy network written here op by op on the drop-in's modules, in training and inference, fixed-step and
    occupancy; it trains; a checkpoint of the op-by-op module renders the same through the class.
Nothing here reads the reference tree."""
import math

import numpy as np
import pytest
import torch

from oracle import torch_cpu_nerf
from util import assert_half_close, to_np

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -10
LOSS_SCALE = 4096.0
PAIRS = [(1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g, device="cuda").half()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


# ---------------------------------------------------------------- kernels
def _colour_head(fn_fwd, fn_bwd, h, ray_sh, T, W, B, layers, grad, pad):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    st = stream_of(h)
    extra = () if pad is None else (pad,)
    out = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    check(getattr(lib, fn_fwd)(ptr(h), ptr(ray_sh), T, ptr(W), B, 64, layers, 0, ptr(out), 16, None, *extra, st), "fwd")
    grad_h = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    g_w = torch.empty(W.numel(), dtype=torch.float16, device="cuda")
    ws = torch.empty(lib.foc_ffmlp_backward_workspace_bytes(32, 64, layers), dtype=torch.uint8, device="cuda")
    check(getattr(lib, fn_bwd)(ptr(grad), ptr(h), ptr(ray_sh), T, None, ptr(W), B, 64, layers, 0, ptr(grad_h), ptr(g_w), ptr(ws), ws.numel(), 16,
                               None, None, *extra, st), "bwd")
    torch.cuda.synchronize()
    return out, grad_h, g_w


@pytest.mark.parametrize("nlc", [2, 3])
@pytest.mark.parametrize("B", [1, 31, 32, 4097, 1 << 21])
def test_colour_head_pad31_is_the_plain_mlp_on_the_materialised_input(nlc, B):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    g = torch.Generator(device="cuda").manual_seed(100 * nlc + B)
    T = 64 if B % 64 == 0 else 1
    N = B // T
    # integers in {-1, 0, 1}: every activation, delta and product is an integer and the per-tile fp32 sums are exact
    h = _ints(g, (B, 16), -1, 1)
    ray_sh = _ints(g, (N, 16), -1, 1)
    n_w = 64 * (32 + 64 * (nlc - 1) + 16)
    W = _ints(g, (n_w,), -1, 1)
    grad = torch.zeros(B, 16, dtype=torch.float16, device="cuda")
    grad[:, :3] = _ints(g, (B, 3), -1, 1)
    if B > 4096:                                       # about 4096 rows carry a gradient: the weight gradients' sums stay inside fp16's range
        grad[torch.randint(0, B // 4096, (B,), generator=g, device="cuda") != 0] = 0
    out, grad_h, g_w = _colour_head("foc_color_head_forward_pad31", "foc_color_head_backward_pad31", h, ray_sh, T, W, B, nlc, grad, 1.0)

    # the plain fused MLP on [SH16 | h[:,1:16] | 1.0]
    cin = torch.cat([ray_sh.repeat_interleave(T, 0), h[:, 1:], torch.ones(B, 1, dtype=torch.float16, device="cuda")], 1).contiguous()
    st = stream_of(h)
    ref = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    check(lib.foc_ffmlp_forward(ptr(cin), ptr(W), B, 32, 16, 64, nlc, 0, 6, None, ptr(ref), st), "plain fwd")
    g_in = torch.empty(B, 32, dtype=torch.float16, device="cuda")
    g_w_ref = torch.empty(n_w, dtype=torch.float16, device="cuda")
    ws = torch.empty(lib.foc_ffmlp_backward_workspace_bytes(32, 64, nlc), dtype=torch.uint8, device="cuda")
    check(lib.foc_ffmlp_backward(ptr(grad), ptr(cin), ptr(W), None, B, 32, 16, 64, nlc, 0, 6, 1, None, ptr(g_in), ptr(g_w_ref), ptr(ws), ws.numel(), st),
          "plain bwd")
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(g_w.float()).all() and torch.isfinite(g_in.float()).all()
    if B >= 32:
        assert out.float().abs().max() >= 1, "degenerate test data"
    assert torch.equal(_bits(out), _bits(ref)), "logits"
    assert torch.equal(_bits(grad_h[:, 1:]), _bits(g_in[:, 16:31])), "grad_h"
    assert torch.all(grad_h[:, 0] == 0)
    dW0 = g_w[:64 * 32].view(64, 32)
    if B >= 32:
        assert dW0[:, 31].float().abs().max() > 0, "the pad column's gradient is there"
    assert torch.equal(g_w, g_w_ref), "weight gradient (dW0[:, 31] included)"
    nz = g_w_ref != 0
    assert torch.equal(_bits(g_w[nz]), _bits(g_w_ref[nz]))
    # the pad shows: column 31 = 0 gives other logits
    zero = _colour_head("foc_color_head_forward_pad31", "foc_color_head_backward_pad31", h, ray_sh, T, W, B, nlc, grad, 0.0)
    if B >= 32:
        assert not torch.equal(zero[0], out)

    # pad 0: the twins are the old entry points, bit for bit (random data)
    W = (torch.randn(n_w, generator=g, device="cuda") * 0.2).half()
    h = (torch.randn(B, 16, generator=g, device="cuda") * 0.7).half()
    a = _colour_head("foc_color_head_forward_pad31", "foc_color_head_backward_pad31", h, ray_sh, T, W, B, nlc, grad, 0.0)
    b = _colour_head("foc_color_head_forward", "foc_color_head_backward", h, ray_sh, T, W, B, nlc, grad, None)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("B", [1, 4097, 1 << 21])
def test_field_forward_pad31_is_bitwise_the_two_calls(pair, B):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    nls, nlc = pair
    g = torch.Generator(device="cuda").manual_seed(10 * nls + nlc + B)
    T = 7
    n_rays = (B + T - 1) // T
    planes = ((torch.rand(16, B, 2, generator=g, device="cuda") - 0.5) * 2).half()
    w_s = (torch.randn(64 * (32 + 64 * (nls - 1) + 16), generator=g, device="cuda") * 0.25).half()
    w_c = (torch.randn(64 * (32 + 64 * (nlc - 1) + 16), generator=g, device="cuda") * 0.25).half()
    ray_sh = (torch.randn(n_rays, 16, generator=g, device="cuda") * 0.5).half()
    st = stream_of(planes)
    for pad in (1.0, 0.0):
        h1 = torch.empty(B, 16, dtype=torch.float16, device="cuda")
        c1 = torch.empty(B, 4, dtype=torch.float16, device="cuda")
        check(lib.foc_ffmlp_forward_planar(ptr(planes), ptr(w_s), B, 32, 16, 64, nls, 0, 6, ptr(h1), st), "sigma forward")
        check(lib.foc_color_head_forward_pad31(ptr(h1), ptr(ray_sh), T, ptr(w_c), B, 64, nlc, 0, ptr(c1), 4, None, pad, st), "colour forward")
        h2 = torch.full((B + 8, 16), 5.0, dtype=torch.float16, device="cuda")
        c2 = torch.full((B + 8, 4), 5.0, dtype=torch.float16, device="cuda")
        check(lib.foc_field_forward_train_pad31(ptr(planes), ptr(w_s), nls, ptr(ray_sh), T, ptr(w_c), nlc, 64, 0, B, ptr(h2), ptr(c2), 4, None, pad, st),
              "fused forward")
        torch.cuda.synchronize()
        assert torch.all(h2[B:] == 5.0) and torch.all(c2[B:] == 5.0), "rows past B were written"
        assert torch.equal(_bits(h2[:B]), _bits(h1)), "h differs from foc_ffmlp_forward_planar"
        assert torch.equal(_bits(c2[:B]), _bits(c1)), "colour logits differ from foc_color_head_forward_pad31"
        if pad == 0:                                   # pad 0: the old entry point gives the same bits
            c3 = torch.empty(B, 4, dtype=torch.float16, device="cuda")
            check(lib.foc_field_forward_train(ptr(planes), ptr(w_s), nls, ptr(ray_sh), T, ptr(w_c), nlc, 64, 0, B, ptr(h2), ptr(c3), 4, None, st), "old")
            torch.cuda.synchronize()
            assert torch.equal(_bits(c3), _bits(c1))
        else:
            c_pad = c1.clone()
        if B > 1000:
            assert h1.float().abs().max() > 0.5 and c1.float().abs().max() > 0.1, "degenerate test data"
    if B > 1000:
        assert not torch.equal(c_pad, c1), "the pad is part of the result"


def _sh16(dirs):
    return torch.from_numpy(torch_cpu_nerf.sh_encode_deg4(dirs.detach().cpu().float()).numpy().astype(np.float16)).cuda()


@pytest.mark.parametrize("pair", PAIRS)
@pytest.mark.parametrize("blocked", [False, True])
def test_field_inference_pad31_against_the_chain(pair, blocked):
    """foc_nerf_field_inference_pad31 (k_nerf_infer, P31): planes -> sigma net -> [SH | geo | 1.0] -> colour net -> exp / sigmoid, against
    foc_ffmlp_forward_planar -> the materialised row -> foc_ffmlp_inference -> torch's exp / sigmoid."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    nls, nlc = pair
    g = torch.Generator(device="cuda").manual_seed(7 * nls + nlc)
    T = 8
    N = 200 if blocked else 3000
    B = (-(-N // 64) * 64 * T) if blocked else N
    planes = ((torch.rand(16, B, 2, generator=g, device="cuda") - 0.5) * 2).half()
    w_s = (torch.randn(64 * (32 + 64 * (nls - 1) + 16), generator=g, device="cuda") * 0.25).half()
    w_c = (torch.randn(64 * (32 + 64 * (nlc - 1) + 16), generator=g, device="cuda") * 0.25).half()
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g, device="cuda"), dim=-1)
    st = stream_of(planes)

    def infer(fn, *extra):
        sigma = torch.empty(B, dtype=torch.float32, device="cuda")
        rgb = torch.empty(B, 3, dtype=torch.float32, device="cuda")
        check(fn(ptr(planes), 1, ptr(d), T if blocked else 1, 64 if blocked else 0, N, ptr(w_s), nls, ptr(w_c), nlc, 64, 0, B, ptr(sigma), ptr(rgb), None,
                 *extra, st), "inference")
        torch.cuda.synchronize()
        return sigma, rgb

    sigma, rgb = infer(lib.foc_nerf_field_inference_pad31, 1.0)
    h = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    check(lib.foc_ffmlp_forward_planar(ptr(planes), ptr(w_s), B, 32, 16, 64, nls, 0, 6, ptr(h), st), "sigma")
    ray = torch.arange(B, device="cuda")
    if blocked:
        ray = torch.clamp((ray // (64 * T)) * 64 + ray % 64, max=N - 1)
    cin = torch.cat([_sh16(d)[ray], h[:, 1:], torch.ones(B, 1, dtype=torch.float16, device="cuda")], 1).contiguous()
    c = torch.empty(B, 16, dtype=torch.float16, device="cuda")
    check(lib.foc_ffmlp_inference(ptr(cin), ptr(w_c), B, 32, 16, 64, nlc, 0, 6, None, ptr(c), st), "colour")
    torch.cuda.synchronize()
    h0 = to_np(h[:, 0]).astype(np.float32)
    assert_half_close(np.log(to_np(sigma)), h0, ulps=2.0, atol=1e-4, what="density logit")
    rgb_ref = torch.sigmoid(c[:, :3].float()).half().float()
    # the two sum the colour network's products in another order: a logit may round one half-ulp apart, which the sigmoid carries into rgb
    # as up to ~1e-3 where |logit| is near 4 (tests/test_gpu_network_tcnn_layout.py's 2 half-ulps held there for its data, not for these)
    assert float((rgb - rgb_ref).abs().max()) <= 1e-3
    assert (rgb == rgb_ref).float().mean() > 0.97
    # pad 0: the old entry point's bits; and the pad is part of the result
    a = infer(lib.foc_nerf_field_inference_pad31, 0.0)
    b = infer(lib.foc_nerf_field_inference)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    assert (a[1] - rgb).abs().max() > 1e-2


# ---------------------------------------------------------------- the network
HASH = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16}
SH = {"otype": "SphericalHarmonics", "degree": 4}


def _mlp(layers):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": layers}


def _legacy_ops(bound, cuda_ray=True):
    """torch-ngp's tcnn network (legacy/nerf/network_tcnn.py: sigma 32 -> 64 -> 16, SH((d + 1) / 2), colour 31 -> 64 -> 64 -> 3, the input
    padded by the module) on the drop-in's modules, op by op through NeRFRenderer — written here on focnerf_amd.renderer, not copied."""
    from focnerf_amd import tcnn
    from focnerf_amd.activation import trunc_exp
    from focnerf_amd.renderer import NeRFRenderer

    class LegacyTcnnOps(NeRFRenderer):
        def __init__(self):
            super().__init__(bound, cuda_ray=cuda_ray, density_scale=1, min_near=0.05)
            self.encoder = tcnn.Encoding(3, dict(HASH, per_level_scale=float(np.exp2(np.log2(2048 * bound / 16) / 15))))
            self.sigma_net = tcnn.Network(32, 16, _mlp(1))
            self.encoder_dir = tcnn.Encoding(3, SH)
            self.color_net = tcnn.Network(31, 3, _mlp(2))

        def _colour(self, d, geo_feat):
            return torch.sigmoid(self.color_net(torch.cat([self.encoder_dir((d + 1) / 2), geo_feat], dim=-1)))

        def forward(self, x, d):
            field = self.density(x)
            return field['sigma'], self._colour(d, field['geo_feat'])

        def density(self, x):
            h = self.sigma_net(self.encoder((x + self.bound) / (2 * self.bound)))
            return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

        def color(self, x, d, mask=None, geo_feat=None, **kwargs):
            if mask is None:
                return self._colour(d, geo_feat)
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if mask.any():
                rgbs[mask] = self._colour(d[mask], geo_feat[mask]).to(rgbs.dtype)
            return rgbs

        def get_params(self, lr):
            return [{'params': m.parameters(), 'lr': lr} for m in (self.encoder, self.sigma_net, self.encoder_dir, self.color_net)]

    return LegacyTcnnOps()


def _grads(model):
    """Parameter gradients under tcnn's names and layout."""
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    if isinstance(model, NeRFNetwork):
        return {"encoder": model.encoder.embeddings.grad.reshape(-1), "sigma_net": model.sigma_net.weights.grad, "color_net": model.color_net.weights.grad}
    return {k: getattr(model, k).params.grad for k in ("encoder", "sigma_net", "color_net")}


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


def _pair(bound=2, seed=0):
    """The op-by-op module with a non-trivial table and the class holding the same state_dict, both on the analytic occupancy grid."""
    from focnerf_amd import synthetic
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    torch.manual_seed(seed)
    ops = _legacy_ops(bound).cuda()
    with torch.no_grad():
        ops.encoder.params.uniform_(-0.5, 0.5)
    ops.set_density_grid(synthetic.analytic_density_grid(bound, device="cuda"))
    net = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda()
    net.load_state_dict(ops.state_dict(), strict=True)
    return ops, net


def _rays(bound, n, seed, w=64):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(w, w, bound, 1, seed=seed, device="cuda")
    g = torch.Generator().manual_seed(seed)
    pick = torch.randperm(o.shape[1], generator=g)[:n].cuda()
    return o[:, pick].contiguous(), d[:, pick].contiguous()


def _occ_step(m, o, d, seed=7, **kw):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=True, **kw)
        target = 0.5 + 0.5 * torch.sin(3.0 * d)
        loss = torch.nn.functional.mse_loss(out["image"], target) + 1e-3 * out["weights_sum"].mean()
    (loss * LOSS_SCALE).backward()
    torch.cuda.synchronize()
    return out, {k: g.detach().float() / LOSS_SCALE for k, g in _grads(m).items()}


@pytest.mark.parametrize("budget", [False, True])
def test_occupancy_training_node_against_the_chain(budget, monkeypatch):
    """The fused node (the library call with a sample budget, the call-by-call node without) against FOC_FUSED_OCC=0: the same samples
    (the march does not depend on the network: the step counters agree), image / depth / opacity within 4 fp16 eps — the chain's colour
    network sees the pad as an input column, the node as the accumulators' start value, so the two sum in another order — and every
    parameter gradient within 4e-3 of its range (tests/test_gpu_occtrain.py's bound). With pad 0 the twins give the old node's bits (the
    hash-table gradient up to the order of its fp32 sums, which is not fixed from run to run)."""
    from focnerf_amd.field import field_plan
    _, m = _pair()
    m.train()
    plan = field_plan(m)
    assert plan.occ and plan.colour_input_pad == 1.0 and (plan.sigma.num_layers, plan.colour.num_layers) == (1, 2)
    o, d = _rays(2, 1500, 3)
    if budget:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            m.render(o, d, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, force_all_rays=True)
        m.mean_count = int(m.step_counter[(m.local_step - 1) % 16, 0]) + 500
    kw = dict(force_all_rays=not budget, bg_color=None)
    calls = _count_calls(monkeypatch, ["foc_occ_train_forward_pad31", "foc_occ_train_backward_pad31", "foc_color_head_forward_pad31",
                                       "foc_color_head_backward_pad31"])
    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    ref, g_ref = _occ_step(m, o, d, **kw)
    counter_ref = m.step_counter[(m.local_step - 1) % 16].clone()
    assert sum(calls.values()) == 0
    monkeypatch.setenv("FOC_FUSED_OCC", "1")
    got, g_got = _occ_step(m, o, d, **kw)
    counter_got = m.step_counter[(m.local_step - 1) % 16].clone()
    if budget:
        assert calls["foc_occ_train_forward_pad31"] == 1 and calls["foc_occ_train_backward_pad31"] == 1, calls
    else:
        assert calls["foc_color_head_forward_pad31"] == 1 and calls["foc_color_head_backward_pad31"] == 1, calls
    assert torch.equal(counter_ref, counter_got) and int(counter_got[0]) > 1000
    for k in ("image", "depth", "weights_sum"):
        diff = float((ref[k] - got[k]).detach().abs().max())
        assert diff <= 4 * FP16_EPS, f"{k}: max |fused - chain| = {diff:.3g}"
    assert float(ref["weights_sum"].max()) > 0.5
    for k in g_ref:
        scale = float(g_ref[k].abs().max())
        err = float((g_ref[k] - g_got[k]).abs().max())
        assert scale > 0 and err <= 4e-3 * scale, f"grad {k} off by {err / scale:.2e} of its range"

    # pad 0 through the twins (the node's, and the colour head's on the call-by-call node) against the old entry points, bit for bit
    from focnerf_amd import _lib
    monkeypatch.setattr(m, "colour_input_pad", 0.0, raising=False)
    old, g_old = _occ_step(m, o, d, **kw)
    for name in ("foc_occ_train_forward", "foc_occ_train_backward", "foc_color_head_forward", "foc_color_head_backward"):
        twin = getattr(_lib.lib, name + "_pad31")                     # the twin's signature: the old one with the pad before the stream
        monkeypatch.setattr(_lib.lib, name, lambda *a, _t=twin: _t(*a[:-1], 0.0, a[-1]))
    new, g_new = _occ_step(m, o, d, **kw)
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(_bits(old[k]), _bits(new[k])), k
    for k in ("sigma_net", "color_net"):
        assert torch.equal(g_old[k], g_new[k]), k
    # the hash-table gradient's fp32 sums have no fixed order from run to run (bench.py's hash-grid gradient sample moves the same way)
    err, scale = float((g_old["encoder"] - g_new["encoder"]).abs().max()), float(g_old["encoder"].abs().max())
    assert scale > 0 and err <= 4e-3 * scale, f"grad encoder off by {err / scale:.2e} of its range"
    assert not torch.equal(old["image"], got["image"])


def test_native_inference_loop_is_the_python_loop(monkeypatch):
    """run_cuda in inference: the native loop (foc_occ_render_step_pad31) against the Python loop with the reference's boolean-mask
    compaction on the same network — image and depth bit for bit; with pad 0 the step's twin is the old step."""
    _, m = _pair(seed=4)
    m.eval()
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(40, 40, 2, 1, seed=6, device="cuda")
    kw = dict(staged=False, dt_gamma=1 / 128, max_steps=1024, bg_color=1.0, T_thresh=1e-4, perturb=False)
    calls = _count_calls(monkeypatch, ["foc_occ_render_step_pad31", "foc_occ_render_step"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = m.render(o, d, device_compaction=False, **kw)
        assert sum(calls.values()) == 0
        b = m.render(o, d, device_compaction=True, **kw)
        assert calls["foc_occ_render_step_pad31"] > 0 and calls["foc_occ_render_step"] == 0, calls
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth"], b["depth"])
        assert float(b["image"].std()) > 1e-2
        from focnerf_amd import _lib
        monkeypatch.setattr(m, "colour_input_pad", 0.0, raising=False)
        c = m.render(o, d, device_compaction=True, **kw)
        twin = _lib.lib.foc_occ_render_step_pad31
        monkeypatch.setattr(_lib.lib, "foc_occ_render_step", lambda *a: twin(*a[:-1], 0.0, a[-1]))
        e = m.render(o, d, device_compaction=True, **kw)
    assert torch.equal(c["image"], e["image"]) and torch.equal(c["depth"], e["depth"])
    assert not torch.equal(c["image"], b["image"])


def test_network_against_the_op_by_op_module(monkeypatch):
    """The same parameters in the class and in the op-by-op module: fixed-step (run(fused=True), 4096 rays x 256 samples) and occupancy
    (render) paths, in training and inference — the image within 16 fp16 eps, every parameter gradient within 32 eps relative (the bounds
    of tests/test_gpu_network_tcnn_layout.py); the fused entry points ran."""
    from focnerf_amd import synthetic
    ops, net = _pair()
    rays_o, rays_d = synthetic.make_view_rays(64, 64, 2, 1, seed=0, device="cuda")
    rays_o, rays_d = rays_o[0].contiguous(), rays_d[0].contiguous()
    target = 0.5 + 0.4 * torch.sin(3 * rays_d)
    calls = _count_calls(monkeypatch, ["foc_field_forward_train_pad31", "foc_color_head_backward_pad31", "foc_nerf_field_inference_pad31",
                                       "foc_occ_train_forward_pad31", "foc_occ_render_step_pad31"])

    def train_step(m, fused, occ):
        m.train()
        m.zero_grad(set_to_none=True)
        torch.manual_seed(5)
        with torch.autocast("cuda", dtype=torch.float16):
            if occ:
                out = m.render(rays_o[None], rays_d[None], staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=1.0)
            elif fused:
                out = m.run(rays_o, rays_d, None, fused=True, num_steps=256, upsample_steps=0, bg_color=1.0, perturb=False)
            else:
                out = m.run(rays_o, rays_d, None, num_steps=256, upsample_steps=0, bg_color=1.0, perturb=False)
            loss = torch.nn.functional.mse_loss(out["image"].float().view(-1, 3), target)
        (loss * LOSS_SCALE).backward()
        return out["image"].detach().float().view(-1, 3), {k: g.detach().float() / LOSS_SCALE for k, g in _grads(m).items()}

    for occ in (False, True):
        img_ref, g_ref = train_step(ops, False, occ)
        img, g = train_step(net, True, occ)
        diff = float((img - img_ref).abs().max())
        assert diff <= 16 * FP16_EPS, f"occ={occ}: image max |fused - ops| = {diff:.3g}"
        assert float(img_ref.std()) > 1e-2, "degenerate scene"
        for k in g_ref:
            rel = float((g[k] - g_ref[k]).norm() / g_ref[k].norm().clamp_min(1e-30))
            assert float(g_ref[k].norm()) > 0 and rel <= 32 * FP16_EPS, f"occ={occ}: {k}: relative gradient error {rel:.3g}"
    assert calls["foc_field_forward_train_pad31"] == 1 and calls["foc_color_head_backward_pad31"] >= 1, calls

    net.eval()
    ops.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = net.run(rays_o, rays_d, None, fused=True, num_steps=256, upsample_steps=0, bg_color=1.0, perturb=False)["image"].float()
        b = ops.run(rays_o, rays_d, None, num_steps=256, upsample_steps=0, bg_color=1.0, perturb=False)["image"].float()
        assert float((a - b).abs().max()) <= 16 * FP16_EPS, "fixed-step inference"
        a = net.render(rays_o[None], rays_d[None], staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=1.0)["image"].float()
        b = ops.render(rays_o[None], rays_d[None], staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=1.0)["image"].float()
        assert float((a - b).abs().max()) <= 16 * FP16_EPS, "occupancy inference"
    assert calls["foc_nerf_field_inference_pad31"] >= 1 and calls["foc_occ_render_step_pad31"] >= 1, calls


def test_training_on_the_occupancy_grid_and_checkpoints(tmp_path):
    """Three hundred Adam steps on the synthetic scene on the occupancy grid, the density grid updated every 16 steps (the legacy trainer's
    schedule), lower the loss; a checkpoint saved from the op-by-op module renders the same through the class."""
    from focnerf_amd import synthetic
    from focnerf_amd.checkpoint import load_checkpoint, save_checkpoint
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    torch.manual_seed(0)
    bound = 1
    net = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda().train()
    o, d = synthetic.make_view_rays(48, 48, bound, 1, seed=1, device="cuda")
    target = (0.5 + 0.4 * torch.sin(3 * d)).float()
    opt = torch.optim.Adam(net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    losses = []
    for it in range(300):
        if it % 16 == 0:
            with torch.autocast("cuda", dtype=torch.float16):
                net.update_extra_state()
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.render(o, d, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=True, bg_color=1.0)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses) and all(torch.isfinite(p).all() for p in net.parameters())
    assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:10]), f"loss {np.mean(losses[:10]):.4g} -> {np.mean(losses[-10:]):.4g}"

    # a checkpoint of the op-by-op module, rendered through the class (occupancy grid, native loop) and by the module itself
    ops, _ = _pair(bound=bound, seed=9)
    path = str(tmp_path / "legacy_ops.pth")
    save_checkpoint(ops, path)
    other = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05).cuda()
    assert load_checkpoint(other, path) == ([], [])
    other.eval()
    ops.eval()
    ro, rd = synthetic.make_view_rays(40, 40, bound, 1, seed=2, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = other.render(ro, rd, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=1.0)["image"].float()
        b = ops.render(ro, rd, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=1.0)["image"].float()
    assert float(b.std()) > 1e-2
    assert float((a - b).abs().max()) <= 16 * FP16_EPS, f"checkpoint render: max |class - ops| = {float((a - b).abs().max()):.3g}"
