"""GPU: torch-ngp's default network (focnerf_amd/network_linear.py: bias-free nn.Linear layers, packed into FFMLP blobs for the kernels)
and its background model (csrc/background.hip).

  * the background kernel against the reference's background() body on this package's ops under autocast, over ragged N up to 640 000:
    rgb within a few fp16 ulps, its weight gradients bit-identical from run to run, the table gradient against an fp32 restatement, the
    inference form and the coordinates form bit for bit the training form;
  * the network on the fused kernels against its own op route (every FOC_FUSED_* switch off: nn.Linear on the drop-in encoders), fixed
    step and occupancy grid, background off and on: image, loss and every parameter gradient, encoder_bg and bg_net included;
  * the native occupancy loop is bit for bit the Python loop with the background on;
  * cpu_network.npz (made by the reference's nerf/network.py class on the CPU) replayed through the class in fp32 on the GPU;
  * training with the background through the fused path; a checkpoint of the op route renders the same through the fused route.
Nothing here reads the reference tree."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FP16_EPS = 2.0 ** -10
LOSS_SCALE = 4096.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OP_ROUTE = ("FOC_FUSED_FIELD", "FOC_FUSED_TAIL", "FOC_FUSED_INFER", "FOC_FUSED_OCC", "FOC_FUSED_HEAD", "FOC_RENDER_NATIVE", "FOC_FUSED_BG")


def _net(bg=32.0, bound=2, seed=0, cuda_ray=True):
    from focnerf_amd import synthetic
    from focnerf_amd.network_linear import NeRFNetwork
    torch.manual_seed(seed)
    m = NeRFNetwork(bound=bound, cuda_ray=cuda_ray, density_scale=1, min_near=0.05, bg_radius=bg).cuda()
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-0.5, 0.5)
        # nn.Linear's default initialisation leaves sigma ~ 1 and every colour ~ 0.5 (an image std of 4e-3 on the fixed-step view): three
        # times larger weights give densities and colours that vary from ray to ray, so that the comparisons below can see a difference
        for layer in list(m.sigma_net) + list(m.color_net):
            layer.weight.mul_(3.0)
        if bg > 0:
            m.encoder_bg.embeddings.uniform_(-1.0, 1.0)
    if cuda_ray:
        m.set_density_grid(synthetic.analytic_density_grid(bound, device="cuda"))
    return m


def _op_route(monkeypatch, on):
    for k in OP_ROUTE:
        monkeypatch.setenv(k, "1" if on else "0")


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


def _rays(N, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    o = (torch.rand(N, 3, generator=g, device="cuda") * 2 - 1) * 0.9
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g, device="cuda"), dim=-1)
    return o.contiguous(), d.contiguous()


def _op_chain(m, o, d):
    """legacy/nerf/network.py:145-160 after sph_from_ray (legacy/nerf/renderer.py:232-234), written here on this package's modules."""
    from focnerf_amd import raymarching
    x = raymarching.sph_from_ray(o, d, m.bg_radius)
    h = m.encoder_bg(x)
    h = torch.cat([m.encoder_dir(d), h], dim=-1)
    h = torch.nn.functional.relu(m.bg_net[0](h))
    return torch.sigmoid(m.bg_net[1](h))


def _bg_grads(m):
    return m.encoder_bg.embeddings.grad.clone(), m.bg_net[0].weight.grad.clone(), m.bg_net[1].weight.grad.clone()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 4095, 4096, 4097, 640000])
def test_background_kernel_against_the_op_chain(N, monkeypatch):
    from focnerf_amd import raymarching
    from focnerf_amd.background import background_rgb
    from focnerf_amd.field import field_plan
    m = _net(cuda_ray=False)
    assert field_plan(m).background
    o, d = _rays(N, N)
    g = (torch.rand(N, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) - 0.5).half()
    calls = _count_calls(monkeypatch, ["foc_background_forward", "foc_background_backward"])

    def fused():
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            rgb = background_rgb(m, d, rays_o=o, radius=m.bg_radius)
        rgb.backward(g)
        return rgb.detach(), _bg_grads(m)

    rgb, (g_emb, g_w0, g_w1) = fused()
    assert rgb.dtype == torch.float16 and rgb.shape == (N, 3)
    assert calls == {"foc_background_forward": 1, "foc_background_backward": 1}
    # a second run: the weight gradients are the same bits (fixed-order sums); the table's fp32 atomics are not ordered
    rgb2, (g_emb2, g_w0b, g_w1b) = fused()
    assert torch.equal(rgb, rgb2) and torch.equal(g_w0, g_w0b) and torch.equal(g_w1, g_w1b)
    assert float((g_emb - g_emb2).abs().max()) <= 1e-4 * max(float(g_emb.abs().max()), 1e-30)

    # the op chain under autocast
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        ref = _op_chain(m, o, d)
    ref.backward(g)
    r_emb, r_w0, r_w1 = _bg_grads(m)
    ref = ref.detach()
    diff = float((rgb.float() - ref.float()).abs().max())
    assert diff <= 4 * FP16_EPS, f"rgb: max |kernel - op chain| = {diff:.3g}"
    if N >= 4096:
        assert float(ref.float().std()) > 1e-2, "degenerate background"
    for name, a, b in (("bg_net.0", g_w0, r_w0), ("bg_net.1", g_w1, r_w1), ("encoder_bg", g_emb, r_emb)):
        rel = float((a - b).norm() / b.norm().clamp_min(1e-30))
        assert float(b.norm()) > 0 and rel <= 16 * FP16_EPS, f"{name}: relative gradient distance to the op chain {rel:.3g}"

    # the table gradient against an fp32 restatement (the op chain without autocast: fp32 table, fp32 atomics, fp32 GEMMs)
    m.zero_grad(set_to_none=True)
    _op_chain(m, o, d).backward(g.float())
    f_emb = m.encoder_bg.embeddings.grad
    rel = float((g_emb - f_emb).norm() / f_emb.norm().clamp_min(1e-30))
    assert rel <= 16 * FP16_EPS, f"table gradient: relative distance to the fp32 restatement {rel:.3g}"

    # inference form and coordinates form: the training form's bits
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        inf = background_rgb(m, d, rays_o=o, radius=m.bg_radius)
        via = m.background(raymarching.sph_from_ray(o, d, m.bg_radius), d)
    assert torch.equal(inf, rgb) and torch.equal(via, rgb)


def _train_step(m, o, d, target, occ, fused, bg_color=1.0):
    m.train()
    m.zero_grad(set_to_none=True)
    torch.manual_seed(5)
    with torch.autocast("cuda", dtype=torch.float16):
        if occ:
            out = m.render(o[None], d[None], staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, bg_color=bg_color)
        else:
            out = m.run(o, d, None, fused=fused, num_steps=256, upsample_steps=0, bg_color=bg_color, perturb=False)
        loss = torch.nn.functional.mse_loss(out["image"].float().view(-1, 3), target)
    (loss * LOSS_SCALE).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().float() / LOSS_SCALE for k, p in m.named_parameters() if p.grad is not None}
    return out["image"].detach().float().view(-1, 3), float(loss), out["depth"].detach().float().reshape(-1), grads


@pytest.mark.parametrize("bg", [-1.0, 32.0])
@pytest.mark.parametrize("occ", [False, True])
def test_network_fused_against_the_op_route(bg, occ, monkeypatch):
    """Image within 16 fp16 eps, depth within 16 eps (fixed step) and every parameter gradient within 32 eps relative — the bounds of
    tests/test_gpu_network_tcnn_legacy.py; the fused entry points ran."""
    from focnerf_amd import synthetic
    m = _net(bg=bg)
    o, d = synthetic.make_view_rays(64, 64, 2, 1, seed=0, device="cuda")
    o, d = o[0].contiguous(), d[0].contiguous()
    target = 0.5 + 0.4 * torch.sin(3 * d)
    _op_route(monkeypatch, False)
    img_ref, loss_ref, depth_ref, g_ref = _train_step(m, o, d, target, occ, fused=False)
    _op_route(monkeypatch, True)
    calls = _count_calls(monkeypatch, ["foc_background_forward", "foc_background_backward", "foc_field_forward_train", "foc_color_head_backward"])
    img, loss, depth, g = _train_step(m, o, d, target, occ, fused=True)
    if not occ:
        assert calls["foc_field_forward_train"] == 1, calls
    assert calls["foc_color_head_backward"] >= 1, calls
    if bg > 0:
        assert calls["foc_background_forward"] == 1 and calls["foc_background_backward"] == 1, calls
        assert {"encoder_bg.embeddings", "bg_net.0.weight", "bg_net.1.weight"} <= set(g)
    assert set(g) == set(g_ref)
    diff = float((img - img_ref).abs().max())
    assert diff <= 16 * FP16_EPS, f"image: max |fused - op route| = {diff:.3g}"
    assert float(img_ref.std()) > 1e-2, "degenerate scene"
    assert abs(loss - loss_ref) <= 16 * FP16_EPS * max(loss_ref, 1e-3)
    if not occ:
        assert float((depth - depth_ref).abs().max()) <= 16 * FP16_EPS
    for k in g_ref:
        rel = float((g[k] - g_ref[k]).norm() / g_ref[k].norm().clamp_min(1e-30))
        assert float(g_ref[k].norm()) > 0 and rel <= 32 * FP16_EPS, f"{k}: relative gradient distance {rel:.3g}"


def test_native_loop_is_the_python_loop_with_the_background(monkeypatch):
    from focnerf_amd import synthetic
    from focnerf_amd.field import field_plan
    m = _net(seed=4)
    m.eval()
    plan = field_plan(m)
    assert plan.native_loop and plan.background and plan.occ
    o, d = synthetic.make_view_rays(40, 40, 2, 1, seed=6, device="cuda")
    kw = dict(staged=False, dt_gamma=1 / 128, max_steps=1024, bg_color=1.0, T_thresh=1e-4, perturb=False)
    calls = _count_calls(monkeypatch, ["foc_occ_render_step", "foc_background_forward"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = m.render(o, d, device_compaction=False, **kw)
        assert calls["foc_occ_render_step"] == 0
        b = m.render(o, d, device_compaction=True, **kw)
    assert calls["foc_occ_render_step"] > 0 and calls["foc_background_forward"] == 2, calls
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["depth"], b["depth"])
    assert float(b["image"].std()) > 1e-2


def test_fixed_step_inference_and_staged_render_with_the_background(monkeypatch):
    """Whole-field inference (run(fused=True)) and render(staged=True), which takes the background per chunk, against the op route."""
    from focnerf_amd import synthetic
    m = _net(seed=2, cuda_ray=False)
    m.eval()
    o, d = synthetic.make_view_rays(48, 48, 2, 1, seed=3, device="cuda")
    calls = _count_calls(monkeypatch, ["foc_nerf_field_inference", "foc_background_forward"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        a = m.run(o[0], d[0], None, fused=True, num_steps=128, upsample_steps=0, perturb=False)["image"].float()
        s = m.render(o, d, staged=True, max_ray_batch=512, fused=True, num_steps=128, upsample_steps=0, perturb=False, return_fields=False)
        _op_route(monkeypatch, False)
        b = m.run(o[0], d[0], None, num_steps=128, upsample_steps=0, perturb=False)["image"].float()
    assert calls["foc_nerf_field_inference"] >= 2 and calls["foc_background_forward"] >= 2, calls
    assert float((a - b).abs().max()) <= 16 * FP16_EPS, f"fixed-step inference: {float((a - b).abs().max()):.3g}"
    assert float((s["image"][0].float() - a).abs().max()) <= 1e-6, "staged render == one chunk"


def test_cpu_network_fixture_replays_on_the_gpu(monkeypatch):
    """cpu_network.npz: the reference's nerf/network.py class on the CPU with a small hash grid (8 levels, 2^12 rows). The class loads its
    parameters with strict=True and its op path in fp32 on the GPU reproduces the evaluation image, depth and weights_sum within 1e-4, and
    the training loss within 1e-4 relative and every gradient within 1e-3 relative."""
    from focnerf_amd import network_linear
    from focnerf_amd.encoding import get_encoder
    g = np.load(os.path.join(GOLDEN, "cpu_network.npz"))
    nl, base, log2, des = (int(v) for v in g["encoder_cfg"])
    small = dict(num_levels=nl, base_resolution=base, log2_hashmap_size=log2, desired_resolution=des)
    monkeypatch.setattr(network_linear, "get_encoder", lambda enc, **kw: get_encoder(enc, **{**kw, **(small if enc == "hashgrid" else {})}))
    bound, T = int(g["bound"]), int(g["T"])
    m = network_linear.NeRFNetwork(bound=bound)
    m.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}, strict=True)
    m = m.cuda()
    o, d = torch.from_numpy(g["rays_o"]).cuda(), torch.from_numpy(g["rays_d"]).cuda()
    m.eval()
    with torch.no_grad():
        ev = m.run(o[None], d[None], None, num_steps=T, upsample_steps=0, bg_color=None, perturb=False)
    for k, ref in (("image", g["eval_image"]), ("depth", g["eval_depth"]), ("weights_sum", g["eval_weights_sum"])):
        got = ev[k].reshape(ref.shape).cpu().numpy()
        # a ray that misses the box has a NaN depth in the reference's run (nerf/renderer.py): the same rays are NaN here
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"eval {k}: NaN at other rays"
        hit = ~np.isnan(ref)
        assert np.abs(got[hit] - ref[hit]).max() <= 1e-4, f"eval {k}: max diff {np.abs(got[hit] - ref[hit]).max():.3g}"
    m.train()
    N = o.shape[0]
    tr = m.run(o[None], d[None], (torch.ones(1, N, T, dtype=torch.bool, device="cuda"), None, None), num_steps=T, upsample_steps=0, bg_color=None,
               perturb=False)
    ok = torch.isfinite(tr["depth"][0])
    target = torch.from_numpy(g["train_target"]).cuda()
    loss = torch.nn.functional.mse_loss(tr["image"][0][ok], target[ok])
    loss.backward()
    assert abs(float(loss) - float(g["train_loss"])) <= 1e-4 * float(g["train_loss"])
    grads = {"grad_embeddings": m.encoder.embeddings.grad}
    grads.update({f"grad_sigma_net_{i}": l.weight.grad for i, l in enumerate(m.sigma_net)})
    grads.update({f"grad_color_net_{i}": l.weight.grad for i, l in enumerate(m.color_net)})
    for k, v in grads.items():
        ref = torch.from_numpy(g[k]).cuda()
        rel = float((v - ref).norm() / ref.norm().clamp_min(1e-30))
        assert rel <= 1e-3, f"{k}: relative distance {rel:.3g}"


def test_training_with_the_background_and_checkpoints(tmp_path, monkeypatch):
    """300 Adam steps on the synthetic scene on the occupancy grid with the background model, through the fused path and through the op
    route from the same start: both lower the loss by half, the fused curve's last losses stay within 25 % of the op route's, and the
    GradScaler never meets an inf or NaN (its scale stays put). A checkpoint saved from the op route renders the same through the fused
    route (16 fp16 eps)."""
    from focnerf_amd import synthetic
    from focnerf_amd.network_linear import NeRFNetwork
    bound = 1
    o, d = synthetic.make_view_rays(48, 48, bound, 1, seed=1, device="cuda")
    target = (0.5 + 0.4 * torch.sin(3 * d)).float()

    def train(fused):
        _op_route(monkeypatch, fused)
        torch.manual_seed(0)
        net = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05, bg_radius=4.0).cuda().train()
        opt = torch.optim.Adam(net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        scaler = torch.amp.GradScaler("cuda", init_scale=LOSS_SCALE)
        losses = []
        for it in range(300):
            if it % 16 == 0:
                with torch.autocast("cuda", dtype=torch.float16):
                    net.update_extra_state()
            with torch.autocast("cuda", dtype=torch.float16):
                out = net.render(o, d, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=True)
                loss = torch.nn.functional.mse_loss(out["image"].float(), target)
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            losses.append(float(loss.detach()))
        assert scaler.get_scale() == LOSS_SCALE, "GradScaler met an inf or NaN"
        return net, losses

    net, fused = train(True)
    ops, ref = train(False)
    for losses in (fused, ref):
        assert all(math.isfinite(v) for v in losses)
        assert np.mean(losses[-10:]) < 0.5 * np.mean(losses[:10]), f"loss {np.mean(losses[:10]):.4g} -> {np.mean(losses[-10:]):.4g}"
    assert abs(np.mean(fused[-20:]) - np.mean(ref[-20:])) <= 0.25 * np.mean(ref[-20:]), (np.mean(fused[-20:]), np.mean(ref[-20:]))

    path = str(tmp_path / "op_route.pth")
    torch.save({"model": ops.state_dict()}, path)
    other = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1, min_near=0.05, bg_radius=4.0).cuda()
    other.load_state_dict(torch.load(path)["model"], strict=True)
    other.eval()
    ops.eval()
    ro, rd = synthetic.make_view_rays(40, 40, bound, 1, seed=2, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        _op_route(monkeypatch, True)
        a = other.render(ro, rd, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False)["image"].float()
        _op_route(monkeypatch, False)
        b = ops.render(ro, rd, staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False)["image"].float()
    assert float(b.std()) > 1e-2
    assert float((a - b).abs().max()) <= 16 * FP16_EPS, f"checkpoint render: max |fused - op route| = {float((a - b).abs().max()):.3g}"
