"""GPU: deterministic mode (the library switch FOC_DETERMINISTIC, include/focnerf.h "Deterministic mode").

Every case runs a passing computation a fixed, small number of times and compares bits:
  1. the binned grid backward with many chunks per (level, segment) slot: three calls agree bit for bit and stay inside the bound
     tests/test_gpu_gridencoder.py states against the fp32-summed oracle; the default mode's spread is printed, not asserted;
  2. with run merging off the gradient does not depend on the order of the samples either;
  3. one chunk per slot: the mode changes no bit;
  4. eight optimizer steps of four networks, twice from one seed: every parameter, every loss and the occupancy state agree;
  5. the headline step replayed as a HIP graph gives the eager step's parameters;
  6. the entry points without a deterministic form refuse with a RuntimeError naming the option, and run as before with it off; the ones
     that got a form (background, density-grid mean, split-K MLP weight gradient) repeat bit for bit and keep their accuracy bounds.
Bounds that are not another test's are derived where they are stated."""
import numpy as np
import pytest
import torch

import oracle
from util import to_np
import test_gpu_gridencoder as tge
import test_gpu_network_linear as tnl

pytestmark = pytest.mark.gpu

OPT = "FOC_DETERMINISTIC"
FOC_GRID = (3, 2, 16, 16, 19, 2048)          # D, C, L, H, log2 table size, finest resolution: FOC's encoder (tests/test_gpu_gridencoder.py CASES[0])


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))       # bit patterns: NaN-safe, -0.0 != 0.0


def _grid_case(B, seed=3):
    D, C, L, H, lh, desired = FOC_GRID
    pls, S, off, table = tge._setup(D, C, L, H, lh, desired, seed, np.float16)
    x = tge._points(B, D, seed + 1, oob=False)
    grad = (np.random.default_rng(seed + 6).standard_normal((L, B, C)) * 0.1).astype(np.float16)
    return S, off, table, x, grad


def _grid_backward(S, off, table, xt, gt):
    D, C, L, H, _, _ = FOC_GRID
    B = xt.shape[0]
    tt, ot = torch.from_numpy(table).cuda(), torch.from_numpy(off).cuda()
    ge = torch.zeros(int(off[-1]), C, dtype=torch.float16, device="cuda")
    tge._be().grid_encode_backward(gt, xt, tt, ot, ge, B, D, C, L, S, H, None, None, 0, False, 0)
    torch.cuda.synchronize()
    return ge


def test_many_chunks_per_slot_repeat_bit_for_bit(lib_option):
    D, C, L, H, _, _ = FOC_GRID
    B = 1 << 20
    S, off, table, x, grad = _grid_case(B)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(grad).cuda()
    # 2^20 points give 4 * 2^20 records on a level (one segment on the coarse ones): up to 128 chunks of 32768 records per slot
    lib_option(OPT, 0)
    off_runs = [_grid_backward(S, off, table, xt, gt) for _ in range(3)]
    spread = max(float((off_runs[0].float() - r.float()).abs().max()) for r in off_runs[1:])
    print(f"\nFOC_DETERMINISTIC=0: largest |difference| between three calls {spread:.3e} "
          f"(elements that differ: {int((_bits(off_runs[0]) != _bits(off_runs[1])).sum())} of {off_runs[0].numel()})")
    lib_option(OPT, 1)
    runs = [_grid_backward(S, off, table, xt, gt) for _ in range(3)]
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])
    lib_option(OPT, 2)                                     # the per-chunk-plane variant sums the same integers: the same bits
    assert _same(runs[0], _grid_backward(S, off, table, xt, gt))
    # the bound of tests/test_gpu_gridencoder.py::test_backward for the binned path, against the same (half-valued) gradients summed in fp32
    want32 = oracle.grid_encode_backward(grad.astype(np.float32), x, off, int(off[-1]), D, C, L, S, H, None, 0, False, 0).astype(np.float32)
    got = to_np(runs[0]).astype(np.float32)
    err = np.abs(got - want32).max()
    print(f"FOC_DETERMINISTIC=1: max |grad - fp32-summed oracle| {err:.3e} (bound {2e-3 * np.abs(want32).max() + 1e-3:.3e}); "
          f"default mode {np.abs(to_np(off_runs[0]).astype(np.float32) - want32).max():.3e}")
    assert err <= 2e-3 * np.abs(want32).max() + 1e-3, err


def test_sample_order_does_not_matter_without_run_merging(lib_option):
    B = 1 << 20
    S, off, table, x, grad = _grid_case(B, seed=11)
    lib_option(OPT, 1)
    lib_option("FOC_GB_MERGE_MAX_RES", 0)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(grad).cuda()
    a = _grid_backward(S, off, table, xt, gt)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(5)).cuda()
    b = _grid_backward(S, off, table, xt[perm].contiguous(), gt[:, perm].contiguous())
    assert float(a.float().abs().max()) > 0
    assert _same(a, b)


def test_one_chunk_per_slot_gives_the_default_bits(lib_option):
    B = 4096                                               # at most 4 * 4096 = 16384 records per level: no slot has a second chunk
    S, off, table, x, grad = _grid_case(B, seed=21)
    xt, gt = torch.from_numpy(x).cuda(), torch.from_numpy(grad).cuda()
    lib_option(OPT, 0)
    a = _grid_backward(S, off, table, xt, gt)
    lib_option(OPT, 1)
    b = _grid_backward(S, off, table, xt, gt)
    assert float(a.float().abs().max()) > 0 and _same(a, b)


# ---------------------------------------------------------------- whole steps
T_STEPS = 256                                              # samples per ray: 4096 x 256 points per step, 32 - 128 chunks on the coarse slots
N_OPT_STEPS = 8


def _adam(model, **kw):
    return torch.optim.Adam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True, **kw)


def _batches(n, seed):
    import bench
    dev = torch.device("cuda", 0)
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=seed)
    gen = torch.Generator().manual_seed(seed)
    return [bench.sample_batch(poses, intr, dev, gen) for _ in range(n)]


def _fixed_step(kind):
    import bench
    dev = torch.device("cuda", 0)

    def run():
        torch.manual_seed(0)
        yolo = None
        if kind == "network":
            m = bench.build_model(2, dev, cuda_ray=False, seed=0).train()
        elif kind == "network_foc":
            m = bench.build_foc_model(2, dev, seed=0).train()
            yolo = bench.foc_yolo_details(dev, bench.NUM_RAYS, 7)
        else:
            m = tnl._net(bg=32.0, cuda_ray=False, seed=0).train()
            assert m.bg_radius > 0
        opt, scaler = _adam(m), torch.amp.GradScaler("cuda")
        torch.manual_seed(1234)                            # the perturbation noise of the steps
        losses = []
        for o, d, t in _batches(N_OPT_STEPS, 3):
            opt.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.render(o, d, yolo, staged=False, num_steps=T_STEPS, upsample_steps=0, perturb=True, bg_color=None, fused=True)
                loss = torch.nn.functional.mse_loss(out["image"], t)
                if out.get("criterion_outside_mask") is not None:
                    loss = loss + 1e-8 * out["criterion_outside_mask"]
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}, losses, {}
    return run


def _occupancy():
    import bench
    dev = torch.device("cuda", 0)

    def run():
        torch.manual_seed(0)
        m = bench.build_model(2, dev, cuda_ray=True, seed=0).train()
        opt, scaler = _adam(m), torch.amp.GradScaler("cuda")
        torch.manual_seed(1234)
        losses = []
        for i, (o, d, t) in enumerate(_batches(N_OPT_STEPS, 4)):
            losses.append(bench.cuda_ray_train_step(m, opt, scaler, o, d, t).detach().clone())
            if i in (2, 5):
                if i == 5:
                    m.iter_density = 16                    # the second update takes the steady-state branch (random and occupied cells)
                with torch.autocast("cuda", dtype=torch.float16):
                    m.update_extra_state()
        torch.cuda.synchronize()
        extra = {"density_grid": m.density_grid.clone(), "density_bitfield": m.density_bitfield.clone(), "step_counter": m.step_counter.clone(),
                 "mean_density": torch.tensor(float(m.mean_density), dtype=torch.float64), "mean_count": torch.tensor(int(m.mean_count))}
        return {k: v.detach().clone() for k, v in m.state_dict().items()}, losses, extra
    return run


@pytest.mark.parametrize("kind", ["network", "network_foc", "network_linear_bg", "network_cuda_ray"])
def test_whole_steps_repeat_bit_for_bit(kind, lib_option):
    lib_option(OPT, 1)
    run = _occupancy() if kind == "network_cuda_ray" else _fixed_step(kind)
    (p0, l0, e0), (p1, l1, e1) = run(), run()
    assert len(l0) == N_OPT_STEPS and all(bool(torch.isfinite(v)) for v in l0), [float(v) for v in l0]
    moved = [k for k in p0 if p0[k].is_floating_point() and k.split(".")[-1] in ("embeddings", "weight", "weights", "params")]
    assert moved, list(p0)
    for i, (a, b) in enumerate(zip(l0, l1)):
        assert _same(a, b), f"loss of step {i}: {float(a)!r} vs {float(b)!r}"
    for k in p0:
        assert torch.equal(p0[k], p1[k]) if not p0[k].is_floating_point() else _same(p0[k], p1[k]), k
    for k in e0:
        assert torch.equal(e0[k], e1[k]), f"{k}: {e0[k]} vs {e1[k]}"
    if kind == "network_cuda_ray":
        assert {"density_grid", "density_bitfield", "mean_density"} <= set(e0)
        assert 0 < int((e0["density_bitfield"] != 0).sum()), "the updated occupancy grid is empty"


def test_graph_replay_gives_the_eager_parameters(lib_option):
    """The headline step captured by GraphedStep under the option and replayed twice on one batch, against the same steps run eagerly
    from the same state (GraphedStep runs three eager warm-up steps before it captures: the eager run takes them too)."""
    import bench
    from focnerf_amd.graph import GraphedStep
    lib_option(OPT, 1)
    dev = torch.device("cuda", 0)
    batch = _batches(1, 9)[0]

    def make():
        torch.manual_seed(0)
        m = bench.build_model(2, dev, cuda_ray=False, seed=0).train()
        opt, scaler = _adam(m, capturable=True), torch.amp.GradScaler("cuda")
        torch.manual_seed(4321)
        return m, (lambda o, d, t: bench.train_step(m, opt, scaler, o, d, t, fused=True))

    def params(m):
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in m.state_dict().items()}

    m, step = make()
    eager = []
    for i in range(5):
        step(*batch)
        if i >= 3:
            eager.append(params(m))
    m, step = make()
    g = GraphedStep(step, batch)
    for want in eager:
        g(*batch)
        got = params(m)
        for k in want:
            assert torch.equal(want[k], got[k]) if not want[k].is_floating_point() else _same(want[k], got[k]), k


# ---------------------------------------------------------------- refusals and the other deterministic forms
def _small_grid(D, C, dtype, gridtype=0):
    L, H = 4, 8
    pls, S, off, table = tge._setup(D, C, L, H, 14, 64, 1, dtype, gridtype="hash")
    B = 3000
    x = tge._points(B, D, 2)
    grad = (np.random.default_rng(5).standard_normal((L, B, C)) * 0.1).astype(dtype)
    tdt = torch.float32 if dtype == np.float32 else torch.float16
    args = dict(xt=torch.from_numpy(x).cuda(), tt=torch.from_numpy(table).cuda(), ot=torch.from_numpy(off).cuda(), gt=torch.from_numpy(grad).cuda())

    def backward():
        ge = torch.zeros(int(off[-1]), C, dtype=tdt, device="cuda")
        tge._be().grid_encode_backward(args["gt"], args["xt"], args["tt"], args["ot"], ge, B, D, C, L, S, H, None, None, gridtype, False, 0)
        torch.cuda.synchronize()
        return ge

    def tv():
        gtv = torch.zeros(int(off[-1]), C, dtype=tdt, device="cuda")
        tge._be().grad_total_variation(args["xt"].to(tdt), args["tt"], gtv, args["ot"], 1e-2, B, D, C, L, S, H, gridtype, False)
        torch.cuda.synchronize()
        return gtv
    return backward, tv


@pytest.mark.parametrize("what", ["atomic_c4", "atomic_tiled", "atomic_d2", "atomic_nd4", "binned_fp32", "tv", "tv_nd5"])
def test_entry_points_without_a_deterministic_form_refuse(what, lib_option):
    D, C, dtype, gridtype = {"atomic_c4": (3, 4, np.float16, 0), "atomic_tiled": (3, 2, np.float16, 1), "atomic_d2": (2, 2, np.float32, 0),
                             "atomic_nd4": (4, 2, np.float16, 0), "binned_fp32": (3, 2, np.float32, 0), "tv": (3, 2, np.float16, 0),
                             "tv_nd5": (5, 2, np.float16, 0)}[what]
    backward, tv = _small_grid(D, C, dtype, gridtype)
    call = tv if what.startswith("tv") else backward
    lib_option(OPT, 0)
    before = call()
    assert float(before.float().abs().max()) > 0
    lib_option(OPT, 1)
    with pytest.raises(RuntimeError, match=OPT):
        call()
    lib_option(OPT, 0)
    after = call()                                         # as before (float atomics: to their spread, a few ulps of the sums)
    assert float((after.float() - before.float()).abs().max()) <= 2e-2 * float(before.float().abs().max()) + 1e-3


def test_background_backward_repeats_and_keeps_its_bounds(lib_option, monkeypatch):
    """foc_background_backward under the option: the table gradient repeats bit for bit, differs from the default mode's by no more than
    that test allows between two default runs, and holds the bounds of tests/test_gpu_network_linear.py::
    test_background_kernel_against_the_op_chain (16 fp16 eps relative to the op chain under autocast and to its fp32 restatement; the
    references are computed with the option off: their encoder_bg backward is the atomic kernel, which the option refuses)."""
    from focnerf_amd.background import background_rgb
    N = 4097
    m = tnl._net(cuda_ray=False)
    o, d = tnl._rays(N, N)
    g = (torch.rand(N, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) - 0.5).half()
    calls = tnl._count_calls(monkeypatch, ["foc_background_backward"])

    def fused():
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            rgb = background_rgb(m, d, rays_o=o, radius=m.bg_radius)
        rgb.backward(g)
        return rgb.detach(), tnl._bg_grads(m)

    lib_option(OPT, 0)
    rgb0, (e0, w0a, w1a) = fused()
    m.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        ref = tnl._op_chain(m, o, d)
    ref.backward(g)
    r_emb = tnl._bg_grads(m)[0]
    m.zero_grad(set_to_none=True)
    tnl._op_chain(m, o, d).backward(g.float())
    f_emb = m.encoder_bg.embeddings.grad.clone()
    lib_option(OPT, 1)
    rgb1, (e1, w0b, w1b) = fused()
    rgb2, (e2, w0c, w1c) = fused()
    assert calls["foc_background_backward"] == 3
    assert _same(rgb0, rgb1) and _same(w0a, w0b) and _same(w1a, w1b) and _same(w0b, w0c) and _same(w1b, w1c)
    assert float(e1.abs().max()) > 0 and _same(e1, e2)
    assert float((e1 - e0).abs().max()) <= 1e-4 * float(e0.abs().max())
    for name, want in (("op chain", r_emb), ("fp32 restatement", f_emb)):
        rel = float((e1 - want).norm() / want.norm().clamp_min(1e-30))
        assert rel <= 16 * tnl.FP16_EPS, f"table gradient: relative distance to the {name} {rel:.3g}"


def test_density_grid_mean_repeats(lib_option):
    """foc_grid_update_apply: per-workgroup partial sums added in workgroup order. Against the default mode the mean may differ in its last
    bit (another order of the same double additions, rounded to fp32 once): 2^-22 relative is two fp32 ulps."""
    from focnerf_amd import densitygrid
    C, H = 2, 128
    gen = torch.Generator(device="cuda").manual_seed(3)
    grid0 = torch.rand(C, H ** 3, device="cuda", generator=gen) * 2 - 0.5
    sig = torch.rand(C * H ** 3, device="cuda", generator=gen) * 3

    def apply():
        grid, bits, mean = grid0.clone(), torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device="cuda"), torch.empty(1, device="cuda")
        densitygrid.grid_update_apply(grid, C, H, sig, None, 1.0, 0.95, 0.01, bits, mean)
        torch.cuda.synchronize()
        return grid, bits, mean

    lib_option(OPT, 0)
    g0, b0, m0 = apply()
    lib_option(OPT, 1)
    (g1, b1, m1), (g2, b2, m2) = apply(), apply()
    assert _same(m1, m2) and torch.equal(b1, b2) and _same(g1, g2) and _same(g0, g1)
    assert float(m1) > 0 and abs(float(m1) - float(m0)) <= 2.0 ** -22 * float(m0)


def test_split_k_weight_gradient_repeats(lib_option):
    """k_mlp_dw (hidden 128: the two-kernel backward) with one blob image per split-K workgroup, summed in workgroup order. Both modes round
    one fp32 sum per weight to half; the sums differ by the order of fp32 additions, so the results differ by at most one half ulp on a
    few weights: 2^-10 relative in the L2 norm is two half ulps on EVERY weight."""
    from focnerf_amd.ffmlp import FFMLP
    torch.manual_seed(0)
    mlp = FFMLP(32, 16, 128, 2).cuda()
    B = 1 << 16
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, 32, device="cuda", generator=gen).half()
    g = (torch.randn(B, 16, device="cuda", generator=gen) * 0.01).half()

    def grad():
        mlp.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            y = mlp(x)
        y.backward(g.to(y.dtype))
        torch.cuda.synchronize()
        return next(p.grad for p in mlp.parameters() if p.grad is not None).detach().clone()

    lib_option(OPT, 0)
    a = grad()
    lib_option(OPT, 1)
    b, c = grad(), grad()
    assert float(b.float().abs().max()) > 0 and _same(b, c)
    rel = float((a.float() - b.float()).norm() / a.float().norm())
    assert rel <= 2.0 ** -10, rel
