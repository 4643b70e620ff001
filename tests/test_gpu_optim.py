"""GPU: focnerf_amd.optim (csrc/optim.hip) against the float64 statement of the step in tests/adam_ref.py, with the fp32 bounds derived
there from the kernel's operations (adam_ref.fp32_bounds), against torch's own fused Adam, and on the library's real training path.

Inputs: params in +-1; grad magnitudes log-uniform in [1e-6, 1e2] times the loss scale, random signs, one element in eight exactly 0 —
g^2 stays out of fp32 underflow, where a float64 reference and ANY fp32 Adam part ways at eps = 1e-15. Every scale is a power of two."""
import numpy as np
import pytest
import torch

import adam_ref

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.99), 1e-15


def _grad(n, scale, gen):
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    keep = (torch.rand(n, generator=gen) >= 0.125).double()
    return (mag * sign * keep).float().mul(float(scale)).cuda()


def _param(n, gen, offset=0):
    """A parameter of n elements in +-1; offset = 1: a view one element into its storage (4-byte aligned only)."""
    buf = (torch.rand(n + offset, generator=gen) * 2 - 1).cuda()
    p = torch.nn.Parameter(buf[offset:])
    assert p.data_ptr() % 16 == 4 * offset or offset == 0
    return p


def _snapshot(opt, params):
    """(p, exp_avg, exp_avg_sq, step) of every param as float64 / float numpy, zeros where the state does not exist yet."""
    out = []
    for p in params:
        st = opt.state.get(p, {})
        m = st["exp_avg"].detach().cpu().numpy().copy() if "exp_avg" in st else np.zeros(p.shape, np.float32)
        v = st["exp_avg_sq"].detach().cpu().numpy().copy() if "exp_avg_sq" in st else np.zeros(p.shape, np.float32)
        out.append((p.detach().cpu().numpy().copy(), m, v, float(st["step"]) if "step" in st else 0.0))
    return out


def _hyper(opt, p):
    for g in opt.param_groups:
        if any(q is p for q in g["params"]):
            return float(g["lr"]), float(g["weight_decay"])
    raise KeyError


def _assert_step_within_bounds(opt, params, before, grads_scaled, scale, what=""):
    """Every tensor after the step against adam_ref evaluated in float64 on what the kernel read (`before`, the scaled grads)."""
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for p, (p0, m0, v0, t0), g in zip(params, before, grads_scaled):
        if g is None:
            continue
        lr, wd = _hyper(opt, p)
        ref = adam_ref.adam_step(p0, g.cpu().numpy(), m0, v0, t0, scale=scale, lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
        assert not ref["skipped"]
        bound = adam_ref.fp32_bounds(ref, p0, m0, scale=scale, betas=BETAS, weight_decay=wd)
        st = opt.state[p]
        got = {"p": p.detach().cpu().numpy().astype(np.float64), "m": st["exp_avg"].cpu().numpy().astype(np.float64),
               "v": st["exp_avg_sq"].cpu().numpy().astype(np.float64)}
        for k in ("v", "m", "p"):
            err = np.abs(got[k] - ref[k])
            ratio = float(np.max(err / np.maximum(bound[k], 1e-300)))
            worst[k] = max(worst[k], ratio)
            assert (err <= bound[k]).all(), f"{what} {k}: n={p.numel()} worst error / bound = {ratio:.3f} at {int(np.argmax(err / np.maximum(bound[k], 1e-300)))}"
        assert float(st["step"]) == ref["step"]
    print(f"{what} worst error / bound: v {worst['v']:.3f} m {worst['m']:.3f} p {worst['p']:.3f}")
    return worst


def _mixed_setup(gen):
    """The sizes around the kernel's chunk in two groups (different lr, one with weight decay), a param and a grad one element into their
    storage, one param without a grad."""
    from focnerf_amd import FusedAdam, optim
    C = optim.CHUNK
    sizes = [1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 7]
    params = [_param(n, gen, offset=1 if n == C + 1 else 0) for n in sizes]
    gradless = _param(9, gen)
    opt = FusedAdam([{"params": params[0::2] + [gradless], "lr": 1e-2}, {"params": params[1::2], "lr": 3e-3, "weight_decay": 0.1}],
                    betas=BETAS, eps=EPS)
    return opt, params, gradless


def _set_grads(params, scale, gen):
    grads = []
    for p in params:
        g = _grad(p.numel(), scale, gen)
        if p.numel() == 5:                                           # this grad sits one element into its storage
            buf = torch.zeros(6, device="cuda")
            buf[1:] = g
            g = buf[1:]
        p.grad = g
        grads.append(g.clone())
    return grads


def test_one_step_against_float64():
    """1. Eight sizes around the chunk in one call: within 4 ulp (exp_avg_sq), 4 * 2^-24 max(|m_old|, |g|) (exp_avg) and
    ulp(p)/2 + 8 * 2^-23 step_size max(|m_old|, |g|) / denom (param) of float64; the weight-decay group with the terms adam_ref.fp32_bounds
    derives for the fma that adds wd * p. A second step runs on non-zero moments."""
    from focnerf_amd import LossScaler
    gen = torch.Generator().manual_seed(11)
    opt, params, gradless = _mixed_setup(gen)
    scaler = LossScaler(init_scale=1024.0)
    for it in (1, 2):
        grads = _set_grads(params, 1024.0, gen)
        before = _snapshot(opt, params)
        opt.step(scaler=scaler)
        _assert_step_within_bounds(opt, params, before, grads, 1024.0, what=f"one step ({it})")
        for p, g in zip(params, grads):
            assert float(opt.state[p]["step"]) == it and torch.equal(p.grad, g), "grads are left alone without zero_grads"
        assert float(opt.state.get(gradless, {}).get("step", 0.0)) == 0.0 and len(opt.state.get(gradless, {})) == 0
    assert scaler.get_scale() == 1024.0 and scaler._get_growth_tracker() == 2


@pytest.mark.parametrize("zero_grads", [False, True])
@pytest.mark.parametrize("where", ["inf_last", "nan_first"])
def test_overflow_skips_the_whole_step(where, zero_grads):
    """2. One inf in the last element of the last tensor / one nan in the first of the first: params, moments and counters bit-identical,
    scale halved, tracker 0. zero_grads=True zeroes the grads of a skipped step too (documented in FusedAdam.step; torch leaves them)."""
    from focnerf_amd import LossScaler
    gen = torch.Generator().manual_seed(12)
    opt, params, gradless = _mixed_setup(gen)
    scaler = LossScaler(init_scale=1024.0)
    _set_grads(params, 1024.0, gen)
    opt.step(scaler=scaler)                                          # a clean step first: the moments exist and are not zero
    grads = _set_grads(params, 1024.0, gen)
    if where == "inf_last":
        params[-1].grad[-1] = float("inf")
    else:
        params[0].grad[0] = float("nan")
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), opt.state[p]["step"].clone()) for p in params]
    gl = gradless.detach().clone()
    opt.step(scaler=scaler, zero_grads=zero_grads)
    for p, (p0, m0, v0, t0) in zip(params, before):
        st = opt.state[p]
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32)) and torch.equal(st["exp_avg"].view(torch.int32), m0.view(torch.int32))
        assert torch.equal(st["exp_avg_sq"].view(torch.int32), v0.view(torch.int32)) and float(st["step"]) == float(t0) == 1.0
        if zero_grads:
            assert not p.grad.any()
    if not zero_grads:
        bad = params[-1] if where == "inf_last" else params[0]
        assert not torch.isfinite(bad.grad).all() and torch.equal(params[3].grad, grads[3])
    assert torch.equal(gradless.detach(), gl)
    assert scaler.get_scale() == 512.0 and scaler._get_growth_tracker() == 0
    # and the step after it is a step again, at the new scale
    grads = _set_grads(params, 512.0, gen)
    snap = _snapshot(opt, params)
    opt.step(scaler=scaler, zero_grads=zero_grads)
    _assert_step_within_bounds(opt, params, snap, grads, 512.0, what="after the skipped step")
    assert scaler._get_growth_tracker() == 1 and (not zero_grads or not any(p.grad.any() for p in params))


def test_scale_doubling_every_step_never_tears():
    """3. growth_interval = 1: the first launch doubles the scale in every step. 2^20 elements, 4 steps: every element of every step is
    the reference at that step's ONE scale (a workgroup that read a half-updated scale or counter would be off by a factor of two)."""
    from focnerf_amd import FusedAdam, LossScaler
    gen = torch.Generator().manual_seed(13)
    p = _param(1 << 20, gen)
    opt = FusedAdam([p], lr=1e-2, betas=BETAS, eps=EPS)
    scaler = LossScaler(init_scale=1024.0, growth_interval=1)
    scale = 1024.0
    for it in range(4):
        grads = _set_grads([p], scale, gen)
        before = _snapshot(opt, [p])
        opt.step(scaler=scaler)
        _assert_step_within_bounds(opt, [p], before, grads, scale, what=f"scale race step {it}")
        scale *= 2.0
    assert scaler.get_scale() == 1024.0 * 16 and float(opt.state[p]["step"]) == 4.0


def test_eight_step_trajectory_against_torch():
    """4. The same grads (independent of the params) to FusedAdam and to torch.optim.Adam(fused=True, capturable=True). The yardstick is
    measured here: the largest distance between torch's foreach and fused Adam on these inputs, relative to max(|p|, lr); FusedAdam lies
    within twice that of torch's fused result, and within the per-step bounds against float64."""
    from focnerf_amd import FusedAdam, LossScaler, optim
    gen = torch.Generator().manual_seed(14)
    sizes = [5, optim.CHUNK + 1, 3 * optim.CHUNK]
    lr = 1e-2
    init = [_param(n, gen) for n in sizes]

    def copies():
        return [torch.nn.Parameter(p.detach().clone()) for p in init]
    p_ours, p_fused, p_foreach = copies(), copies(), copies()
    ours = FusedAdam(p_ours, lr=lr, betas=BETAS, eps=EPS)
    fused = torch.optim.Adam(p_fused, lr=lr, betas=BETAS, eps=EPS, fused=True, capturable=True)
    foreach = torch.optim.Adam(p_foreach, lr=lr, betas=BETAS, eps=EPS, foreach=True, capturable=True)
    scaler = LossScaler(init_scale=1024.0)

    def rel(a, b):
        return max(float(((x.detach().double() - y.detach().double()).abs() / torch.clamp(y.detach().double().abs(), min=lr)).max()) for x, y in zip(a, b))
    yardstick, ours_dist = 0.0, 0.0
    for it in range(8):
        unscaled = [_grad(n, 1.0, gen) for n in sizes]
        for group, k in ((p_fused, 1.0), (p_foreach, 1.0), (p_ours, 1024.0)):
            for p, g in zip(group, unscaled):
                p.grad = g * k                                       # a power of two: the same grad after the kernel's unscale
        before = _snapshot(ours, p_ours)
        ours.step(scaler=scaler)
        fused.step()
        foreach.step()
        _assert_step_within_bounds(ours, p_ours, before, [p.grad for p in p_ours], 1024.0, what=f"trajectory step {it}")
        yardstick = max(yardstick, rel(p_foreach, p_fused))
        ours_dist = max(ours_dist, rel(p_ours, p_fused))
    print(f"trajectory: torch foreach vs torch fused {yardstick:.3e}, FusedAdam vs torch fused {ours_dist:.3e} (relative to max(|p|, lr))")
    assert ours_dist <= 2.0 * yardstick, (ours_dist, yardstick)
    assert all(float(ours.state[p]["step"]) == 8.0 for p in p_ours)


def test_more_than_sixteen_tensors_share_one_decision():
    """5. 17 tensors in one optimizer = the same tensors in two optimizers of 8 and 9, bit for bit; one inf in tensor 17 skips all 17."""
    from focnerf_amd import FusedAdam, LossScaler
    gen = torch.Generator().manual_seed(15)
    sizes = [3 + 37 * k for k in range(17)]
    init = [_param(n, gen) for n in sizes]
    a = [torch.nn.Parameter(p.detach().clone()) for p in init]
    b = [torch.nn.Parameter(p.detach().clone()) for p in init]
    one = FusedAdam(a, lr=1e-2, betas=BETAS, eps=EPS)
    two = [FusedAdam(b[:8], lr=1e-2, betas=BETAS, eps=EPS), FusedAdam(b[8:], lr=1e-2, betas=BETAS, eps=EPS)]
    s_one, s_two = LossScaler(init_scale=1024.0, growth_interval=2), [LossScaler(init_scale=1024.0, growth_interval=2) for _ in two]
    for it in range(3):                                              # the scale grows after the second step: the third runs at 2048
        scale = 1024.0 if it < 2 else 2048.0
        grads = [_grad(n, scale, gen) for n in sizes]
        for p, q, g in zip(a, b, grads):
            p.grad, q.grad = g.clone(), g.clone()
        one.step(scaler=s_one)
        for o, s in zip(two, s_two):
            o.step(scaler=s)
        for p, q in zip(a, b):
            so, st = one.state[p], (two[0].state[q] if q in two[0].state else two[1].state[q])
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
            assert torch.equal(so["exp_avg"].view(torch.int32), st["exp_avg"].view(torch.int32))
            assert torch.equal(so["exp_avg_sq"].view(torch.int32), st["exp_avg_sq"].view(torch.int32)) and float(so["step"]) == float(st["step"]) == it + 1
    assert s_one.get_scale() == 2048.0 == s_two[0].get_scale() and s_one._get_growth_tracker() == 1
    before = [(p.detach().clone(), one.state[p]["exp_avg"].clone(), one.state[p]["exp_avg_sq"].clone()) for p in a]
    for p, n in zip(a, sizes):
        p.grad = _grad(n, 2048.0, gen)
    a[16].grad[5] = float("inf")
    one.step(scaler=s_one)
    for p, (p0, m0, v0) in zip(a, before):
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32)) and torch.equal(one.state[p]["exp_avg"].view(torch.int32), m0.view(torch.int32))
        assert torch.equal(one.state[p]["exp_avg_sq"].view(torch.int32), v0.view(torch.int32)) and float(one.state[p]["step"]) == 3.0
    assert s_one.get_scale() == 1024.0 and s_one._get_growth_tracker() == 0


@pytest.mark.parametrize("overflow", [False, True])
def test_torch_grad_scaler_route_is_the_loss_scaler_route(overflow):
    """6. The unedited trainer lines — scaler.step(optimizer); scaler.update() with torch's GradScaler — give the bits of
    step(scaler=LossScaler) on the same inputs, for a clean step and for an overflow step (after one clean step each)."""
    from focnerf_amd import FusedAdam, LossScaler
    gen = torch.Generator().manual_seed(16)
    opt_c, params_c, _ = _mixed_setup(gen)
    gen = torch.Generator().manual_seed(16)
    opt_b, params_b, _ = _mixed_setup(gen)
    ls = LossScaler(init_scale=1024.0, growth_interval=2)
    gs = torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    for it in range(3):
        scale = 1024.0
        grads = _set_grads(params_c, scale, gen)
        if overflow and it == 1:
            grads[2][1] = float("-inf")
        for p, q, g in zip(params_c, params_b, grads):
            p.grad, q.grad = g.clone(), g.clone()
        opt_c.step(scaler=ls)
        gs.scale(torch.zeros((), device="cuda"))                     # (creates torch's scale tensor, as scaler.scale(loss) does in a trainer)
        gs.step(opt_b)
        gs.update()
        for p, q in zip(params_c, params_b):
            sc, sb = opt_c.state[p], opt_b.state[q]
            assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)), f"step {it}"
            assert torch.equal(sc["exp_avg"].view(torch.int32), sb["exp_avg"].view(torch.int32))
            assert torch.equal(sc["exp_avg_sq"].view(torch.int32), sb["exp_avg_sq"].view(torch.int32)) and float(sc["step"]) == float(sb["step"])
        assert ls.get_scale() == gs.get_scale() and ls._get_growth_tracker() == gs._get_growth_tracker()
        if not (overflow and it >= 1):
            assert float(opt_c.state[params_c[0]]["step"]) == it + 1
    assert ls.get_scale() == (512.0 if overflow else 2048.0)
    assert not hasattr(opt_b, "grad_scale") and not hasattr(opt_b, "found_inf")


def test_no_host_sync_and_graph_capture():
    """7. step(scaler=...) under torch's sync debug mode "error"; then the step captured in a graph and replayed 3 times with fresh grads
    copied into the captured buffers and a device lr that changes between replays = 3 eager steps, bit for bit."""
    from focnerf_amd import FusedAdam, LossScaler, optim
    gen = torch.Generator().manual_seed(17)
    sizes = [5, optim.CHUNK + 1, 2 * optim.CHUNK + 7]
    init = [_param(n, gen) for n in sizes]
    lrs = [1e-2, 5e-3, 2.5e-3]
    grads = [[_grad(n, 1024.0 * 2.0 ** it, gen) for n in sizes] for it in range(3)]

    def make():
        params = [torch.nn.Parameter(p.detach().clone()) for p in init]
        lr = torch.tensor(lrs[0], dtype=torch.float32, device="cuda")
        opt = FusedAdam(params, lr=lr, betas=BETAS, eps=EPS)
        return params, lr, opt, LossScaler(init_scale=1024.0, growth_interval=1)

    pe, lr_e, opt_e, sc_e = make()
    opt_e.init_state(sc_e)
    has_debug = hasattr(torch.cuda, "set_sync_debug_mode")
    for it in range(3):
        lr_e.fill_(lrs[it])
        for p, g in zip(pe, grads[it]):
            p.grad = g.clone()
        if has_debug:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt_e.step(scaler=sc_e, zero_grads=True)
        finally:
            if has_debug:
                torch.cuda.set_sync_debug_mode("default")
    assert sc_e.get_scale() == 8192.0

    pg, lr_g, opt_g, sc_g = make()
    opt_g.init_state(sc_g)
    for p in pg:
        p.grad = torch.zeros_like(p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step(scaler=sc_g, zero_grads=True)
    assert all(float(opt_g.state[p]["step"]) == 0.0 for p in pg), "a capture executes nothing"
    for it in range(3):
        lr_g.fill_(lrs[it])
        for p, g in zip(pg, grads[it]):
            p.grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(pe, pg):
        se, sg = opt_e.state[p], opt_g.state[q]
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        assert torch.equal(se["exp_avg"].view(torch.int32), sg["exp_avg"].view(torch.int32)) and torch.equal(se["exp_avg_sq"].view(torch.int32), sg["exp_avg_sq"].view(torch.int32))
        assert float(se["step"]) == float(sg["step"]) == 3.0 and not q.grad.any() and not p.grad.any()
    assert sc_g.get_scale() == 8192.0
    # a grad that has moved since the capture: the next eager step simply reads the new tensor
    for p, q, g in zip(pe, pg, grads[0]):
        p.grad, q.grad = g.clone() * 8.0, g.clone() * 8.0
    opt_e.step(scaler=sc_e)
    opt_g.step(scaler=sc_g)
    assert all(torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32)) for p, q in zip(pe, pg))


def test_on_the_real_training_path():
    """8. NeRFNetwork(bound=1).run(fused=True), 64 rays x 64 steps, fp16 autocast, deterministic mode: LossScaler.scale(loss).backward(), then
    FusedAdam(model.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15).step(scaler=...). Every parameter tensor within the bounds of 1. against
    adam_ref on the cloned scaled grads; a second run from the same seed gives the same bits."""
    import focnerf_amd
    from focnerf_amd import FusedAdam, LossScaler, synthetic
    from focnerf_amd.network import NeRFNetwork

    def run():
        torch.manual_seed(5)
        gen = torch.Generator().manual_seed(5)
        m = NeRFNetwork(bound=1).cuda().train()
        poses = synthetic.rand_poses(1, "cuda", radius=2.0, generator=gen)
        ro, rd = synthetic.get_rays(poses, synthetic.intrinsics(8, 8), 8, 8)
        target = torch.rand(1, ro.shape[1], 3, generator=gen).cuda()
        opt = FusedAdam(m.get_params(1e-2), betas=BETAS, eps=EPS)
        scaler = LossScaler(init_scale=1024.0)
        with focnerf_amd.deterministic():
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.run(ro, rd, None, fused=True, num_steps=64, upsample_steps=0, bg_color=1.0, perturb=False)
                loss = torch.nn.functional.mse_loss(out["image"], target)
            scaler.scale(loss).backward()
            params = [p for g in opt.param_groups for p in g["params"] if p.grad is not None]
            grads = [p.grad.clone() for p in params]
            before = _snapshot(opt, params)
            opt.step(scaler=scaler)
        return opt, params, grads, before

    opt, params, grads, before = run()
    assert len(params) >= 3 and all(torch.isfinite(g).all() for g in grads) and any(g.abs().sum() > 0 for g in grads)
    _assert_step_within_bounds(opt, params, before, grads, 1024.0, what="real path")
    opt2, params2, _, _ = run()
    for p, q in zip(params, params2):
        assert torch.equal(p.detach().view(torch.int32), q.detach().view(torch.int32))
        assert torch.equal(opt.state[p]["exp_avg_sq"].view(torch.int32), opt2.state[q]["exp_avg_sq"].view(torch.int32))
