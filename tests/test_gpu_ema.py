"""GPU: focnerf_amd.ParameterEMA (csrc/optim.hip k_ema_update, k_opt_adam_ema) against torch_ema's three torch ops run on the device with
the same 1 - decay_t, bit for bit: the bare update, the EMA inside FusedAdam.step on its three routes, a skipped step, graph replay, the
launch counts, the schedule across n = 170 computed on the device, and the real fused training and render path.

Tensor sizes sit around the kernels' chunk of 4096 elements (0, 1, 3, 4095, 4096, 4097, 2 x 4096 + 5); one parameter is a view one element
into its storage and one aligned parameter has such a shadow (the 4-byte path from either side); 19 tensors take a step (two groups of
the kernels' 16); one parameter has no grad, one is tracked by the EMA and unknown to the optimizer, one is empty."""
import ctypes

import pytest
import torch

import ema_ref

pytestmark = pytest.mark.gpu

BETAS, EPS, DECAY = (0.9, 0.99), 1e-15, 0.95
C = 4096
SIZES = [1, 3, C - 1, C, C + 1, 2 * C + 5]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _grad(n, scale, gen):
    mag = 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 8.0 - 6.0)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    keep = (torch.rand(n, generator=gen) >= 0.125).double()
    return (mag * sign * keep).float().mul(float(scale)).cuda()


def _param(n, gen, offset=0):
    buf = (torch.rand(n + offset, generator=gen) * 2 - 1).cuda()
    p = torch.nn.Parameter(buf[offset:])
    assert p.data_ptr() % 16 == 4 * offset or offset == 0 or n == 0
    return p


def _offset_copy(t):
    """The same values one element into a fresh storage: 4-byte aligned only."""
    buf = torch.zeros(t.numel() + 1, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


class _Setup:
    """19 stepping tensors in two param groups (different lr, one with weight decay), a param without a grad, a param outside the
    optimizer, an empty param; `ema=True`: a ParameterEMA over all of them, one shadow moved one element into its storage."""

    def __init__(self, seed, ema=True, lr=None):
        from focnerf_amd import FusedAdam, ParameterEMA
        gen = torch.Generator().manual_seed(seed)
        sizes = SIZES + [C + 1, C + 3] + [5 + 13 * k for k in range(11)]
        self.stepping = [_param(n, gen, offset=1 if i == len(SIZES) else 0) for i, n in enumerate(sizes)]
        assert len(self.stepping) == 19
        self.gradless, self.outsider, self.empty = _param(37, gen), _param(C + 50, gen), _param(0, gen)
        self.tracked = self.stepping + [self.gradless, self.outsider, self.empty]
        groups = [{"params": self.stepping[0::2] + [self.gradless], "lr": 1e-2 if lr is None else lr},
                  {"params": self.stepping[1::2], "lr": 3e-3 if lr is None else lr, "weight_decay": 0.1}]
        self.opt = FusedAdam(groups, betas=BETAS, eps=EPS)
        self.order = [p for g in self.opt.param_groups for p in g["params"] if p is not self.gradless]       # the order the step takes them in
        self.ema = None
        self.shadows = [p.detach().clone() for p in self.tracked]
        if ema:
            self.ema = ParameterEMA(self.tracked, DECAY)
            k = len(SIZES) + 1                                                       # the aligned C + 3 parameter gets a misaligned shadow
            self.ema.shadow_params[k] = _offset_copy(self.ema.shadow_params[k])
            self.shadows = self.ema.shadow_params
        for s in self.shadows:
            s.mul_(0.75)                                                             # (a shadow equal to a parameter that never moves would stay put)

    def set_grads(self, scale, gen):
        for p in self.stepping:
            p.grad = _grad(p.numel(), scale, gen)

    def torch_rule(self, n):
        """torch_ema's update on the device with the omd of count n (Python double arithmetic, rounded to fp32 by mul_)"""
        one_minus_decay = 1.0 - ema_ref.decay_at(DECAY, n)
        with torch.no_grad():
            for p, s in zip(self.tracked, self.shadows):
                tmp = s - p
                tmp.mul_(one_minus_decay)
                s.sub_(tmp)

    def moved(self, gen):
        with torch.no_grad():
            for p in self.tracked:
                p.add_(((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1).cuda())


def _assert_same_state(a, b, what=""):
    for i, (p, q) in enumerate(zip(a.tracked, b.tracked)):
        assert _same(p, q), f"{what} param {i} (n={p.numel()})"
        sa, sb = a.opt.state.get(p, {}), b.opt.state.get(q, {})
        assert sa.keys() == sb.keys()
        for k in sa:
            assert _same(sa[k], sb[k]), f"{what} {k} of param {i} (n={p.numel()})"
    for i, (s, r) in enumerate(zip(a.shadows, b.shadows)):
        assert _same(s, r), f"{what} shadow {i} (n={s.numel()})"


# ---------------------------------------------------------------- the bare update
def test_bare_update_is_the_three_torch_ops():
    gen = torch.Generator().manual_seed(21)
    a, b = _Setup(1), _Setup(1, ema=False)
    assert a.ema.shadow_params[len(SIZES) + 1].data_ptr() % 16 == 4 and a.tracked[len(SIZES)].data_ptr() % 16 == 4
    for it in range(5):
        g1, g2 = torch.Generator().manual_seed(100 + it), torch.Generator().manual_seed(100 + it)
        a.moved(g1)
        b.moved(g2)
        a.ema.update()
        b.torch_rule(it + 1)
        for i, (s, r) in enumerate(zip(a.shadows, b.shadows)):
            assert _same(s, r), f"update {it} shadow {i} (n={s.numel()})"
    assert a.ema.num_updates == 5 and a.ema._count.dtype == torch.int64 and a.ema._count.is_cuda and a.ema._count.dim() == 0
    assert not any(_same(s, p) for s, p in zip(a.shadows, a.tracked) if p.numel() > 1), "the shadows lag the parameters"
    assert a.ema.state_dict()["num_updates"] == 5
    del gen


def test_constant_decay_and_explicit_parameters_on_the_device():
    from focnerf_amd import ParameterEMA
    gen = torch.Generator().manual_seed(22)
    params = [_param(n, gen) for n in (3, C + 1)]
    ema = ParameterEMA(params, 0.9, use_num_updates=False)
    ref = [p.detach().clone() for p in params]
    for it in range(2):
        with torch.no_grad():
            for p in params:
                p.mul_(1.5)
        ema.update(params)
        for p, s in zip(params, ref):
            tmp = s - p.detach()
            tmp.mul_(1.0 - 0.9)
            s.sub_(tmp)
    assert ema.num_updates is None and ema._count is None and all(_same(s, r) for s, r in zip(ema.shadow_params, ref))


# ---------------------------------------------------------------- the EMA inside the step
def _take_step(setup, route, scaler, zero_grads, with_ema):
    kw = dict(ema=setup.ema) if with_ema else {}
    if route == "loss":
        setup.opt.step(scaler=scaler, zero_grads=zero_grads, **kw)
    elif route == "grad":
        scaler.scale(torch.zeros((), device="cuda"))
        scaler.step(setup.opt, zero_grads=zero_grads, **kw)
        scaler.update()
    else:
        setup.opt.step(zero_grads=zero_grads, **kw)


def _scaler(route):
    from focnerf_amd import LossScaler
    if route == "loss":
        return LossScaler(init_scale=1024.0, growth_interval=2)
    if route == "grad":
        return torch.amp.GradScaler("cuda", init_scale=1024.0, growth_interval=2)
    return None


def _scale_state(route, scaler):
    if route == "loss":
        return scaler.get_scale(), scaler._get_growth_tracker()
    if route == "grad":
        return scaler.get_scale(), scaler._get_growth_tracker()
    return None


@pytest.mark.parametrize("zero_grads", [False, True])
@pytest.mark.parametrize("route", ["loss", "grad", "none"])
def test_step_with_ema_is_step_then_the_torch_rule(route, zero_grads):
    """19 stepping tensors (two groups of 16), a gradless, an outside and an empty tracked tensor: step(ema=) against a twin that takes
    step() and then torch_ema's three ops — params, moments, step counters, scale, tracker and shadows bit for bit, over three steps (the
    scale grows after the second)."""
    a, b = _Setup(2), _Setup(2, ema=False)
    sa, sb = _scaler(route), _scaler(route)
    for it in range(3):
        scale = 1.0 if route == "none" else (1024.0 if it < 2 else 2048.0)
        g1, g2 = torch.Generator().manual_seed(200 + it), torch.Generator().manual_seed(200 + it)
        a.set_grads(scale, g1)
        b.set_grads(scale, g2)
        _take_step(a, route, sa, zero_grads, True)
        _take_step(b, route, sb, zero_grads, False)
        b.torch_rule(it + 1)
        _assert_same_state(a, b, f"{route} step {it}")
        assert _scale_state(route, sa) == _scale_state(route, sb)
        for p, q in zip(a.stepping, b.stepping):
            assert _same(p.grad, q.grad) and (not zero_grads or not p.grad.any())
        assert all(float(a.opt.state[p]["step"]) == it + 1 for p in a.stepping) and len(a.opt.state.get(a.gradless, {})) == 0
    assert a.ema.num_updates == 3
    if route != "none":
        assert _scale_state(route, sa) == (2048.0, 1)


@pytest.mark.parametrize("route", ["loss", "grad"])
def test_overflow_skips_the_step_and_the_ema_still_moves(route):
    """One inf in a grad of the SECOND group, after one clean step: params, moments and step counters untouched, the scale backed off, and
    every shadow moved by the rule toward the unchanged parameter; the counter reads 2."""
    a = _Setup(3)
    scaler = _scaler(route)
    a.set_grads(1024.0, torch.Generator().manual_seed(300))
    _take_step(a, route, scaler, False, True)
    a.set_grads(1024.0, torch.Generator().manual_seed(301))
    victim = a.order[17]
    victim.grad[victim.numel() // 2] = float("inf")
    before = [(p.detach().clone(), {k: v.clone() for k, v in a.opt.state.get(p, {}).items()}) for p in a.tracked]
    want = [s.clone() for s in a.shadows]
    one_minus_decay = 1.0 - ema_ref.decay_at(DECAY, 2)
    for p, s in zip(a.tracked, want):
        tmp = s - p.detach()
        tmp.mul_(one_minus_decay)
        s.sub_(tmp)
    _take_step(a, route, scaler, False, True)
    for p, (p0, st0) in zip(a.tracked, before):
        assert _same(p, p0) and all(_same(a.opt.state[p][k], v) for k, v in st0.items())
    assert all(float(a.opt.state[p]["step"]) == 1.0 for p in a.stepping)
    assert _scale_state(route, scaler) == (512.0, 0)
    for i, (s, w) in enumerate(zip(a.shadows, want)):
        assert _same(s, w), f"shadow {i} (n={s.numel()})"
    assert a.ema.num_updates == 2


def test_no_grads_at_all_is_a_bare_update():
    a, b = _Setup(4), _Setup(4, ema=False)
    a.opt.step(ema=a.ema)
    b.torch_rule(1)
    _assert_same_state(a, b, "no grads")
    assert a.ema.num_updates == 1
    with pytest.raises(TypeError, match="ParameterEMA"):
        a.opt.step(ema=object())


# ---------------------------------------------------------------- no host synchronisation, graph replay, launch counts
def _small(seed, n_stepping=3):
    """(params, gradless-free optimizer, LossScaler, ParameterEMA over the stepping params [+ one outsider])"""
    from focnerf_amd import FusedAdam, LossScaler, ParameterEMA
    gen = torch.Generator().manual_seed(seed)
    sizes = ([5, C + 1, 2 * C + 7] + [9 + 7 * k for k in range(16)])[:n_stepping]
    params = [_param(n, gen) for n in sizes]
    outsider = _param(C + 9, gen)
    lr = torch.tensor(1e-2, dtype=torch.float32, device="cuda")
    opt = FusedAdam(params, lr=lr, betas=BETAS, eps=EPS)
    return params, outsider, lr, opt, LossScaler(init_scale=1024.0, growth_interval=1), ParameterEMA


def test_no_host_sync_and_graph_capture_with_the_ema():
    """step(scaler=, ema=) under torch's sync debug mode "error" (three eager steps, with a tracked tensor outside the optimizer); then the
    same step captured in a graph and replayed three times with fresh grads and a device lr that changes = the three eager steps, bit for
    bit, the shadows and the counter included."""
    sizes = [5, C + 1, 2 * C + 7]
    lrs = [1e-2, 5e-3, 2.5e-3]
    ggen = torch.Generator().manual_seed(41)
    grads = [[_grad(n, 1024.0 * 2.0 ** it, ggen) for n in sizes] for it in range(3)]

    def make():
        params, outsider, lr, opt, scaler, EMA = _small(40)
        ema = EMA(params + [outsider], DECAY)
        ema.shadow_params[-1].mul_(0.75)                             # (a shadow equal to a parameter that never moves would stay put)
        opt.init_state(scaler, ema=ema)
        assert ema._count is not None and ema._count.is_cuda and int(ema._count) == 0
        return params, outsider, lr, opt, scaler, ema

    pe, oe, lr_e, opt_e, sc_e, ema_e = make()
    has_debug = hasattr(torch.cuda, "set_sync_debug_mode")
    for it in range(3):
        lr_e.fill_(lrs[it])
        for p, g in zip(pe, grads[it]):
            p.grad = g.clone()
        if has_debug:
            torch.cuda.set_sync_debug_mode("error")
        try:
            opt_e.step(scaler=sc_e, zero_grads=True, ema=ema_e)
        finally:
            if has_debug:
                torch.cuda.set_sync_debug_mode("default")
    assert sc_e.get_scale() == 8192.0 and ema_e.num_updates == 3

    pg, og, lr_g, opt_g, sc_g, ema_g = make()
    for p in pg:
        p.grad = torch.zeros_like(p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt_g.step(scaler=sc_g, zero_grads=True, ema=ema_g)
    assert int(ema_g._count) == 0 and all(_same(s, p) for s, p in zip(ema_g.shadow_params[:-1], pg)), "a capture executes nothing"
    for it in range(3):
        lr_g.fill_(lrs[it])
        for p, g in zip(pg, grads[it]):
            p.grad.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    for p, q in zip(pe, pg):
        se, sg = opt_e.state[p], opt_g.state[q]
        assert _same(p, q) and _same(se["exp_avg"], sg["exp_avg"]) and _same(se["exp_avg_sq"], sg["exp_avg_sq"])
        assert float(se["step"]) == float(sg["step"]) == 3.0 and not q.grad.any()
    for s, r in zip(ema_e.shadow_params, ema_g.shadow_params):
        assert _same(s, r)
    assert not _same(ema_g.shadow_params[1], pg[1]) and not _same(ema_g.shadow_params[-1], og)
    assert ema_g.num_updates == 3 and sc_g.get_scale() == 8192.0


def test_counter_and_workspace_must_exist_before_a_capture(monkeypatch):
    from focnerf_amd import ParameterEMA
    p = _param(8, torch.Generator().manual_seed(42))
    ema = ParameterEMA([p], DECAY)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before a graph capture"):
        ema._on(p.device)
    with pytest.raises(RuntimeError, match="before a graph capture"):
        ema._workspace(p.device)


def _hip_runtime():
    """The HIP runtime this process has loaded (torch's), for hipGraphGetNodes."""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    return ctypes.CDLL(paths[0])


def _captured_kernels(fn):
    """Nodes of the graph that one call of `fn` captures: every launch is one kernel node (the step enqueues nothing else)."""
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        fn()
    hip = _hip_runtime()
    hip.hipGraphGetNodes.restype = ctypes.c_int
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    del graph
    return n.value


@pytest.mark.parametrize("route,n_stepping,launches", [("loss", 3, 2), ("loss", 16, 2), ("loss", 19, 7), ("grad", 3, 2), ("grad", 19, 4), ("none", 3, 2)])
def test_launch_counts_do_not_change_with_the_ema(route, n_stepping, launches):
    """Counted as nodes of a captured graph. LossScaler, up to 16 tensors: check + update = 2; 19 tensors: 2 checks, the decision, 2 x
    (record + update) = 7. torch's GradScaler (its found_inf / grad_scale handed over as GradScaler.step does) and no scaler: (record +
    update) per group. With an EMA over the same tensors: the same counts; a tracked tensor outside the step: one launch more."""
    params, outsider, lr, opt, scaler, EMA = _small(50, n_stepping)
    ema, ema_out = EMA(params, DECAY), EMA(params + [outsider], DECAY)
    opt.init_state(scaler, ema=ema)
    opt.init_state(ema=ema_out)
    for p in params:
        p.grad = torch.zeros_like(p)
    if route == "grad":
        opt.grad_scale, opt.found_inf = torch.full((), 1024.0, device="cuda"), torch.zeros((), device="cuda")
    kw = dict(scaler=scaler) if route == "loss" else {}
    plain = _captured_kernels(lambda: opt.step(**kw))
    with_ema = _captured_kernels(lambda: opt.step(ema=ema, **kw))
    with_out = _captured_kernels(lambda: opt.step(ema=ema_out, **kw))
    print(f"{route} {n_stepping} tensors: {plain} launches, {with_ema} with the EMA, {with_out} with a tracked tensor outside the step")
    assert plain == launches and with_ema == launches and with_out == launches + 1
    bare = _captured_kernels(lambda: ema_out.update())
    assert bare == (n_stepping + 1 + 15) // 16


# ---------------------------------------------------------------- the schedule on the device
def test_schedule_across_170_on_the_device():
    """num_updates = 168 through load_state_dict, then n = 169 .. 172 by the bare update and by the step's record (lr = 0: the parameter
    stays -1). s = 0, p = -1 leaves s = -omd: the fp32 bits of the device's 1 - decay_t against Python's double arithmetic."""
    import numpy as np
    from focnerf_amd import FusedAdam, LossScaler, ParameterEMA
    for how in ("update", "step", "step_grad_scaler_form"):
        p = torch.nn.Parameter(torch.full((1,), -1.0, device="cuda"))
        ema = ParameterEMA([p], DECAY)
        ema.load_state_dict({"decay": DECAY, "num_updates": 168, "shadow_params": [torch.zeros(1)], "collected_params": None})
        assert ema.shadow_params[0].is_cuda
        opt, scaler = FusedAdam([p], lr=0.0, betas=BETAS, eps=EPS), LossScaler(init_scale=2.0)
        for n in (169, 170, 171, 172):
            ema.shadow_params[0].zero_()
            p.grad = torch.ones_like(p)
            if how == "update":
                ema.update()
            elif how == "step":
                opt.step(scaler=scaler, ema=ema)
            else:
                opt.step(ema=ema)
            want = np.float32(1.0 - min(DECAY, (1 + n) / (10 + n)))
            got = (-ema.shadow_params[0]).cpu().numpy()
            assert float(p.detach()) == -1.0 and got.view(np.uint32)[0] == want.view(np.uint32), (how, n, float(got[0]), float(want))
            assert ema.num_updates == n


# ---------------------------------------------------------------- the real path
def test_real_training_and_render_path():
    """NeRFNetwork(bound=1) on the fused fixed-step training path, three steps with the EMA in the step; then fused renders: under
    average_parameters() = a fresh model loaded with the shadows, != the raw parameters' render; after the context = the raw render again
    — also with one half_cache_scope open around all of it, where the fp16 weight copies are kept and copy_to / restore must drop them."""
    import focnerf_amd
    from focnerf_amd import FusedAdam, LossScaler, ParameterEMA, synthetic
    from focnerf_amd.field import half_cache_scope
    from focnerf_amd.network import NeRFNetwork

    torch.manual_seed(6)
    gen = torch.Generator().manual_seed(6)
    m = NeRFNetwork(bound=1).cuda().train()
    poses = synthetic.rand_poses(1, "cuda", radius=2.0, generator=gen)
    ro, rd = synthetic.get_rays(poses, synthetic.intrinsics(8, 8), 8, 8)
    target = torch.rand(1, ro.shape[1], 3, generator=gen).cuda()
    opt = FusedAdam(m.get_params(1e-2), betas=BETAS, eps=EPS)
    scaler = LossScaler(init_scale=1024.0)
    ema = ParameterEMA(m.parameters(), DECAY)
    twin = [s.clone() for s in ema.shadow_params]
    params = list(m.parameters())
    with focnerf_amd.deterministic():
        for it in range(3):
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.run(ro, rd, None, fused=True, num_steps=64, upsample_steps=0, bg_color=1.0, perturb=False)
                loss = torch.nn.functional.mse_loss(out["image"], target)
            scaler.scale(loss).backward()
            opt.step(scaler=scaler, zero_grads=True, ema=ema)
            one_minus_decay = 1.0 - ema_ref.decay_at(DECAY, it + 1)
            for p, s in zip(params, twin):
                tmp = s - p.detach()
                tmp.mul_(one_minus_decay)
                s.sub_(tmp)
        assert ema.num_updates == 3 and all(_same(s, t) for s, t in zip(ema.shadow_params, twin))
        assert any(float((s - p.detach()).abs().max()) > 0 for s, p in zip(ema.shadow_params, params))

        def render(model):
            model.eval()
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                return model.render(ro, rd, staged=True, max_ray_batch=40, num_steps=64, upsample_steps=0, perturb=False, fused=True, bg_color=1.0)["image"].clone()

        fresh = NeRFNetwork(bound=1).cuda()
        for q, s in zip(fresh.parameters(), ema.shadow_params):
            q.data.copy_(s)
        want_avg, want_raw = render(fresh), render(m)
        assert not torch.equal(want_avg, want_raw)
        with ema.average_parameters():
            assert torch.equal(render(m), want_avg)
        assert torch.equal(render(m), want_raw)
        with half_cache_scope():
            assert torch.equal(render(m), want_raw)
            with ema.average_parameters():
                assert torch.equal(render(m), want_avg), "copy_to() inside an open half_cache_scope: the fp16 copies are made again"
            assert torch.equal(render(m), want_raw), "restore() inside an open half_cache_scope: the fp16 copies are made again"
