"""GPU: the differentiable depth of the occupancy-grid training tail (foc_occ_tail_forward_depth / _backward_depth, the node's
FocOccTrainTail companion, run_cuda(..., depth_grad=True)) against the float64 statement of tests/depth_ref.py through the raw ABI, so that
no MLP noise enters, then through the networks.

Cases: depth_ref.cases() — ragged_ref.train_cases() (lengths 0..1024, stops at samples 0, 62, 63, 64, 127, 128 and the last one, T_thresh
1e-4 / 1e-3 / 1e-2 / 0, rays that do not fit, a permuted ray index) with nears / fars replaced so that three rays of four are unclamped
(test_depth_ref.py asserts, on the reference alone, that every clamp and every constructed stop is decided) — with and without the
criterion, c_width 4 / 16.

Bound per element: |kernel - float64| <= C * 2^-24 * (T + K) * mag, C = 2, K = 16 (+ half an fp16 ulp on the fp16 gradients, + (T + K) 2^-126
on fp32 values), mag from depth_ref (the families' own magnitudes plus the depth's terms). A ray must match at ONE of the stops float64
cannot exclude. Every pre-existing output of the _depth forward is bit for bit the plain / _sumsq / _dist entry point's, the _depth backward
with grad_depth NULL or 0 is the plain backward's bits, a ray that is clamped or whose own grad_depth is 0 has the plain rows, rows behind a
stop carry no depth gradient, guard elements around depth_raw keep their sentinel.

The struct's layout against gcc's (tests/test_abi.py) and the host-side refusals (tests/test_depth_ref.py) need no GPU.

Through the network the depth does not depend on the colour network (t, near and far carry no gradient, the weights are the density's): a
depth-only loss gives a non-zero gradient on the embeddings and the density blob and an exactly zero one on the colour blob and the object
feature; with an image term beside it every parameter has one, and the depth term changes the embeddings' and the density blob's alone.

Measured on MI355X over every case of this file, worst ratio |kernel - float64| / (2^-24 (T + K) mag) per output (asserted C = 2):
    depth_raw 0.030, grad_h0 0.00063, grad_c 0.0022 — the same with the distortion and the criterion in the launch (ray_dist 0.031, ray_wm 0.030)
    (the pre-existing outputs: weights_sum / image_raw 0.031, image 0.018, sumsq 0.020, depth 0.026 on the replaced nears / fars).
A margin of 65 x at the least, C = 2 is enough. What the bound still notices: test_depth_ref.py's mutants on the fp32 CPU evaluation of the
same cases (the depth term left out: 1284). Wall time of the file: 6.6 s for its 15 tests.
"""
import numpy as np
import pytest
import torch

import depth_ref as DR
import distortion_ref as D
import ragged_ref as R
from depth_ref import C
from util import to_np

pytestmark = pytest.mark.gpu

CASES = DR.cases()
IDS = [d["name"] for d in CASES]
SENTINEL = 0x7FC0BEEF
WORST = {}
_REF = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    return torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")


def _inner(buf):
    b = to_np(buf)
    assert b[0] == SENTINEL and b[-1] == SENTINEL, "guard elements around a per-ray output"
    assert (b[1:-1] != SENTINEL).all(), "every ray's element is written"
    return b[1:-1].view(np.float32)


def _ptr1(buf):
    import ctypes
    return ctypes.c_void_p(buf.data_ptr() + 4)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _candidates(d):
    if d["name"] not in _REF:
        vals, mags, fwd = R.evaluate(d, "tail", None, mags=True)
        _REF[d["name"]] = R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]
    return _REF[d["name"]]


# ---------------------------------------------------------------- raw ABI
@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_occ_tail_depth_against_float64(d):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    j = IDS.index(d["name"])
    c_width = (4, 16)[j % 2]
    N, M, thr, ds = d["N"], d["M"], d["T_thresh"], d["density_scale"]
    rng = np.random.default_rng(5)
    h = rng.normal(0, 1, (M, 16)).astype(np.float16)
    h[:, 0] = d["h0"]
    c = (rng.normal(0, 1, (M, c_width)) * 30).astype(np.float16)
    c[:, :3] = d["c"]
    ht, ct, dt, yt = _cuda(h), _cuda(c), _cuda(d["deltas"]), _cuda(d["rays"])
    nt, ft, bt = _cuda(d["nears"]), _cuda(d["fars"]), _cuda(d["bg"])
    counter = torch.tensor([d["total"], N], dtype=torch.int32, device="cuda")
    cands, L = _candidates(d)
    gdep, gdist = d["grad_depth"], D.grad_dist_of(d)
    gdept, gdistt = _cuda(gdep), _cuda(gdist)
    st = stream_of(ht)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device="cuda")
    names = ("weights_sum", "image_raw", "image", "depth")
    fresh = lambda crit: {k: nan(N, 3) if "image" in k else nan(N) for k in names + (("sumsq",) if crit else ())}
    inside = np.zeros(M, bool)
    inside[L["rows"][L["valid"]]] = True
    for crit in (False, True):
        plain, o, od, o3 = fresh(crit), fresh(crit), fresh(crit), fresh(crit)
        args = lambda q: (ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), M, N, thr, ds, ptr(bt), R.BG_SCALAR, ptr(nt), ptr(ft), ptr(q["weights_sum"]),
                          ptr(q["image_raw"]), ptr(q["image"]), ptr(q["depth"]))
        if crit:
            check(lib.foc_occ_tail_forward_sumsq(*args(plain), ptr(plain["sumsq"]), st), "fwd_sumsq")
        else:
            check(lib.foc_occ_tail_forward(*args(plain), st), "fwd")
        draw = _guarded(N)
        check(lib.foc_occ_tail_forward_depth(*args(o), ptr(o.get("sumsq")), None, None, _ptr1(draw), st), "fwd_depth")
        dist0, wm0, dist, wm, draw3 = _guarded(N), _guarded(N), _guarded(N), _guarded(N), _guarded(N)
        check(lib.foc_occ_tail_forward_dist(*args(od), ptr(od.get("sumsq")), _ptr1(dist0), _ptr1(wm0), st), "fwd_dist")
        check(lib.foc_occ_tail_forward_depth(*args(o3), ptr(o3.get("sumsq")), _ptr1(dist), _ptr1(wm), _ptr1(draw3), st), "fwd_depth+dist")
        for k, v in plain.items():
            assert torch.equal(_bits(v), _bits(o[k])) and torch.equal(_bits(v), _bits(o3[k])), f"{k} of the _depth forward is the plain forward's"
        assert torch.equal(dist0, dist) and torch.equal(wm0, wm) and torch.equal(draw, draw3), "ray_dist / ray_wm are the _dist forward's, depth_raw its own"
        got_raw = _inner(draw)
        fwd_got = {k: R.by_list(L, to_np(v)) for k, v in o.items()}
        fwd_got["depth_raw"] = R.by_list(L, got_raw)
        assert not fwd_got["depth_raw"][~L["fits"]].any(), "rays that do not fit: exactly 0"
        on = R.TERMS if crit else R.TERMS[:2]
        g = R.grads_of(d, on, "tail")
        gi, gw = _cuda(g["grad_image"]), _cuda(g["grad_ws"])
        gq = _cuda(g["grad_sumsq"]) if crit else None

        def bwd(entry, *extra):
            grad_c, grad_h0 = nan(M, c_width, dtype=torch.float16), nan(M, dtype=torch.float16)
            check(entry(ptr(gi), ptr(gw), ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), ptr(counter), ptr(o["weights_sum"]), ptr(o["image_raw"]), M, N, thr, ds,
                        ptr(bt), R.BG_SCALAR, ptr(grad_c), ptr(grad_h0), *extra, st), "bwd")
            return grad_c, grad_h0

        def depth_bwd(gd_dist, gd_depth):
            return bwd(lib.foc_occ_tail_backward_depth, ptr(gq), _ptr1(wm) if gd_dist is not None else None, _ptr1(dist) if gd_dist is not None else None,
                       ptr(gd_dist), ptr(nt), ptr(ft), _ptr1(draw), ptr(gd_depth))

        def measure(tag, grad_c, grad_h0, with_dist):
            gc, gh = to_np(grad_c).astype(np.float64), to_np(grad_h0).astype(np.float64)
            assert not np.isnan(gc).any() and not np.isnan(gh).any(), "every row is written"
            assert not gc[:, 3:].any() and not gc[~inside].any() and not gh[~inside].any()
            got = dict(fwd_got, grad_h0=R.gather(L, gh), grad_c=R.gather(L, gc[:, :3]))
            if with_dist:
                got.update(ray_dist=R.by_list(L, _inner(dist)), ray_wm=R.by_list(L, _inner(wm)))

            def want(stops):
                key = (d["name"], crit, with_dist, tuple(int(x) for x in stops))
                if key not in _REF:
                    _REF[key] = DR.evaluate(d, stops, on=on, grad_depth=gdep, grad_dist=gdist if with_dist else None, mags=True)[:2]
                v, m = _REF[key]
                return ({k: x for k, x in v.items() if crit or k != "sumsq"}, m)
            best, chosen, per = R.match(cands, want, got, L)
            for k, v in per.items():
                WORST[f"{tag}.{k}"] = max(WORST.get(f"{tag}.{k}", 0.0), v)
            print(d["name"], tag, "crit", crit, per)
            assert best.max() <= C, (tag, crit, per, int(np.argmax(best)))
            behind = inside.copy()
            behind[L["rows"][L["valid"] & (L["col"] <= np.asarray(chosen)[:, None])]] = False
            assert not gc[behind].any() and (crit or not gh[behind].any()), "behind a stop: no depth gradient"
            return behind

        grad_c, grad_h0 = depth_bwd(None, gdept)
        behind = measure("depth", grad_c, grad_h0, False)
        # grad_depth NULL, and 0 on every ray: the plain backward's bits
        p_c, p_h0 = bwd(lib.foc_occ_tail_backward_sumsq, ptr(gq)) if crit else bwd(lib.foc_occ_tail_backward)
        for gz in (torch.zeros(N, device="cuda"), None):
            z_c, z_h0 = depth_bwd(None, gz)
            assert torch.equal(_bits(z_c), _bits(p_c)) and torch.equal(_bits(z_h0), _bits(p_h0)), "grad_depth = 0 / NULL: the plain backward"
        assert torch.equal(_bits(grad_c), _bits(p_c)), "the depth does not depend on the colour"
        # a ray that is clamped, or whose own grad_depth is 0, has the plain rows; so do the rows behind a stop
        quiet_ray = R.by_list(L, d["clamped"] | (gdep == 0))
        quiet = np.zeros(M, bool)
        quiet[L["rows"][L["valid"] & quiet_ray[:, None]]] = True
        quiet |= behind | ~inside
        a, b = to_np(_bits(grad_h0)), to_np(_bits(p_h0))
        assert np.array_equal(a[quiet], b[quiet])
        loud = L["fits"] & ~quiet_ray
        if loud.any():
            assert (a[~quiet] != b[~quiet]).any(), "an unclamped ray with a depth gradient differs from the plain backward"
        # depth + distortion (+ criterion) in one launch against the float64 sum of the terms
        grad_c, grad_h0 = depth_bwd(gdistt, gdept)
        measure("depth+dist", grad_c, grad_h0, True)
        d_c, d_h0 = bwd(lib.foc_occ_tail_backward_dist, ptr(gq), _ptr1(wm), _ptr1(dist), ptr(gdistt))
        z_c, z_h0 = depth_bwd(gdistt, None)
        assert torch.equal(_bits(z_c), _bits(d_c)) and torch.equal(_bits(z_h0), _bits(d_h0)), "grad_depth NULL beside grad_dist: the _dist backward"
        _inner(draw), _inner(dist), _inner(wm)                            # the backwards left the guards alone too


def test_worst_ratios_are_reported():
    """Runs last in the file: prints what the docstring's table is made of."""
    print("worst ratios", {k: round(v, 5) for k, v in sorted(WORST.items())})


# ---------------------------------------------------------------- through the networks
def _model(kind):
    from focnerf_amd import network, network_foc, synthetic
    torch.manual_seed(0)
    m = {"plain": network.NeRFNetwork, "foc": network_foc.NeRFNetwork}[kind](bound=2, cuda_ray=True).cuda()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    m.set_density_grid(synthetic.analytic_density_grid(2, device="cuda"))
    return m.train()


@pytest.mark.parametrize("kind", ["plain", "foc"])
def test_run_cuda_depth_grad(kind, monkeypatch, lib_option):
    """One occupancy batch of 37 rays on network.NeRFNetwork and on network_foc.NeRFNetwork with a ray mask (module docstring)."""
    from focnerf_amd import synthetic
    from focnerf_amd._lib import lib
    lib_option("FOC_DETERMINISTIC", 1)                                    # the bit comparisons below: no atomics in the encoder's backward
    m = _model(kind)
    o, d = synthetic.make_view_rays(64, 64, 2, 1, seed=0, device="cuda")
    pick = torch.randperm(o.shape[1], generator=torch.Generator().manual_seed(1))[:37].cuda()
    o, d = o[:, pick].contiguous(), d[:, pick].contiguous()
    yolo = ()
    if kind == "foc":
        g = torch.Generator().manual_seed(5)
        yolo = (((torch.rand(1, 37, generator=g) < 0.5).cuda(), None, torch.randn(144, generator=g).cuda()),)
    kw = dict(staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=True, force_all_rays=False)
    calls = {n: 0 for n in ("foc_occ_train_forward_tail", "foc_occ_train_backward_tail", "foc_occ_tail_forward_depth", "foc_occ_tail_backward_depth")}
    for n in calls:
        real = getattr(lib, n)
        monkeypatch.setattr(lib, n, lambda *a, _r=real, _n=n: (calls.__setitem__(_n, calls[_n] + 1), _r(*a))[1])
    target = torch.linspace(0.1, 0.9, 37, device="cuda").view(1, 37)

    def step(w_image, w_depth, w_dist=0.0, **extra):
        for p in m.parameters():
            p.grad = None
        kept = {}
        if kind == "foc":
            def encode(y, dev):
                kept["obj16"] = type(m).encode_object_feature(m, y, dev)
                kept["obj16"].retain_grad()
                return kept["obj16"]
            m.encode_object_feature = encode
        try:
            torch.manual_seed(7)
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.render(o, d, *yolo, **kw, **extra)
                loss = 0.0
                if w_image:
                    loss = loss + w_image * torch.nn.functional.mse_loss(out["image"], 0.5 + 0.5 * torch.sin(3.0 * d))
                    if out.get("criterion_outside_mask") is not None:
                        loss = loss + 1e-3 * out["criterion_outside_mask"]
                if w_depth:
                    loss = loss + w_depth * torch.nn.functional.mse_loss(out["depth"], target)
                if w_dist:
                    loss = loss + w_dist * out["distortion"].mean()
            (loss * 1024.0).backward()
        finally:
            if kind == "foc":
                del m.encode_object_feature
        grads = {n: (p.grad.clone() if p.grad is not None else None) for n, p in
                 (("embeddings", m.encoder.embeddings), ("sigma_net", m.sigma_net.weights), ("color_net", m.color_net.weights))}
        if kind == "foc":
            grads["obj16"] = kept["obj16"].grad.clone() if kept["obj16"].grad is not None else None
        return out, grads

    def same(a, b, what):
        out_a, g_a = a
        out_b, g_b = b
        assert set(out_a) == set(out_b), what
        for k in out_a:
            if torch.is_tensor(out_a[k]):
                assert torch.equal(out_a[k], out_b[k]), (what, k)
        for n in g_a:
            assert torch.equal(g_a[n], g_b[n]), (what, n)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        m.render(o, d, *yolo, **dict(kw, perturb=False, force_all_rays=True))       # fills step_counter
    m.mean_count = int(m.step_counter[(m.local_step - 1) % 16, 0]) + 500      # a sample budget: the one-call route (tests/test_gpu_occtrain.py)
    assert m.mean_count > 1000
    plain = step(1.0, 0.0)
    assert not plain[0]["depth"].requires_grad and not any(calls.values())
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, *yolo, **kw)
    with pytest.raises(RuntimeError, match="does not require grad"):
        out["depth"].sum().backward()
    # the keyword: depth requires grad, the one-call route carries it; zero weight on the depth: the plain call's bits
    zero = step(1.0, 0.0, depth_grad=True)
    assert zero[0]["depth"].requires_grad and calls["foc_occ_train_forward_tail"] == 1 and calls["foc_occ_train_backward_tail"] == 1
    assert not calls["foc_occ_tail_forward_depth"]
    same(plain, zero, "depth_grad=True with no weight on the depth")
    assert (kind == "foc") == (zero[0].get("criterion_outside_mask") is not None)
    # a depth-only loss
    out, g = step(0.0, 1.0, depth_grad=True)
    assert out["depth"].shape == (1, 37) and bool((out["depth"] > 0).any())
    assert float(g["embeddings"].abs().max()) > 0 and float(g["sigma_net"].abs().max()) > 0
    for n in ("color_net", "obj16"):                                      # the depth does not depend on the colour network or its inputs
        assert n not in g or (g[n] is not None and not g[n].any()), n
    # beside an image term every parameter has a gradient, and the depth term moves the density side alone
    both = step(1.0, 1.0, depth_grad=True)
    for n, v in both[1].items():
        assert float(v.abs().max()) > 0, n
    assert not torch.equal(both[1]["embeddings"], plain[1]["embeddings"]) and not torch.equal(both[1]["sigma_net"], plain[1]["sigma_net"])
    # the one-call route against the call-by-call chain, and a repeated step, bit for bit: depth, distortion, both
    for extra, w_dist in ((dict(depth_grad=True), 0.0), (dict(distortion=True), 10.0), (dict(depth_grad=True, distortion=True), 10.0)):
        w_depth = 1.0 if "depth_grad" in extra else 0.0
        before = dict(calls)
        one = step(1.0, w_depth, w_dist, **extra)
        again = step(1.0, w_depth, w_dist, **extra)
        assert calls["foc_occ_train_forward_tail"] == before["foc_occ_train_forward_tail"] + 2
        monkeypatch.setenv("FOC_OCC_NATIVE_NODE", "0")
        before = dict(calls)
        chain = step(1.0, w_depth, w_dist, **extra)
        monkeypatch.delenv("FOC_OCC_NATIVE_NODE")
        assert calls["foc_occ_train_forward_tail"] == before["foc_occ_train_forward_tail"], "FOC_OCC_NATIVE_NODE=0: the chain"
        assert (calls["foc_occ_tail_backward_depth"] == before["foc_occ_tail_backward_depth"] + 1) == ("depth_grad" in extra)
        same(one, again, f"{extra}: the step repeated")
        same(one, chain, f"{extra}: one call against call by call")
        assert ("distortion" in one[0]) == ("distortion" in extra)
    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(ValueError, match="depth_grad=True needs the fused occupancy training node"):
        m.render(o, d, *yolo, **kw, depth_grad=True)
    monkeypatch.delenv("FOC_FUSED_OCC")
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), pytest.raises(ValueError, match="depth_grad=True needs the fused occupancy training node"):
        m.render(o, d, *yolo, **kw, depth_grad=True)
    # run() takes the keyword and ignores it: its depth is always differentiable
    if kind == "plain":
        m.train()
        with torch.autocast("cuda", dtype=torch.float16):
            assert m.run(o, d, num_steps=16, depth_grad=True)["depth"].requires_grad
