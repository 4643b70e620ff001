"""GPU: the ray distortion of the training tails (foc_fixed_tail_forward_dist / _backward_dist, foc_occ_tail_forward_dist / _backward_dist)
against the float64 reference of tests/distortion_ref.py through the raw ABI, so that no MLP noise enters, then through the networks.

Cases: the fixed-step draws of test_gpu_fixed_tail_reference.py at T in {2, 63, 64, 65, 128, 129, 200} x N in {1, 3, 4, 5, 37} (transparent,
typical, opaque, clamp and box-missing rays) in two configurations — noise, sums of sigma^2, per-ray background, c_width 4, density_scale 1 /
none of them, c_width 16, density_scale 3; ragged_ref.train_cases() (lengths 0..1024, stops at samples 0, 62, 63, 64, 127, 128 and the last
one, T_thresh 1e-4 / 1e-3 / 1e-2 / 0, rays that do not fit, a permuted ray index) with and without the criterion, c_width 4 / 16.

Bound per element: |kernel - float64| <= C * 2^-24 * (T + K) * mag, C = 2, K = 16 (+ half an fp16 ulp on the fp16 gradients, + (T + K) 2^-126
on fp32 values), mag from distortion_ref (the families' own magnitudes plus the distortion's terms). A ragged ray must match at ONE of the
stops float64 cannot exclude; at most 2 % of a case's rays, none of a constructed case's, are undecided (asserted on the reference alone).
Every pre-existing output of the _dist forward is bit for bit the plain entry point's, the _dist backward with grad_dist = 0 is the plain
backward's bits, guard elements around ray_dist / ray_wm keep their sentinel.

Measured on MI355X over every case of this file, worst ratio |kernel - float64| / (2^-24 (T + K) mag) per output (asserted C = 2):
    fixed-step: ray_dist 0.020, ray_wm 0.024, grad_h0 0.034          ragged: ray_dist 0.031, ray_wm 0.030, grad_h0 0.00065, grad_c 0.0022
    (the pre-existing outputs as in test_gpu_ragged_reference.py: weights_sum / image_raw 0.031, image 0.018, sumsq 0.020, depth 0.0005).
A margin of 59 x at the least, C = 2 is enough. What the bound still notices (fp32 CPU evaluation of the same cases, test_distortion_ref.py's
machinery): the distortion gradient left out gives ratios of 59 .. 222 (102 on the fixed-step layout), a grad_dist off by 1 % gives 0.6 ..
2.2. Wall time of the file: 6.5 s for its 31 tests.
"""
import numpy as np
import pytest
import torch

import distortion_ref as D
import ragged_ref as R
from distortion_ref import C
from util import to_np

pytestmark = pytest.mark.gpu

CASES = R.train_cases()
IDS = [d["name"] for d in CASES]
SENTINEL = 0x7FC0BEEF
WORST = {}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n):
    """[n + 2] int32 filled with the sentinel; the kernels get the n elements in the middle."""
    return torch.full((n + 2,), SENTINEL, dtype=torch.int32, device="cuda")


def _inner(buf):
    b = to_np(buf)
    assert b[0] == SENTINEL and b[-1] == SENTINEL, "guard elements around a per-ray output"
    assert (b[1:-1] != SENTINEL).all(), "every ray's element is written"
    return b[1:-1].view(np.float32)


def _ptr1(buf):
    import ctypes
    return ctypes.c_void_p(buf.data_ptr() + 4)


def _record(tag, k, r):
    r = float(np.max(r, initial=0.0))
    WORST[f"{tag}.{k}"] = max(WORST.get(f"{tag}.{k}", 0.0), r)
    return r


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


# ---------------------------------------------------------------- fixed-step tail, raw ABI
@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("T", D.FIXED_T)
def test_fixed_tail_distortion_against_float64(T, cfg):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from test_gpu_fixed_tail_reference import _reference, _tail_bwd, _tail_fwd
    for N in D.FIXED_N:
        d, g, gd, o = D.fixed_case(N, T, cfg)
        M = N * T
        t, plain = _tail_fwd(d, N, T, o["c_width"], noise=o["noise"], sumsq=o["sumsq"], bg_ray=o["bg_ray"], ds=o["ds"], thresh=o["thresh"])
        out = {k: (torch.full_like(v, float("nan")) if v is not None else None) for k, v in plain.items()}
        dist, wm = _guarded(N), _guarded(N)
        st = stream_of(t["h"])
        check(lib.foc_fixed_tail_forward_dist(ptr(t["h"]), ptr(t["c"]), ptr(t["near"]), ptr(t["far"]), ptr(t["noise"]), ptr(t["bg"]), 0.7, N, T, o["ds"],
                                              o["thresh"], ptr(out["sigma"]), ptr(out["trans"]), ptr(out["weights"]), ptr(out["weights_sum"]),
                                              ptr(out["depth"]), ptr(out["image"]), o["c_width"], ptr(out["sumsq"]), _ptr1(dist), _ptr1(wm), st), "fwd_dist")
        for k, v in plain.items():
            if v is not None:
                assert torch.equal(_bits(v), _bits(out[k])), f"{k} of the _dist forward is the plain forward's"
        got_dist, got_wm = _inner(dist), _inner(wm)
        mask = to_np(out["weights"]).reshape(N, T) > o["thresh"]
        ref = _reference(d, t, N, T, o["ds"], mask, bg_ray=o["bg_ray"])
        dd = D.fixed(ref)
        mags = D.fixed_magnitudes(ref, dd, gd, **g)
        tag = f"fixed[{N}x{T},{cfg}]"
        for k, got, key in (("ray_dist", got_dist, "dist"), ("ray_wm", got_wm, "wm")):
            r = _record("fixed", k, R.ratios(got, dd[key].detach().numpy(), mags[key].numpy(), T))
            print(tag, k, r)
            assert r <= C, (tag, k, r)
        assert not got_dist[d["missed"]].any() and not got_wm[d["missed"]].any(), "a ray that misses the box: exactly 0"
        # backward: all the family's terms of this configuration plus grad_dist
        gt = {k: _cuda(v) for k, v in g.items()}
        gdt = _cuda(gd)
        grad_c = torch.full((M, o["c_width"]), float("nan"), dtype=torch.float16, device="cuda")
        grad_h0 = torch.full((M,), float("nan"), dtype=torch.float16, device="cuda")

        def bwd(gdist, grad_c, grad_h0):
            check(lib.foc_fixed_tail_backward_dist(ptr(gt["grad_image"]), ptr(gt.get("grad_ws")), ptr(gt.get("grad_depth")), ptr(t["c"]), ptr(out["sigma"]),
                                                   ptr(out["trans"]), ptr(out["weights"]), ptr(out["weights_sum"]), ptr(t["near"]), ptr(t["far"]),
                                                   ptr(t["noise"]), ptr(t["bg"]), 0.7, N, T, o["ds"], o["thresh"], ptr(grad_c), ptr(grad_h0), o["c_width"],
                                                   ptr(gt.get("grad_sumsq")), _ptr1(wm), _ptr1(dist), ptr(gdist), st), "bwd_dist")
        bwd(gdt, grad_c, grad_h0)
        want = D.fixed_backward(ref, dd, gd, **g)
        live = ~d["missed"]                                               # a missed ray's rows are NaN under a depth gradient: the family's own test
        gh = to_np(grad_h0).astype(np.float64).reshape(N, T)
        gc = to_np(grad_c).astype(np.float64)[:, :3].reshape(N, T, 3)
        r = _record("fixed", "grad_h0", R.ratios(gh[live], want["grad_h0"].numpy()[live], mags["grad_h0"].numpy()[live], T, half=True))
        print(tag, "grad_h0", r)
        assert r <= C, (tag, "grad_h0", r)
        r = _record("fixed", "grad_c", R.ratios(gc[live], want["grad_c"].numpy()[live], mags["grad_c"].numpy()[live], T, half=True))
        assert r <= C, (tag, "grad_c", r)
        # grad_dist = 0 on every ray, and NULL: the plain backward's bits
        p_c, p_h0 = _tail_bwd(t, plain, {k: g.get(k) for k in ("grad_image", "grad_ws", "grad_depth", "grad_sumsq")}, N, T, o["c_width"], o["ds"], o["thresh"])
        for gz in (torch.zeros(N, device="cuda"), None):
            z_c, z_h0 = torch.full_like(grad_c, float("nan")), torch.full_like(grad_h0, float("nan"))
            bwd(gz, z_c, z_h0)
            assert torch.equal(_bits(z_c), _bits(p_c)) and torch.equal(_bits(z_h0), _bits(p_h0)), "grad_dist = 0 / NULL: the plain backward"
        # a ray whose own grad_dist is 0 has the plain backward's rows
        quiet = np.repeat(gd == 0, T)
        assert np.array_equal(to_np(_bits(grad_h0))[quiet], to_np(_bits(p_h0))[quiet])


# ---------------------------------------------------------------- ragged tail, raw ABI
_REF = {}


def _candidates(d):
    if d["name"] not in _REF:
        vals, mags, fwd = R.evaluate(d, "tail", None, mags=True)
        _REF[d["name"]] = R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]
    return _REF[d["name"]]


def test_undecided_cap_on_the_reference():
    for d in CASES:
        cands, _ = _candidates(d)
        n = sum(len(c) > 1 for c in cands)
        assert n <= 0.02 * d["N"] and ("stops" not in d or n == 0), (d["name"], n)


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_occ_tail_distortion_against_float64(d):
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
    gd = D.grad_dist_of(d)
    gdt = _cuda(gd)
    st = stream_of(ht)
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device="cuda")
    for crit in (False, True):
        names = ("weights_sum", "image_raw", "image", "depth")
        plain, o = {k: nan(N, 3) if "image" in k else nan(N) for k in names}, {k: nan(N, 3) if "image" in k else nan(N) for k in names}
        args = lambda q: (ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), M, N, thr, ds, ptr(bt), R.BG_SCALAR, ptr(nt), ptr(ft), ptr(q["weights_sum"]),
                          ptr(q["image_raw"]), ptr(q["image"]), ptr(q["depth"]))
        dist, wm = _guarded(N), _guarded(N)
        if crit:
            plain["sumsq"], o["sumsq"] = nan(N), nan(N)
            check(lib.foc_occ_tail_forward_sumsq(*args(plain), ptr(plain["sumsq"]), st), "fwd_sumsq")
        else:
            check(lib.foc_occ_tail_forward(*args(plain), st), "fwd")
        check(lib.foc_occ_tail_forward_dist(*args(o), ptr(o.get("sumsq")), _ptr1(dist), _ptr1(wm), st), "fwd_dist")
        for k, v in plain.items():
            assert torch.equal(_bits(v), _bits(o[k])), f"{k} of the _dist forward is the plain forward's"
        got_dist, got_wm = _inner(dist), _inner(wm)
        fwd_got = {k: R.by_list(L, to_np(v)) for k, v in o.items()}
        fwd_got.update(ray_dist=R.by_list(L, got_dist), ray_wm=R.by_list(L, got_wm))
        assert not fwd_got["ray_dist"][~L["fits"]].any() and not fwd_got["ray_wm"][~L["fits"]].any(), "rays that do not fit: exactly 0"
        on = R.TERMS if crit else R.TERMS[:2]
        g = R.grads_of(d, on, "tail")
        gi, gw = _cuda(g["grad_image"]), _cuda(g["grad_ws"])
        gq = _cuda(g["grad_sumsq"]) if crit else None

        def bwd(entry, *extra):
            grad_c, grad_h0 = nan(M, c_width, dtype=torch.float16), nan(M, dtype=torch.float16)
            check(entry(ptr(gi), ptr(gw), ptr(ht), ptr(ct), c_width, ptr(dt), ptr(yt), ptr(counter), ptr(o["weights_sum"]), ptr(o["image_raw"]), M, N, thr, ds,
                        ptr(bt), R.BG_SCALAR, ptr(grad_c), ptr(grad_h0), *extra, st), "bwd")
            return grad_c, grad_h0
        grad_c, grad_h0 = bwd(lib.foc_occ_tail_backward_dist, ptr(gq), _ptr1(wm), _ptr1(dist), ptr(gdt))
        gc, gh = to_np(grad_c).astype(np.float64), to_np(grad_h0).astype(np.float64)
        assert not np.isnan(gc).any() and not np.isnan(gh).any(), "every row is written"
        inside = np.zeros(M, bool)
        inside[L["rows"][L["valid"]]] = True
        assert not gc[:, 3:].any() and not gc[~inside].any() and not gh[~inside].any()
        got = dict(fwd_got, grad_h0=R.gather(L, gh), grad_c=R.gather(L, gc[:, :3]))

        def want(stops):
            key = (d["name"], crit, tuple(int(x) for x in stops))
            if key not in _REF:
                _REF[key] = D.ragged_evaluate(d, stops, on=on, grad_dist=gd, mags=True)[:2]
            v, m = _REF[key]
            return ({k: x for k, x in v.items() if crit or k != "sumsq"}, m)
        best, chosen, per = R.match(cands, want, got, L)
        for k, v in per.items():
            _record("ragged", k, v)
        print(d["name"], crit, per)
        assert best.max() <= C, (crit, per, int(np.argmax(best)))
        behind = inside.copy()
        behind[L["rows"][L["valid"] & (L["col"] <= np.asarray(chosen)[:, None])]] = False
        assert not gc[behind].any() and (crit or not gh[behind].any()), "behind a stop: no distortion gradient"
        # grad_dist = 0 on every ray, and NULL: the plain backward's bits
        p_c, p_h0 = bwd(lib.foc_occ_tail_backward_sumsq, ptr(gq)) if crit else bwd(lib.foc_occ_tail_backward)
        for gz in (torch.zeros(N, device="cuda"), None):
            z_c, z_h0 = bwd(lib.foc_occ_tail_backward_dist, ptr(gq), _ptr1(wm), _ptr1(dist), ptr(gz))
            assert torch.equal(_bits(z_c), _bits(p_c)) and torch.equal(_bits(z_h0), _bits(p_h0)), "grad_dist = 0 / NULL: the plain backward"
        _inner(dist), _inner(wm)                                          # the backward left the guards alone too


# ---------------------------------------------------------------- through the networks
# Distance between the fused tail's distortion and loss.ray_distortion on the unfused route (same weights bit for bit on the fixed-step path:
# the two differ in fp32 summation order only), as max |a - b| / max |b| over the rays, and of every parameter gradient of the step (the
# routes' fp16 gradients round at different places); bounds = measured on MI355X x 1.5:
#     network.NeRFNetwork:      value 2.14e-7, gradients 1.03e-4          network_foc.NeRFNetwork (with a ray mask): value 2.14e-7, gradients 8.21e-4
PY_TOL = {"fixed.value": 3.3e-7, "fixed.grad": 1.6e-4, "foc.value": 3.3e-7, "foc.grad": 1.3e-3}


def _fixed_model(kind, seed=0):
    from focnerf_amd import network, network_foc
    torch.manual_seed(seed)
    m = {"plain": network.NeRFNetwork, "foc": network_foc.NeRFNetwork}[kind](bound=1).cuda()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m.train()


def _fixed_step(m, o, d, yolo, lam, **kw):
    for p in m.parameters():
        p.grad = None
    torch.manual_seed(3)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(o, d, yolo, staged=False, num_steps=65, upsample_steps=0, perturb=True, fused=True, **kw)
        loss = torch.nn.functional.mse_loss(out["image"], 0.5 + 0.5 * torch.sin(3.0 * d))
        if out.get("criterion_outside_mask") is not None:
            loss = loss + 1e-3 * out["criterion_outside_mask"]
        if lam:
            loss = loss + lam * out["distortion"].mean()
    (loss * 1024.0).backward()
    return out, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("kind", ["plain", "foc"])
def test_render_fixed_steps_distortion(kind, monkeypatch, lib_option):
    """render(..., fused=True, distortion=True) at 64 rays x 65 steps on network.NeRFNetwork and network_foc.NeRFNetwork (the latter with a
    ray mask: the sums of sigma^2 and the distortion leave the tail together): value and parameter gradients against the torch fallback on
    the route without the fused tail; without the keyword the result and the gradients are the plain call's bits; no gradient: ValueError."""
    from focnerf_amd import synthetic
    lib_option("FOC_DETERMINISTIC", 1)                                     # the bit comparisons below: no fp32 atomics in the encoder's backward
    m = _fixed_model(kind)
    o, d = synthetic.make_view_rays(8, 8, 1, 1, seed=1, device="cuda", radius=2.0)
    yolo = None
    if kind == "foc":
        g = torch.Generator().manual_seed(5)
        yolo = ((torch.rand(1, 64, generator=g) < 0.5).cuda(), None, torch.randn(144, generator=g).cuda())
    lam = 10.0
    fused, g_fused = _fixed_step(m, o, d, yolo, lam, distortion=True)
    assert fused["distortion"].shape == fused["depth"].shape and fused["distortion"].requires_grad
    assert (kind == "foc") == (fused["criterion_outside_mask"] is not None)
    monkeypatch.setenv("FOC_FUSED_TAIL", "0")
    ref, g_ref = _fixed_step(m, o, d, yolo, lam, distortion=True)
    monkeypatch.delenv("FOC_FUSED_TAIL")
    scale = ref["distortion"].abs().max().item()
    assert scale > 0
    dv = (fused["distortion"] - ref["distortion"]).abs().max().item() / scale
    print(kind, "distortion value distance", dv, "scale", scale)
    worst = 0.0
    for n in g_ref:
        worst = max(worst, (g_fused[n] - g_ref[n]).abs().max().item() / max(g_ref[n].abs().max().item(), 1e-30))
    print(kind, "gradient distance", worst)
    key = "fixed" if kind == "plain" else "foc"
    assert dv <= PY_TOL[key + ".value"] and worst <= PY_TOL[key + ".grad"]
    # the distortion term reaches the parameters
    _, g_zero = _fixed_step(m, o, d, yolo, 0.0, distortion=True)
    assert any((g_fused[n] != g_zero[n]).any() for n in g_zero)
    # without the keyword: the plain call, bit for bit (and the keyword adds nothing but its key)
    plain, g_plain = _fixed_step(m, o, d, yolo, 0.0)
    assert "distortion" not in plain and set(fused) - set(plain) == {"distortion"}
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(plain[k], fused[k])
    for n in g_plain:
        assert torch.equal(g_plain[n], g_zero[n]), n
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), pytest.raises(ValueError, match="distortion=True needs the training route"):
        m.render(o, d, yolo, staged=False, num_steps=65, upsample_steps=0, fused=True, distortion=True)


def test_run_fallback_distortion_matches_the_fused_tail():
    """NeRFRenderer.run (fused=False) with distortion=True: loss.ray_distortion on its autograd weights, the fused tail's value for the same
    network and rays up to the routes' own distance (the MLP kernels differ: fp16 noise on sigma)."""
    from focnerf_amd import synthetic
    m = _fixed_model("plain")
    o, d = synthetic.make_view_rays(8, 8, 1, 1, seed=1, device="cuda", radius=2.0)
    with torch.autocast("cuda", dtype=torch.float16):
        a = m.render(o, d, staged=False, num_steps=65, upsample_steps=0, perturb=False, fused=True, distortion=True)["distortion"]
        b = m.render(o, d, staged=False, num_steps=65, upsample_steps=0, perturb=False, fused=False, distortion=True)["distortion"]
    assert b.requires_grad and a.shape == b.shape
    dist = (a - b).abs().max().item() / b.abs().max().item()
    print("run() fallback distance", dist)
    # fp16 logits: where the two routes' MLP kernels round h0 differently, an ulp of h0 is 1e-3 relative on sigma, and the distortion is
    # quadratic in the weights (measured on MI355X: 3.2e-7 — the routes share their MLP kernels today)
    assert dist <= 2e-2


def test_run_cuda_distortion(monkeypatch):
    """One occupancy batch of 37 rays: run_cuda(..., distortion=True) on the fused node (call-by-call chain) returns the key, its gradient
    reaches the parameters, image and weights_sum are the bits of the call without the keyword (one-call node); FOC_FUSED_OCC=0 and the
    inference route raise ValueError."""
    from focnerf_amd import synthetic
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    m = NeRFNetwork(bound=2, cuda_ray=True).cuda()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    m.set_density_grid(synthetic.analytic_density_grid(2, device="cuda"))
    m.train()
    o, d = synthetic.make_view_rays(64, 64, 2, 1, seed=0, device="cuda")
    pick = torch.randperm(o.shape[1], generator=torch.Generator().manual_seed(1))[:37].cuda()
    o, d = o[:, pick].contiguous(), d[:, pick].contiguous()
    kw = dict(staged=False, dt_gamma=1 / 128, max_steps=1024, perturb=False, force_all_rays=False)

    def step(lam, **extra):
        for p in m.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.render(o, d, **kw, **extra)
            loss = torch.nn.functional.mse_loss(out["image"], 0.5 + 0.5 * torch.sin(3.0 * d))
            if lam:
                loss = loss + lam * out["distortion"].mean()
        (loss * 1024.0).backward()
        return out, {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    step(0.0)                                                             # fills the sample budget (mean_count)
    plain, g_plain = step(0.0)
    with_key, g_zero = step(0.0, distortion=True)
    assert with_key["distortion"].shape == (1, 37) and with_key["distortion"].requires_grad and (with_key["distortion"] >= 0).all()
    assert with_key["distortion"].abs().max() > 0 and set(with_key) - set(plain) == {"distortion"}
    assert torch.equal(plain["image"], with_key["image"]) and torch.equal(plain["weights_sum"], with_key["weights_sum"])
    _, g_dist = step(10.0, distortion=True)
    assert any((g_dist[n] != g_zero[n]).any() for n in g_zero), "the distortion term reaches the parameters"
    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    with torch.autocast("cuda", dtype=torch.float16), pytest.raises(ValueError, match="needs the fused occupancy training node"):
        m.render(o, d, **kw, distortion=True)
    monkeypatch.delenv("FOC_FUSED_OCC")
    m.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16), pytest.raises(ValueError, match="needs the fused occupancy training node"):
        m.render(o, d, **kw, distortion=True)
