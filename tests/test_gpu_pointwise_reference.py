"""GPU: the pointwise kernels against the float64 references of tests/pointwise_ref.py (error model, bounds and mutants: its docstring),
through the raw ABI (focnerf_amd._lib), every output in front of a guard band that must come back untouched.

    part 1  foc_sh_encode (fp32) and the SH columns of foc_sample_head_forward's cin (half) against the basis FROM ITS DEFINITION;
            nf_sh16_half observed through foc_nerf_field_inference with selector weights (sigma net 0, colour net routing three SH
            columns to the logits: rgb = sigmoid_h(half(SH_k(d)))), layer pairs (2, 2) and (1, 2), per-sample and blocked directions,
            and one blocked call large enough that a wave's run of tiles crosses 64-ray blocks
    part 2  csrc/head.hip: k_head_fwd, k_head_bwd, k_rgb_fwd, k_rgb_bwd, widths 32 and 48, with and without obj, NULL outputs
    part 3  the frequency encoder forward (K_SIN ulp32 of float64 sin of the exact fp32 argument) and backward
    part 4  hidden activations 1..5 of the fused MLP, layer by layer on the kernel's own fb / bb, plus EVERY finite half through each
            activation's forward and backward (an identity layer)
    probes  device sinf alone (deg = 1, D = 1 encoder) and logf through the softplus layer: they fix K_SIN and K_LOG

M of parts 1 and 2: {1, 255, 256, 257, 2048 * 256 + 1} (the last: foc_grid_1d's cap sends thread 0 round its stride loop again).
Encoder: (deg, D) in {(4, 3), (10, 3), (30, 5), (1, 100), (1, 3000)} x B in {1, 257, 1000}, and 256 * 2048 + 3 rows at (4, 3).

Routes of part 4: a call with activation 1..5 never takes the single-pass kernel (csrc/ffmlp.hip mlp_bwd_launch: `gen`), whatever
FOC_MLP_BWD_FUSED says, and hidden_dim 256 / wide inputs are other shapes than the issue's: the routes are mlp_ref's `two_kernel`
(k_mlp_bwd<H, 2, true>, k_mlp_dw<H>, k_mlp_dw_finalize) and `two_kernel_det` (FOC_DETERMINISTIC: k_mlp_dw_finalize_slots). Each test
asserts the route as test_gpu_mlp_reference._select does. The forward forms (training, inference, forward_buffer-free) must agree
bit for bit.

Measured on MI355X (256 CUs). Worst |kernel - float64| / bound, asserted <= 1; "loose share" = the finite elements within E of a half
midpoint, which keep the bound alone (asserted <= 1 %); every other element must be, and is, the rounded float64 value bit for bit:

    kernel / quantity                                   worst ratio   loose share   note
    foc_sh_encode (fp32), five sizes                    0.931         -             against the definition, n roundings per column
    foc_sample_head_forward  sigma                      0.662         -             of 2 U: expf is off by at most 0.66 ulp32 here
                             cin SH columns (half)      1.000         0.41 %        1.000 = a half-ulp rounding, E is < 1 % of the bound
                             cin columns 16 .. 47       bits                        widths 32 / 48, with / without obj, pad columns +0
    foc_sample_head_backward grad_h[:, 0]               1.000         0.05 %        clamp edges, inf, NaN, subnormal, 1e-30 .. 1e30
                             grad_h[:, 1:16]            bits                        and +0 columns for either NULL gradient
    foc_rgb_head_forward     rgb                        1.000         0.04 %        every value a half; 2^-24 / 0 either side of 2^-25
    foc_rgb_head_backward    grad_c[:, :3]              1.000         0.84 %        on the kernel's own rgb; columns 3..15 +0
    nf_sh16_half through foc_nerf_field_inference       1.000         0.06 - 0.09 % 0.5 - 0.8 % of the SH values name two halves
    foc_freq_encode_forward                             0.401         -             of K_SIN = 4 ulp32: 1.6 ulp32, deg 30 included
    foc_freq_encode_backward                            0.429         -             C = 2
    activation layers  fb (1..5)                        1.000 0.999 1.000 0.999 0.999   loose 0.03 0.57 0.07 0.27 0.10 % (x >= 0 for 4, 5)
                       bb                               bits, or between the candidates (24 - 36 % of the deltas name more than one half)
                       out / grad_inputs / grad_weights 0.986 / 0.990 / 1.000   (scales 2^-16 .. 2^8: 0.966 / 1.000 / 0.954)
    every finite half through activation 1..5           1.000 0.999 1.000 1.000 0.999   forward and backward, both bit-checked
    device sinf alone (probe)                           1.530 ulp32 over 2 636 000 arguments; |a| >= 2^20: 1.528; |a| >= 2^29: 1.475
    device logf through softplus (probe)                99.948 % of 50 288 finite outputs are the rounded float64 value and the other
                                                        roundings explain the rest: 0 ulp32 attributable to logf, K_LOG = 1

two_kernel and two_kernel_det give the same figures (the deterministic option changes the order of k_mlp_dw's chunk sums only).
69 tests; wall time of the file 8.3 s, the slowest test 1.1 s (test_head_forward at 524 289 rows; the float64 side dominates).

No kernel changed: the first run had every element inside its bound.
A build of the library with six of the mutants in the kernels themselves (an SH constant of nf_sh16_half off by 2^-18, the clamp at
14.5, o1[0] = g2[6], grad_rgb unrounded, pi/2 added in double, the sigmoid factor in fp32) fails 26 of the 69 tests, every one that runs
a mutated line except the blocked selector calls, whose triples either leave out the mutated column or (200 rays then, 1000 now) held
too few directions for a 2^-18 error to cross a half boundary; the per-sample calls catch that constant.
NOTEBOOK.md, "Pointwise kernels against float64", has the error model, the mutants and the per-binade sinf figures.
"""
import math

import numpy as np
import pytest
import torch

import mlp_ref as M
import pointwise_ref as P
import test_gpu_mlp_reference as G
from util import to_np

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.float16, np.float32, np.float64
GUARD = 4096
FILL = 7.0
WORST = P.WORST              # name -> worst ratio / share (read by whoever runs this module to record it)


def _abi():
    from focnerf_amd._lib import check, lib, ptr, stream_of
    return lib, ptr, stream_of, check


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out:
    """An output of `shape` and dtype in front of a guard band; everything starts as FILL."""

    def __init__(self, dtype, *shape):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), FILL, dtype=dtype, device="cuda")
        self.t = self.flat[:n].view(*shape)
        self.n = n

    def intact(self):
        return bool(torch.all(self.flat[self.n:] == FILL))

    def untouched(self):
        return bool(torch.all(self.flat == FILL))

    def np(self):
        return to_np(self.t)


def _bits(a):
    return np.ascontiguousarray(a).view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---------------------------------------------------------------- probes: device sinf and logf
def _sinf_arguments():
    rng = np.random.default_rng(123)
    parts = []
    for e in range(-20, 31):                                            # every binade [2^e, 2^(e+1)), e = -20 .. 30
        parts.append(np.ldexp(rng.uniform(1.0, 2.0, 9000), e))
    a = np.concatenate(parts).astype(F32)
    k = np.concatenate([np.arange(1, 20001), rng.integers(20001, int(2.0 ** 30 / (math.pi / 2)), 20000)]).astype(F64)
    near = (k * (math.pi / 2)).astype(F32)
    nb = [near]
    for _ in range(2):
        nb.append(np.nextafter(nb[-1], F32(np.inf)))
    lo = near
    for _ in range(2):
        lo = np.nextafter(lo, F32(-np.inf))
        nb.append(lo)
    a = np.concatenate([a] + nb)
    return np.concatenate([a, -a])


def test_probe_device_sinf():
    """sinf alone: foc_freq_encode_forward with deg = 1, D = 1 returns [x, sinf(x), sinf(fl32(x + fl32(pi/2)))]. ~2.3 M arguments, the
    worst error in ulp32 of the result per binade; K_SIN is the next integer at or above twice the worst."""
    lib, ptr, stream_of, check = _abi()
    x = _sinf_arguments()
    xt = _cuda(x[:, None])
    out = _Out(torch.float32, x.size, 3)
    check(lib.foc_freq_encode_forward(ptr(xt), x.size, 1, 1, 3, ptr(out.t), stream_of(xt)), "freq")
    torch.cuda.synchronize()
    assert out.intact()
    got = out.np()
    args = np.stack([x, (x + P.HALF_PI32).astype(F32)], 1).astype(F64)
    ref = np.sin(args)
    ulps = np.abs(got[:, 1:].astype(F64) - ref) / P.ulp32(ref)
    _, e = np.frexp(np.abs(args))
    lines = []
    for b in range(-21, 32):
        sel = e == b + 1
        if sel.any():
            lines.append(f"2^{b}: {ulps[sel].max():.3f} ({int(sel.sum())})")
    worst = float(ulps.max())
    print(f"\ndevice sinf: {args.size} arguments, worst {worst:.3f} ulp32 at {args.reshape(-1)[ulps.argmax()]!r}; worst per binade of |a| (count):\n  "
          + "  ".join(lines))
    big = np.abs(args) >= 2.0 ** 20
    print(f"  |a| >= 2^20: worst {ulps[big].max():.3f} ulp32; 2^29 <= |a|: worst {ulps[np.abs(args) >= 2.0 ** 29].max():.3f} ulp32")
    P.note("probe sinf ulp32", worst)
    assert math.ceil(2 * worst) <= P.K_SIN, f"device sinf is off by {worst:.3f} ulp32: K_SIN = {P.K_SIN} no longer holds"


def test_probe_device_logf_through_softplus():
    """logf is reachable only as softplus = logf(expf(10 x) + 1) / 10 of a half, rounded to half. Every finite half goes through (so
    logf sees every argument it can get, 1 .. 2^128 included); for each output, the least logf error in ulp32 of its result that explains
    the half the kernel wrote, after the other roundings' bound is taken off. K_LOG = max(1, next integer at or above twice the worst)."""
    c = P.sweep_case()
    _, fb = G._forward("train", _cuda(c["x"]), _cuda(c["W"]), 32, 64, 1, P.SOFTPLUS)
    got = to_np(fb)[0][:, :16]
    x = c["x"][:, :16].astype(F64)
    a, E0 = P.act_ref(P.SOFTPLUS, x, k_log=0)
    fin = np.isfinite(a)
    assert np.all(np.isinf(got[~fin])) and np.all(np.isfinite(got[fin]))
    g = got.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        up = (g + np.nextafter(got, F16(np.inf)).astype(F64)) / 2
        dn = (g + np.nextafter(got, F16(-np.inf)).astype(F64)) / 2
        need = np.maximum(np.maximum(dn - a, a - up), 0.0)                # distance of float64 to the interval that rounds to got
        L = a * P.K_ACT
        ulps = np.where(fin, np.maximum(need - E0, 0.0) * P.K_ACT / P.ulp32(L), 0.0)
    worst = float(ulps.max())
    same = float((got[fin] == P.to_half(a[fin])).mean())
    print(f"\ndevice logf through softplus: {int(fin.sum())} finite outputs, {same:.5f} of them the rounded float64 value; least logf error that "
          f"explains the rest {worst:.3f} ulp32")
    P.note("probe logf ulp32 (least that explains the halves)", worst)
    assert max(1, math.ceil(2 * worst)) <= P.K_LOG


# ---------------------------------------------------------------- part 1: the SH basis
@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_sh_encode_against_the_definition(n):
    lib, ptr, stream_of, check = _abi()
    d = P.directions(n, 10 + n % 97)
    dt = _cuda(d)
    out = _Out(torch.float32, n, 16)
    check(lib.foc_sh_encode(ptr(dt), n, ptr(out.t), stream_of(dt)), "sh_encode")
    torch.cuda.synchronize()
    assert out.intact()
    r = P.f32_check("sh_encode", out.np(), P.sh16(d.astype(F64)), P.sh16_bound(d))
    print(f"\nfoc_sh_encode n = {n}: worst error / bound {r:.3f}")


def _field(cols, nls, nlc, dirs, B, dir_div, dir_block, planar):
    lib, ptr, stream_of, check = _abi()
    ws, wc = P.selector_weights(cols, nls, nlc)
    enc = torch.zeros(B * 32, dtype=torch.float16, device="cuda")
    wst, wct, dt = _cuda(ws), _cuda(wc), _cuda(dirs)
    sigma, rgb = _Out(torch.float32, B), _Out(torch.float32, B, 3)
    check(lib.foc_nerf_field_inference(ptr(enc), planar, ptr(dt), dir_div, dir_block, dirs.shape[0], ptr(wst), nls, ptr(wct), nlc, 64, 6, B,
                                       ptr(sigma.t), ptr(rgb.t), None, stream_of(enc)), "nerf_field_inference")
    torch.cuda.synchronize()
    assert sigma.intact() and rgb.intact()
    return sigma, rgb


def _selector_check(name, rgb, dirs_of_rows, cols):
    rgb = np.asarray(rgb, F32)
    assert np.array_equal(P.to_half(rgb).astype(F32), rgb), f"{name}: rgb holds values that are not halves"
    d = dirs_of_rows
    s, Es = P.sh16(d.astype(F64))[:, list(cols)], P.sh16_bound(d)[:, list(cols)]
    return P.through_half(name, P.to_half(rgb), s, Es, P.sigmoid_ref)


@pytest.mark.parametrize("layout", ["per_sample", "blocked"])
@pytest.mark.parametrize("nls,nlc", [(2, 2), (1, 2)])
def test_nf_sh16_half_through_selector_weights(nls, nlc, layout):
    """Six calls route the sixteen SH columns, three at a time, to the logits. Blocked: 1000 rays (not a multiple of 64) x 3 depths."""
    if layout == "per_sample":
        B = 3001
        d = P.directions(B, 51)
        rows, args = np.arange(B), (1, 0, 0)
    else:
        N, T = 1000, 3
        d = P.directions(N, 52)
        rows = P.blocked_rows(N, T)
        B, args = rows.size, (T, 64, 1)
    worst = 0.0
    for cols in P.SELECTOR_TRIPLES:
        sigma, rgb = _field(cols, nls, nlc, d, B, *args)
        assert np.all(sigma.np() == 1.0), "the zero sigma network must give sigma = exp(0) = 1 exactly"
        worst = max(worst, _selector_check(f"nf_sh16_half ({layout})", rgb.np(), d[rows], cols))
    print(f"\nnf_sh16_half through foc_nerf_field_inference, layers ({nls}, {nlc}), {layout}: worst error / bound {worst:.3f}")


def test_nf_sh16_half_when_a_wave_s_run_of_tiles_crosses_blocks():
    """Blocked order with more tiles than the grid has waves (at most 8 workgroups of 4 waves per CU): every wave takes a run of at
    least two consecutive 64-row tiles, and with T = 3 depths per block the kept-in-register SH rows change block inside the run."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    T = 3
    nblk = -(-(2 * 8 * 4 * cus + 1) // T)
    N = nblk * 64 - 37
    rows = P.blocked_rows(N, T)
    B = rows.size
    assert B // 64 > 2 * 8 * 4 * cus
    d = P.directions(N, 53)
    cols = (9, 6, 15)
    sigma, rgb = _field(cols, 2, 2, d, B, T, 64, 1)
    rng = np.random.default_rng(5)
    edges = (rng.integers(1, nblk, 64) * 64 * T)[:, None] + np.arange(-64, 64)[None, :]
    pick = np.unique(np.concatenate([np.arange(512), np.arange(B - 512, B), edges.reshape(-1), rng.integers(0, B, 40000)]))
    st = _cuda(pick)
    assert bool(torch.all(sigma.t == 1.0))
    r = _selector_check("nf_sh16_half (blocked, runs of tiles)", to_np(rgb.t[st]), d[rows[pick]], cols)
    print(f"\nnf_sh16_half, blocked, B = {B} rows, {nblk} blocks of {T} tiles: worst error / bound {r:.3f} on {pick.size} rows")


# ---------------------------------------------------------------- part 2: csrc/head.hip
def _head_forward(c, width, with_obj, sigma=True, cin=True):
    lib, ptr, stream_of, check = _abi()
    n = c["n"]
    ht, dt = _cuda(c["h"]), _cuda(c["dirs"])
    ot = _cuda(c["obj"]) if with_obj else None
    s, ci = _Out(torch.float32, n), _Out(torch.float16, n, width)
    check(lib.foc_sample_head_forward(ptr(ht), ptr(dt), n, ptr(s.t) if sigma else None, ptr(ci.t) if cin else None, ptr(ot), width, stream_of(ht)), "head_forward")
    torch.cuda.synchronize()
    assert s.intact() and ci.intact()
    return s, ci


@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_head_forward(n):
    c = P.head_case(n, 20 + n % 97)
    d = c["dirs"]
    sh_ref, sh_bound = P.sh16(d.astype(F64)), P.sh16_bound(d)
    out, first = {}, None
    for width, with_obj in ((32, False), (48, False), (48, True)):
        s, ci = _head_forward(c, width, with_obj)
        cin = ci.np()
        if first is None:
            out["sigma"] = P.f32_check("head sigma", s.np(), *P.head_sigma(c["h"][:, 0]))
            out["cin SH"] = P.half_check("head cin SH columns", cin[:, :16], sh_ref, sh_bound)
            first = (s.np(), cin[:, :16].copy())
        else:
            assert np.array_equal(_bits(s.np()), _bits(first[0])) and np.array_equal(_bits(cin[:, :16]), _bits(first[1]))
        want = P.head_cin(c["h"], c["obj"] if with_obj else None, width)
        assert np.array_equal(_bits(cin[:, 16:]), _bits(want)), f"cin columns 16..{width - 1} (width {width}, obj {with_obj})"
        assert np.all(_bits(cin[:, -1]) == 0), "the pad column"
    # an absent output is not written
    s, ci = _head_forward(c, 32, False, cin=False)
    assert ci.untouched() and np.array_equal(_bits(s.np()), _bits(_head_forward(c, 32, False)[0].np()))
    s, ci = _head_forward(c, 48, True, sigma=False)
    assert s.untouched()
    print(f"\nfoc_sample_head_forward n = {n}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))


@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_head_backward(n):
    lib, ptr, stream_of, check = _abi()
    r = 0.0
    for width in (32, 48):
        c = P.head_case(n, 20 + n % 97, width)
        ht, gst, gct = _cuda(c["h"]), _cuda(c["grad_sigma"]), _cuda(c["grad_cin"])

        def run(gs, gc):
            gh = _Out(torch.float16, n, 16)
            check(lib.foc_sample_head_backward(ptr(ht), ptr(gs), ptr(gc), n, ptr(gh.t), width, stream_of(ht)), "head_backward")
            torch.cuda.synchronize()
            assert gh.intact()
            return gh.np()
        gh = run(gst, gct)
        r = max(r, P.half_check("head grad_h0", gh[:, 0], *P.head_grad_h0(c["h"][:, 0], c["grad_sigma"])))
        assert np.isnan(gh[np.isnan(c["h"][:, 0]), 0]).all()
        assert np.array_equal(_bits(gh[:, 1:]), _bits(c["grad_cin"][:, 16:31])), f"grad_h[:, 1:16] is not grad_cin[:, 16:31] (width {width})"
        g0 = run(None, gct)
        assert np.all(_bits(g0[:, 0]) == 0) and np.array_equal(_bits(g0[:, 1:]), _bits(gh[:, 1:]))
        g1 = run(gst, None)
        assert np.all(_bits(g1[:, 1:]) == 0) and np.array_equal(_bits(g1[:, 0]), _bits(gh[:, 0]))
    print(f"\nfoc_sample_head_backward n = {n}: grad_h0 worst error / bound {r:.3f}")


@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_rgb_head_forward_and_backward(n):
    lib, ptr, stream_of, check = _abi()
    c = P.head_case(n, 20 + n % 97)
    ct, gt = _cuda(c["c"]), _cuda(c["grad_rgb"])
    rgb, gc = _Out(torch.float32, n, 3), _Out(torch.float16, n, 16)
    check(lib.foc_rgb_head_forward(ptr(ct), n, ptr(rgb.t), stream_of(ct)), "rgb_forward")
    check(lib.foc_rgb_head_backward(ptr(ct), ptr(gt), n, ptr(gc.t), stream_of(ct)), "rgb_backward")
    torch.cuda.synchronize()
    assert rgb.intact() and gc.intact()
    y, g = rgb.np(), gc.np()
    r1 = P.rgb_check("rgb", y, c["c"][:, :3])
    r2 = P.half_check("rgb grad_c", g[:, :3], *P.rgb_grad(c["grad_rgb"], y))
    assert np.all(_bits(g[:, 3:]) == 0), "grad_c columns 3..15 must be +0"
    if n >= 255:
        k = [i for i, v in enumerate(P.LOGIT_SPECIAL) if v in (-17.0, -17.328125, -17.34375, -18.0)]
        rows = [i * len(P.GRGB_SPECIAL) for i in k]
        assert [float(y[r, r % 3]) for r in rows] == [2.0 ** -24, 2.0 ** -24, 0.0, 0.0]
    print(f"\nfoc_rgb_head n = {n}: rgb {r1:.3f}, grad_c {r2:.3f}")


# ---------------------------------------------------------------- part 3: the frequency encoder
def _freq(deg, D, B, seed):
    lib, ptr, stream_of, check = _abi()
    x = P.freq_inputs(B, D, seed)
    C = D + 2 * D * deg
    xt = _cuda(x)
    out = _Out(torch.float32, B, C)
    check(lib.foc_freq_encode_forward(ptr(xt), B, D, deg, C, ptr(out.t), stream_of(xt)), "freq_forward")
    g = np.random.default_rng(B + D).standard_normal((B, C)).astype(F32)
    gt = _cuda(g)
    gi = _Out(torch.float32, B, D)
    check(lib.foc_freq_encode_backward(ptr(gt), ptr(out.t), B, D, deg, C, ptr(gi.t), stream_of(xt)), "freq_backward")
    torch.cuda.synchronize()
    assert out.intact() and gi.intact()
    o = out.np()
    assert np.array_equal(_bits(o[:, :D]), _bits(x)), "identity columns"
    rf = P.f32_check("freq forward", o, *P.freq_forward(x, deg))
    rb = P.f32_check("freq backward", gi.np(), *P.freq_backward(g, o, D, deg))
    return rf, rb


@pytest.mark.parametrize("deg,D", P.FREQ_CASES)
def test_freq_encoder(deg, D):
    for B in P.FREQ_BATCHES:
        rf, rb = _freq(deg, D, B, 30 + deg + D + B % 89)
    print(f"\nfrequency encoder deg {deg} D {D}: forward {P.WORST['freq forward']:.3f} (of K_SIN = {P.K_SIN} ulp32), backward {P.WORST['freq backward']:.3f}")


def test_freq_encoder_second_pass_over_tiles():
    deg, D, B = P.FREQ_LOOP
    rf, rb = _freq(deg, D, B, 30 + deg + D + B % 89)
    print(f"\nfrequency encoder, {B} rows: forward {rf:.3f}, backward {rb:.3f}")


# ---------------------------------------------------------------- part 4: hidden activations 1..5
ROUTES = ("two_kernel", "two_kernel_det")


def _act_check(c, act, rname, worst, sweep=False):
    I, H, nl = c["I"], c["H"], c["nl"]
    what = f"{c['name']} {P.ACT_NAMES[act]} {rname}"
    assert M.routes_for(I, H, nl, act) == list(ROUTES) and M.kernels(rname, I, H, nl, act, True)[0] == "k_mlp_bwd"
    xt, Wt, gt = _cuda(c["x"]), _cuda(c["W"]), _cuda(c["grad"])
    Ws = M.split(c["W"], I, H, nl)
    out, fb = G._forward("train", xt, Wt, I, H, nl, act)
    for form in ("inference", "nofb"):
        o2 = G._forward(form, xt, Wt, I, H, nl, act)[0]
        assert torch.equal(o2.view(torch.int16), out.view(torch.int16)), f"{what}: the {form} forward differs from the training forward"
    fbn = to_np(fb)
    for l in range(nl):
        q = M.forward_layer(l, c["x"], fbn, Ws, M.NONE)
        r = P.act_forward_check(f"act {P.ACT_NAMES[act]} fb", fbn[l], q, act, max_loose=None if sweep else 0.01)
        worst["fb"] = max(worst["fb"], r)
    bb, gi, gw = G._backward(rname, True, gt, xt, Wt, fb, I, H, nl, act)
    bbn = to_np(bb)
    for k in range(nl):
        q = M.delta(k, c["grad"], fbn, bbn, Ws, M.NONE)
        P.act_delta_check(f"act {P.ACT_NAMES[act]} bb", bbn[k], q, fbn[nl - 1 - k], act)
    if sweep:
        return
    assert np.abs(fbn.astype(F32)).max() < M.HALF_MAX
    worst["out"] = max(worst["out"], M.worst_ratio(to_np(out), M.output(fbn, Ws), f"{what} out"))
    worst["grad_inputs"] = max(worst["grad_inputs"], M.worst_ratio(to_np(gi), M.grad_inputs(bbn, Ws), f"{what} grad_inputs"))
    q = M.grad_weights(c["x"], fbn, bbn, c["grad"], nl)
    worst["grad_weights"] = max(worst["grad_weights"], M.worst_ratio(to_np(gw), q, f"{what} grad_weights"))
    bb2, _, gw2 = G._backward(rname, False, gt, xt, Wt, fb, I, H, nl, act)
    assert torch.equal(bb2, bb)
    worst["grad_weights"] = max(worst["grad_weights"], M.worst_ratio(to_np(gw2), q, f"{what} grad_weights (no dx)"))


def _worst():
    return dict(fb=0.0, out=0.0, grad_inputs=0.0, grad_weights=0.0)


@pytest.mark.parametrize("rname", ROUTES)
@pytest.mark.parametrize("act", P.ACTS, ids=[P.ACT_NAMES[a] for a in P.ACTS])
@pytest.mark.parametrize("I,H,nl", P.ACT_SHAPES)
def test_activation_layers(I, H, nl, act, rname, lib_option):
    G._select(rname, I, H, nl, act, lib_option)
    worst = _worst()
    for B in P.ACT_BATCHES:
        _act_check(P.act_case(I, H, nl, B, 40 + B, act=act), act, rname, worst)
    for k, v in worst.items():
        P.note(f"act {P.ACT_NAMES[act]} {k}", v)
    print(f"\n{M.shape_name(I, H, nl)} {P.ACT_NAMES[act]} {rname}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("rname", ROUTES)
@pytest.mark.parametrize("act", P.ACTS, ids=[P.ACT_NAMES[a] for a in P.ACTS])
def test_activation_layers_over_gradient_scales(act, rname, lib_option):
    """Gradients of scale 2^-16 (deltas mostly subnormal halves) .. 2^8 at 32 x 64 x 2, B = 333."""
    G._select(rname, 32, 64, 2, act, lib_option)
    worst = _worst()
    for s in M.SCALES:
        _act_check(P.act_case(32, 64, 2, 333, 60 + s, scale=2.0 ** s, act=act), act, rname, worst)
    print(f"\nscales {P.ACT_NAMES[act]} {rname}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("act", P.ACTS, ids=[P.ACT_NAMES[a] for a in P.ACTS])
def test_every_half_through_the_activation(act, lib_option):
    """An identity layer hands every finite half to foc_act_forward and, with an identity output matrix, every gradient to
    foc_act_backward against that forward value: overflow to inf, subnormal results, NaN from nothing but inf * 0."""
    G._select("two_kernel", 32, 64, 1, act, lib_option)
    _act_check(P.sweep_case(), act, "two_kernel", _worst(), sweep=True)
    print(f"\nevery half through {P.ACT_NAMES[act]}: worst error / bound {P.WORST[f'act {P.ACT_NAMES[act]} fb']:.3f}")


def test_zz_report():
    """Prints what the module measured (the docstring's table is taken from here)."""
    print("\n" + "\n".join(f"    {k:70s} {v:.4f}" for k, v in sorted(P.WORST.items())))
