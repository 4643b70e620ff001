"""Float64 references of the POINTWISE kernels, a bound per element without a tuned constant, numpy fp32 models of the kernels and
deliberately wrong variants of those models (MUTANTS):

    csrc/sample_math.h foc_sh16, csrc/ffmlp.hip nf_sh16_half     the degree-4 real spherical harmonics           (`sh16`, `sh16_poly`)
    csrc/head.hip k_head_fwd / k_head_bwd                         trunc_exp, the colour-input row and its inverse (`head_*`)
    csrc/head.hip k_rgb_fwd / k_rgb_bwd                           the half sigmoid and its backward               (`rgb_*`)
    csrc/freqencoder.hip k_freq_fwd / k_freq_bwd                  sin(2^f x + b pi/2) and its backward            (`freq_*`)
    csrc/activations.h foc_act_forward / foc_act_backward         hidden activations 1..5 of the fused MLP        (`act_*`)

The SH basis comes from its definition, not from the nine constants of the kernels:

    Y_l^m(d) = N_l^|m| Q_l^|m|(z) * { sqrt(2) Re (x + iy)^m, 1, sqrt(2) Im (x + iy)^|m| } for m > 0, m = 0, m < 0, column l^2 + l + m,
    N_l^m = sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!),     Q_l^m(z) = P_l^m(z) / (1 - z^2)^(m/2),

Q by the associated-Legendre recurrence with the Condon-Shortley phase: Q_m^m = (-1)^m (2m - 1)!!, Q_(m+1)^m = (2m + 1) z Q_m^m,
(l - m) Q_l^m = (2l - 1) z Q_(l-1)^m - (l + m - 1) Q_(l-2)^m. On the unit sphere (x + iy)^m = (1 - z^2)^(m/2) e^(i m phi), which is the
textbook form (`sh16(d, angles=True)` evaluates that one, with atan2 and cos / sin(m phi)); written with (x + iy)^m it is the same
polynomial as the kernels' off the sphere too, where the kernels are also called (the directions of a ray are fp32 and not exactly unit).

The error model
---------------
U = 2^-24. Every fp32 + - * is correctly rounded, every constant is rounded to fp32 once, and / and sqrtf are correctly rounded too:
csrc/Makefile compiles with `-O3 -ffp-contract=off -fno-fast-math` and nothing else that touches arithmetic, so hipcc's default
-fhip-fp32-correctly-rounded-divide-sqrt holds (the flag to turn it off is -fno-hip-fp32-correctly-rounded-divide-sqrt; fp32 denormals
are on for gfx9 by default). An expression carries (n, mag): n roundings and the value of the expression with the absolute value of every
term. Inputs are exact (n = 0), a constant has n = 1, a sum has n = max(n_a, n_b) + 1 and mag_a + mag_b, a product n_a + n_b + 1 and
mag_a mag_b (relative errors of BOTH factors add: the "longest path" runs through both). The bound is gamma(n) mag with
gamma(n) = n U / (1 - n U). It holds with or without contraction to FMA, which only removes roundings. mag is not |result|: where a
difference cancels (squareplus of a large negative input, 0.946 z^2 - 0.315 near its zero) the kernel is held to the size of the terms.

Library functions: expf within 1 ulp, 2 U relative (the figure test_gpu_fixed_tail_reference.py rests on). ROCm ships no document with
a ULP figure for sinf or logf (no file under its tree mentions one), so they are MEASURED by the probe tests of
test_gpu_pointwise_reference.py and enter here as K_SIN and K_LOG ulp32 of the result:

    K_SIN = 4: worst 1.530 ulp32 (at a = -1957.4634) over 2 636 000 arguments: every binade 2^-20 .. 2^31, both signs, fl32(k pi/2) and its
               two neighbours on either side for k <= 20 000 and 20 000 random k up to 2^30; 1.528 over |a| >= 2^20, 1.475 over |a| >= 2^29
    K_LOG = 1: the only route to logf is the softplus layer, whose output is a half, so an error of a few ulp32 cannot be read off it.
               The probe hands that layer EVERY finite half (logf then sees every argument it can ever get there, 1 .. 2^128 included)
               and measures the least logf error that explains each output once the other roundings' bound is taken off: 99.948 % of
               the 50 288 finite outputs are the rounded float64 value and the rest are explained without logf, 0 ulp32 measured;
               K_LOG = max(1, 2 * 0), a function that is not correctly rounded being off by more than half an ulp.

Half outputs: bound E + 1/2 ulp_half(|ref| + E), subnormal halves unflushed; and wherever the float64 value is farther than E from every
midpoint between neighbouring halves (`half_check`'s "clear") the output must be exactly the rounded float64. The share of elements left
to the looser check is asserted <= 1 % (measured 0.0 - 0.9 %; one element where 1 % is less than one). Non-finite values must stand exactly where float64, rounded to the output
type with fp32 intermediates overflowing as fp32 does, puts them; within E of the overflow threshold either answer passes.

A value that passes through a half before a function (the pre-activation of an MLP layer, the SH value before the colour network's
sigmoid) is known as s +- E: that names one half, or two neighbours where s lies within E of a midpoint; the function's reference is
taken at that half or at both (`through_half`).
"""
import math

import numpy as np

import mlp_ref as M

U = 2.0 ** -24
K_SIN = 4
K_LOG = 1
FMAX = float(np.finfo(np.float32).max)
HALF_OVER = 65520.0
F32, F16, F64 = np.float32, np.float16, np.float64
WORST = {}                       # name -> worst |model or kernel - float64| / bound seen so far


def gamma(n):
    return n * U / (1.0 - n * U)


def ulp32(v):
    """Spacing of the fp32 numbers around magnitude v (2^-149 below 2^-126)."""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def note(name, r):
    WORST[name] = max(WORST.get(name, 0.0), float(r))
    return r


def expf(x):
    """The models' expf: the correctly rounded one (numpy's own float32 exp is off by more than an ulp)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.exp(np.asarray(x, F32).astype(F64)).astype(F32)


def to_half(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v).astype(F16)


# ---------------------------------------------------------------- checks
def _midpoint_distance(ref):
    """Distance of ref (float64, finite) to the nearest midpoint between neighbouring halves (65520 is the midpoint to inf)."""
    y = to_half(ref)
    yf = y.astype(F64)
    toward = np.where(ref > yf, F16(np.inf), F16(-np.inf))
    with np.errstate(over="ignore", invalid="ignore"):
        nb = np.nextafter(y, toward).astype(F64)
    nb = np.where(np.isinf(nb), np.sign(nb) * 65536.0, nb)
    yfin = np.where(np.isinf(yf), np.sign(yf) * 65536.0, yf)
    with np.errstate(invalid="ignore"):
        mid = np.where(np.isinf(yf), np.sign(yf) * HALF_OVER, (yfin + nb) / 2)
        return np.where(ref == yf, np.inf, np.abs(ref - mid))


def half_eval(got, ref, E):
    """Element by element, a half output against float64 ref with fp32 error E: `ok` (inside E + 1/2 ulp_half(|ref| + E), exact where
    clear of midpoints, non-finite values where float64 puts them), `ratio` |got - ref| / bound, `clear`, `finite` (of the reference)."""
    got = np.asarray(got).astype(F64)
    ref, E = np.broadcast_to(np.asarray(ref, F64), got.shape), np.broadcast_to(np.asarray(E, F64), got.shape)
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore", over="ignore"):
        must_inf = ~nan & (np.abs(ref) - E >= HALF_OVER)
        must_fin = ~nan & (np.abs(ref) + E < HALF_OVER)
        bound = E + 0.5 * M.ulp_half(np.where(nan | np.isinf(ref), 0.0, np.abs(ref)) + E)
        err = np.abs(got - ref)
        inside = err <= bound
        ratio = np.where(must_fin, err / bound, 0.0)
        rounded = to_half(ref).astype(F64)
        clear = must_fin & (_midpoint_distance(np.where(nan, 0.0, ref)) > E)
        same_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
    ok = np.where(nan, np.isnan(got), np.where(must_inf, same_inf, np.where(must_fin, inside & (~clear | (got == rounded)), inside | same_inf)))
    ratio = np.where(ok, ratio, np.inf)
    return dict(ok=ok, ratio=ratio, clear=clear, finite=must_fin, bound=bound, ref=ref)


def half_check(name, got, ref, E, max_loose=0.01):
    """Assert half_eval's `ok` everywhere and the share of finite elements left to the looser check <= max_loose (one element where that
    is less than one: a call with M = 1 has sixteen); records and returns the worst ratio."""
    r = half_eval(got, ref, E)
    bad = ~r["ok"]
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements outside; first at {np.argwhere(bad)[:4].tolist()}: got " \
                          f"{np.asarray(got)[bad][:4]}, float64 {np.broadcast_to(ref, bad.shape)[bad][:4]}"
    n = int(r["finite"].sum())
    loose = float((r["finite"] & ~r["clear"]).sum()) / max(n, 1)
    assert loose <= max(max_loose, 1.0 / max(n, 1)), f"{name}: {loose:.4f} of the elements lie within E of a half midpoint (allowed {max_loose})"
    note(name + " loose share", loose)
    return note(name, float(r["ratio"].max(initial=0.0)))


def f32_eval(got, ref, E):
    """An fp32 output: |got - ref| <= E, inf where |ref| - E is beyond fp32, NaN where ref is NaN."""
    got = np.asarray(got).astype(F64)
    ref, E = np.broadcast_to(np.asarray(ref, F64), got.shape), np.broadcast_to(np.asarray(E, F64), got.shape)
    nan = np.isnan(ref)
    with np.errstate(invalid="ignore", over="ignore"):
        must_inf = ~nan & (np.abs(ref) - E > 2.0 ** 128)
        must_fin = ~nan & (np.abs(ref) + E < FMAX)
        err = np.abs(got - ref)
        inside = np.where(E > 0, err <= E, got == ref)
        same_inf = np.isinf(got) & (np.sign(got) == np.sign(ref))
        ratio = np.where(must_fin & (E > 0), err / np.where(E > 0, E, 1.0), 0.0)
    ok = np.where(nan, np.isnan(got), np.where(must_inf, same_inf, np.where(must_fin, inside, inside | same_inf)))
    return dict(ok=ok, ratio=np.where(ok, ratio, np.inf))


def f32_check(name, got, ref, E):
    r = f32_eval(got, ref, E)
    bad = ~r["ok"]
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} elements outside; first at {np.argwhere(bad)[:4].tolist()}: got " \
                          f"{np.asarray(got)[bad][:4]}, float64 {np.broadcast_to(ref, bad.shape)[bad][:4]}, bound {np.broadcast_to(E, bad.shape)[bad][:4]}"
    return note(name, float(r["ratio"].max(initial=0.0)))


def adjacent_halves(lo, hi):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.nextafter(lo, F16(np.inf)).view(np.uint16) == hi.view(np.uint16)


def through_half(name, got, s, Es, fn, max_loose=0.01, strict=None):
    """got = half(fn(half(s'))) where s' is only known as s +- Es: the reference is fn at half(s - Es) .. half(s + Es). Where both
    ends are the same half (s clear of midpoints) that is half_eval on it, exactness included, and the share of those elements left to
    the looser check is held to max_loose (None: reported only; `strict(x)` restricts the share to the elements it selects). Where they
    are neighbours the output must pass at either; where a run of halves lies between them it may also lie between the two ends'
    values, widened by their bounds: fn must be monotonic over such a run (every function here is; the sine is wherever a run occurs,
    |s| < 0.04, which the caller asserts).
    fn(x) -> (float64 value, fp32 error)."""
    lo, hi = to_half(np.asarray(s, F64) - Es), to_half(np.asarray(s, F64) + Es)
    a, b = half_eval(got, *fn(lo.astype(F64))), half_eval(got, *fn(hi.astype(F64)))
    one = lo.view(np.uint16) == hi.view(np.uint16)
    g = np.asarray(got).astype(F64)
    with np.errstate(invalid="ignore"):
        wide = np.maximum(a["bound"], b["bound"])
        between = ~one & ~adjacent_halves(lo, hi) & a["finite"] & b["finite"] & (g >= np.minimum(a["ref"], b["ref"]) - wide) & (g <= np.maximum(a["ref"], b["ref"]) + wide)
    ok = a["ok"] | b["ok"] | between
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} elements outside; first at {np.argwhere(~ok)[:4].tolist()}: got " \
                     f"{np.asarray(got)[~ok][:4]}, pre-activation {np.asarray(s)[~ok][:4]}"
    fin = a["finite"] & one
    if strict is not None:
        fin = fin & strict(lo.astype(F64))
    loose = float((fin & ~a["clear"]).sum()) / max(int(fin.sum()), 1)
    assert max_loose is None or loose <= max(max_loose, 1.0 / max(int(fin.sum()), 1)), f"{name}: {loose:.4f} of the elements lie within E of a half midpoint (allowed {max_loose})"
    note(name + " loose share", loose)
    note(name + " share with more than one candidate", float((~one).mean()))
    return note(name, float(np.where(between, 0.0, np.minimum(a["ratio"], b["ratio"])).max(initial=0.0)))


# ---------------------------------------------------------------- spherical harmonics
SH_CONSTANTS = (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997, 0.31539156525251999, 0.54627421529603959,
                0.59004358992664352, 2.8906114426405538, 0.45704579946446572, 0.3731763325901154, 1.4453057213202769)
SH_MUTANTS = ("constant_2^-18", "columns_swapped", "sign_of_column_9")


def sh16(d, angles=False):
    """[N,3] -> [N,16] float64 from the definition (module docstring). angles=True: the textbook form in theta, phi (unit vectors only)."""
    d = np.asarray(d, F64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    out = np.empty((d.shape[0], 16))
    w = x + 1j * y
    if angles:
        phi, rho = np.arctan2(y, x), np.sqrt(np.maximum(1.0 - z * z, 0.0))
    for m in range(4):
        q = {m: np.full_like(z, (-1.0) ** m * float(np.prod(np.arange(2 * m - 1, 0, -2))))}        # (-1)^m (2m - 1)!!
        if m + 1 < 4:
            q[m + 1] = (2 * m + 1) * z * q[m]
        for l in range(m + 2, 4):
            q[l] = ((2 * l - 1) * z * q[l - 1] - (l + m - 1) * q[l - 2]) / (l - m)
        for l in range(m, 4):
            N = math.sqrt((2 * l + 1) / (4 * math.pi) * math.factorial(l - m) / math.factorial(l + m))
            if m == 0:
                out[:, l * l + l] = N * q[l]
                continue
            if angles:
                c, s = rho ** m * np.cos(m * phi), rho ** m * np.sin(m * phi)
            else:
                wm = w ** m
                c, s = wm.real, wm.imag
            out[:, l * l + l + m] = math.sqrt(2.0) * N * q[l] * c
            out[:, l * l + l - m] = math.sqrt(2.0) * N * q[l] * s
    return out


def sh16_poly(d, dtype=F64, mutant=None):
    """The polynomial form with the constants, the kernels' order of operations; dtype=float32 is the numpy model of foc_sh16 (every
    constant rounded to fp32 once, every operation rounded)."""
    t = np.dtype(dtype).type
    d = np.asarray(d).astype(dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    k = [t(v) for v in SH_CONSTANTS]
    if mutant == "constant_2^-18":
        k[2] = t(SH_CONSTANTS[2] * (1 + 2.0 ** -18))
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    c = [np.full_like(x, k[0]), -k[1] * y, k[1] * z, -k[1] * x, k[2] * xy, -k[2] * yz, k[3] * z2 - k[4], -k[2] * xz, k[5] * x2 - k[5] * y2,
         k[6] * y * (t(-3.0) * x2 + y2), k[7] * xy * z, k[8] * y * (t(1.0) - t(5.0) * z2), k[9] * z * (t(5.0) * z2 - t(3.0)),
         k[8] * x * (t(1.0) - t(5.0) * z2), k[10] * z * (x2 - y2), k[6] * x * (-x2 + t(3.0) * y2)]
    if mutant == "columns_swapped":
        c[11], c[13] = c[13], c[11]
    if mutant == "sign_of_column_9":
        c[9] = -c[9]
    return np.stack(c, axis=1)


# roundings per column (module docstring): constant 1; c * v 2; c * (uv) 3; c u^2 - c' 4; c * y * (a x^2 + y^2): (c y) 2 + paren 3 + 1 = 6
SH_ROUNDINGS = (1, 2, 2, 2, 3, 3, 4, 3, 4, 6, 4, 6, 6, 6, 5, 6)


def sh16_mag(d):
    d = np.abs(np.asarray(d, F64))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    k = SH_CONSTANTS
    return np.stack([np.full_like(x, k[0]), k[1] * y, k[1] * z, k[1] * x, k[2] * x * y, k[2] * y * z, k[3] * z * z + k[4], k[2] * x * z,
                     k[5] * (x * x + y * y), k[6] * y * (3 * x * x + y * y), k[7] * x * y * z, k[8] * y * (1 + 5 * z * z), k[9] * z * (5 * z * z + 3),
                     k[8] * x * (1 + 5 * z * z), k[10] * z * (x * x + y * y), k[6] * x * (x * x + 3 * y * y)], axis=1)


def sh16_bound(d):
    """Per-column bound of an fp32 evaluation of the polynomial form on fp32 directions."""
    return np.array([gamma(n) for n in SH_ROUNDINGS])[None, :] * sh16_mag(d)


def directions(n, seed):
    """fp32 directions: unit vectors (normalised in float64, then rounded), and among them vectors off the sphere (|d| up to 4), the
    zero vector and the six axes where n allows."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    if n >= 64:
        off = rng.choice(n, n // 8, replace=False)
        d[off] *= rng.uniform(0.0, 4.0, (off.size, 1))
        d[1:7] = np.concatenate([np.eye(3), -np.eye(3)])
        d[7] = 0.0
    return d.astype(F32)


# ---------------------------------------------------------------- csrc/head.hip
H0_SPECIAL = (14.5, -14.5, 15.0, -15.0, 15.0078125, -15.0078125, 65504.0, -65504.0, np.inf, -np.inf, np.nan, 0.0, -0.0, 2.0 ** -24, -3 * 2.0 ** -24)
GS_SPECIAL = (0.0, 1e-30, 1e30, 1.0, -0.37)
LOGIT_SPECIAL = (7.0, -7.0, 12.0, -12.0, 17.0, -17.0, -17.328125, -17.34375, -18.0, -25.0, 65504.0, -65504.0, 0.0)
GRGB_SPECIAL = (1e5, -7e4, 65519.0, 65520.0, 2.0 ** -26, 2.0 ** -24, 1.0, 0.0)
HEAD_SIZES = (1, 255, 256, 257, 2048 * 256 + 1)          # 2048 * 256 + 1: foc_grid_1d caps the grid at 2048 workgroups, one thread strides


def head_case(n, seed, width=32):
    """Inputs of one call of every head kernel: h [n,16] half (h0 ~ N(0, 2) with the specials of the docstring crossed with the
    grad_sigma specials in the first rows), dirs, obj [16], grad_sigma [n], grad_cin [n,width], colour logits c [n,16], grad_rgb [n,3]."""
    rng = np.random.default_rng(seed)
    h = rng.normal(0, 2, (n, 16)).astype(F16)
    gs = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F32)
    c = rng.normal(0, 2, (n, 16)).astype(F16)
    grgb = rng.standard_normal((n, 3)).astype(F32)
    if n >= 255:
        k = 0
        for a in H0_SPECIAL:
            for b in GS_SPECIAL:
                h[k, 0], gs[k] = F16(a), F32(b)
                k += 1
        k = 0
        for a in LOGIT_SPECIAL:
            for b in GRGB_SPECIAL:
                c[k, k % 3], grgb[k, k % 3] = F16(a), F32(b)
                k += 1
        h[200:216, 1:] = (rng.standard_normal((16, 15)) * 2.0 ** -20).astype(F16)            # subnormal geometry features
    gcin = rng.standard_normal((n, width)).astype(F16)
    if n >= 255:
        gcin[200:216] = (rng.standard_normal((16, width)) * 2.0 ** -20).astype(F16)
    obj = rng.standard_normal(16).astype(F16)
    return dict(n=n, h=h, dirs=directions(n, seed + 1), obj=obj, grad_sigma=gs, grad_cin=gcin, c=c, grad_rgb=grgb, width=width)


def head_sigma(h0):
    """sigma = expf(h0): (ref, E) with E = 2 U ref, at least one fp32 subnormal step."""
    with np.errstate(over="ignore"):
        ref = np.exp(np.asarray(h0).astype(F64))
    with np.errstate(invalid="ignore"):
        return ref, np.maximum(2 * U * np.where(np.isfinite(ref), ref, 0.0), 2.0 ** -149)


def head_cin(h, obj, width):
    """What must stand right of the SH columns, bit for bit: [h[:, 1:16] | obj[0] or 0 | width 48: obj[1:16] or 0, 0]."""
    n = h.shape[0]
    out = np.zeros((n, width - 16), F16)
    out[:, :15] = h[:, 1:16]
    if obj is not None:
        out[:, 15] = obj[0]
        out[:, 16:31] = obj[1:16]
    return out


def head_grad_h0(h0, gs, mutant=None):
    """g * exp(clamp(h0, -15, 15)) in float64 and its fp32 error: expf 2 U, the product U."""
    x = np.asarray(h0).astype(F64)
    lim = 14.5 if mutant == "clamp_14.5" else 15.0
    with np.errstate(invalid="ignore", over="ignore"):
        xc = x if mutant == "exp_unclamped" else np.where(x < -lim, -lim, np.where(x > lim, lim, x))
        ref = np.asarray(gs).astype(F64) * np.exp(xc)
        return ref, gamma(3) * np.where(np.isfinite(ref), np.abs(ref), 0.0) + 2.0 ** -149


def model_head_grad_h0(h0, gs, mutant=None):
    """numpy fp32 model of k_head_bwd's column 0."""
    x = np.asarray(h0).astype(F32)
    lim = F32(14.5 if mutant == "clamp_14.5" else 15.0)
    with np.errstate(invalid="ignore", over="ignore"):
        xc = x if mutant == "exp_unclamped" else np.where(x < -lim, -lim, np.where(x > lim, lim, x))
        return to_half(np.asarray(gs, F32) * expf(xc))


def sigmoid_ref(x):
    """1 / (1 + expf(-x)) in fp32: (float64 value, E). expf 2 U on e, the sum and the quotient U each: E = U s (2 e / (1 + e) + 2), and
    2^-126 for the fp32 underflow of the quotient (expf(-x) overflows to inf beyond x = -88.7, the quotient is then 0)."""
    x = np.asarray(x).astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-x)
        s = 1.0 / (1.0 + e)
        share = np.where(np.isinf(e), 1.0, e / (1.0 + e))
        return s, U * s * (2 * share + 2) / (1 - 4 * U) + 2.0 ** -126


def model_sigmoid_h(x, mutant=None):
    """numpy fp32 model of foc_sigmoid_h: the half-rounded sigmoid held in fp32."""
    x = np.asarray(x).astype(F32)
    with np.errstate(over="ignore"):
        s = (F32(1.0) / (F32(1.0) + expf(-x))).astype(F32)
    return s if mutant == "sigmoid_not_rounded" else to_half(s).astype(F32)


def rgb_check(name, rgb, c):
    """k_rgb_fwd: fp32 values that are halves, the half within the sigmoid's bound."""
    rgb = np.asarray(rgb, F32)
    assert np.array_equal(to_half(rgb).astype(F32), rgb), f"{name}: rgb holds values that are not halves"
    return half_check(name, to_half(rgb), *sigmoid_ref(c))


def rgb_grad(grgb, y, mutant=None):
    """half(g) (1 - y) y in float64 on the kernel's own y, and its fp32 error (three roundings; mag |g| (1 + y) y)."""
    g = np.asarray(grgb, F32)
    g = g.astype(F64) if mutant == "grad_rgb_not_rounded" else to_half(g).astype(F64)
    y = np.asarray(y).astype(F64)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = g * (1.0 - y) * y
        mag = np.abs(g) * (1.0 + y) * y
        return ref, gamma(3) * np.where(np.isfinite(mag), mag, 0.0) + 2.0 ** -149


def model_rgb_grad(grgb, y, mutant=None):
    g = np.asarray(grgb, F32)
    g = g if mutant == "grad_rgb_not_rounded" else to_half(g).astype(F32)
    y = np.asarray(y, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return to_half(g * (F32(1.0) - y) * y)


HEAD_MUTANTS = ("clamp_14.5", "exp_unclamped", "sigmoid_not_rounded", "grad_rgb_not_rounded")


# ---------------------------------------------------------------- csrc/freqencoder.hip
HALF_PI32 = F32(F32(3.141592653589793) / F32(2))
FREQ_CASES = ((4, 3), (10, 3), (30, 5), (1, 100), (1, 3000))          # (deg, D): 256, 256, 256, 81 and 2 rows per tile
FREQ_BATCHES = (1, 257, 1000)
FREQ_LOOP = (4, 3, 256 * 2048 + 3)                                      # the grid is capped at 2048 workgroups: a second pass over tiles
FREQ_MUTANTS = ("pi_half_after_the_sum", "no_2^f_in_backward")


def freq_inputs(B, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-4.0, 4.0, (B, D)).astype(F32)
    if B * D >= 16:
        x.reshape(-1)[:8] = np.array([0.0, -0.0, 4.0, -4.0, 2.0 ** -20, 1.5707964, 3.1415927, -3.1415927], F32)
    return x


def freq_args(x, deg, mutant=None):
    """The fp32 arguments of sinf, [B, 2 deg, D]: scalbnf is exact, the cosine columns add fl32(pi/2) with one rounding."""
    x = np.asarray(x, F32)
    out = np.empty((x.shape[0], 2 * deg, x.shape[1]), F32)
    for f in range(deg):
        a = np.ldexp(x, f).astype(F32)
        out[:, 2 * f] = a
        out[:, 2 * f + 1] = (a.astype(F64) + math.pi / 2).astype(F32) if mutant == "pi_half_after_the_sum" else a + HALF_PI32
    return out


def freq_forward(x, deg, k_sin=None):
    """(ref [B, C] float64, bound): identity columns exact, the rest sin in float64 of the exact fp32 argument, K_SIN ulp32 of the result."""
    k_sin = K_SIN if k_sin is None else k_sin
    x = np.asarray(x, F32)
    B, D = x.shape
    s = np.sin(freq_args(x, deg).astype(F64)).reshape(B, 2 * deg * D)
    return np.concatenate([x.astype(F64), s], 1), np.concatenate([np.zeros((B, D)), k_sin * ulp32(s)], 1)


def model_freq_forward(x, deg, mutant=None):
    """numpy model: a correctly rounded sinf of the fp32 argument."""
    x = np.asarray(x, F32)
    B, D = x.shape
    return np.concatenate([x, np.sin(freq_args(x, deg, mutant).astype(F64)).astype(F32).reshape(B, 2 * deg * D)], 1)


def freq_backward(g, out, D, deg):
    """g_d + sum_f 2^f (g_sin o_cos - g_cos o_sin) in float64 on the outputs the kernel was given; bound C U (2 deg + 1) sum|t|."""
    B = g.shape[0]
    g3 = np.asarray(g).astype(F64)[:, D:].reshape(B, deg, 2, D)
    o3 = np.asarray(out).astype(F64)[:, D:].reshape(B, deg, 2, D)
    w = np.ldexp(1.0, np.arange(deg))[None, :, None]
    a, b = w * g3[:, :, 0] * o3[:, :, 1], w * g3[:, :, 1] * o3[:, :, 0]
    g0 = np.asarray(g).astype(F64)[:, :D]
    return g0 + (a - b).sum(1), M.C * U * (2 * deg + 1) * (np.abs(g0) + (np.abs(a) + np.abs(b)).sum(1))


def model_freq_backward(g, out, D, deg, mutant=None):
    """numpy fp32 model of k_freq_bwd: fmaf(2^f, fmaf(g_sin, o_cos, -(g_cos * o_sin)), result), a fused multiply-add as one rounding of
    the float64 value (the product of two fp32 numbers is exact there)."""
    g, out = np.asarray(g, F32), np.asarray(out, F32)
    res = g[:, :D].copy()
    for f in range(deg):
        gs, gc = g[:, D * (1 + 2 * f):D * (2 + 2 * f)], g[:, D * (2 + 2 * f):D * (3 + 2 * f)]
        os_, oc = out[:, D * (1 + 2 * f):D * (2 + 2 * f)], out[:, D * (2 + 2 * f):D * (3 + 2 * f)]
        inner = (gs.astype(F64) * oc.astype(F64) - (gc * os_).astype(F64)).astype(F32)
        w = 1.0 if mutant == "no_2^f_in_backward" else 2.0 ** f
        res = (w * inner.astype(F64) + res.astype(F64)).astype(F32)
    return res


# ---------------------------------------------------------------- csrc/activations.h
EXP, SINE, SIGMOID, SQUAREPLUS, SOFTPLUS = 1, 2, 3, 4, 5
ACTS = (EXP, SINE, SIGMOID, SQUAREPLUS, SOFTPLUS)
ACT_NAMES = {1: "exponential", 2: "sine", 3: "sigmoid", 4: "squareplus", 5: "softplus"}
ACT_SHAPES = ((32, 64, 2), (48, 32, 3))
ACT_BATCHES = (1, 33, 129, 333)
ACT_MUTANTS = ("squareplus_factor_in_half", "sigmoid_factor_in_fp32")
K_ACT = 10.0


def act_ref(act, x, k_sin=None, k_log=None):
    """foc_act_forward before its rounding to half, for a half x: (float64 value, fp32 error E). fp32 intermediates overflow as fp32 does.
    x * 10 is exact in fp32 (an 11-bit times a 4-bit significand)."""
    k_sin, k_log = K_SIN if k_sin is None else k_sin, K_LOG if k_log is None else k_log
    x = np.asarray(x).astype(F64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if act == EXP:
            a = np.exp(x)
            a = np.where(a > FMAX, np.inf, a)
            return a, np.maximum(2 * U * np.where(np.isfinite(a), a, 0.0), 2.0 ** -149)
        if act == SINE:
            a = np.sin(x)
            return a, k_sin * ulp32(a)
        if act == SIGMOID:
            return sigmoid_ref(x)
        if act == SQUAREPLUS:
            s = x * K_ACT                                        # exact
            v = s * s + 4.0
            e_v = U * s * s + U * v                              # the square, the sum
            r = np.sqrt(v)
            e_r = e_v / (2 * r) + U * r
            t = s + r
            e_t = e_r + U * (np.abs(t) + e_r)                   # the sum's own rounding is relative to the sum: the cancellation is in e_r
            a = 0.5 * t / K_ACT
            return a, (e_t * 0.5 / K_ACT + U * (np.abs(a) + e_t * 0.5 / K_ACT)) / (1 - 8 * U)
        if act == SOFTPLUS:
            p = x * K_ACT                                        # exact
            e = np.exp(p)
            over = e > FMAX
            e = np.where(over, 0.0, e)
            e_e = 2 * U * e + 2.0 ** -149
            w = 1.0 + e
            e_w = e_e + U * w
            L = np.log1p(e)
            e_L = e_w / w + k_log * ulp32(L)
            a = L / K_ACT
            E = (e_L / K_ACT + U * (np.abs(a) + e_L / K_ACT)) / (1 - 8 * U)
            return np.where(over, np.inf, a), np.where(over, 0.0, E)
    raise KeyError(act)


def model_act_forward(act, x):
    """numpy fp32 model of foc_act_forward on halves (expf, sinf and logf correctly rounded)."""
    h = np.asarray(x, F16)
    x = h.astype(F32)
    ten = F32(K_ACT)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if act == EXP:
            return to_half(expf(x))
        if act == SINE:
            return to_half(np.sin(x.astype(F64)).astype(F32))
        if act == SIGMOID:
            return to_half(F32(1.0) / (F32(1.0) + expf(-x)))
        if act == SQUAREPLUS:
            s = x * ten
            return to_half(F32(0.5) * (s + np.sqrt(s * s + F32(4.0))) / ten)
        if act == SOFTPLUS:
            return to_half(np.log((expf(x * ten) + F32(1.0)).astype(F64)).astype(F32) / ten)
    raise KeyError(act)


def _hmul(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return to_half(np.asarray(a, F16).astype(F32) * np.asarray(b, F16).astype(F32))


def act_backward_candidates(act, g, fwd, mutant=None):
    """foc_act_backward(g, fwd) on halves, bit for bit in numpy fp16 / fp32: a list of one array — or of two for softplus where the
    bounded expf leaves the factor's half undecided (1 - expf(-10 f) within 2 U e + U of float64, then rounded to half)."""
    g, fwd = np.asarray(g, F16), np.asarray(fwd, F16)
    f = fwd.astype(F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if act == EXP:
            return [_hmul(g, fwd)]
        if act == SINE:
            return [g.copy()]                                    # the reference's pass-through, asserted as it stands
        if act == SIGMOID:
            if mutant == "sigmoid_factor_in_fp32":
                return [_hmul(g, to_half(f * (F32(1.0) - f)))]
            return [_hmul(g, _hmul(fwd, to_half(F32(1.0) - f)))]
        if act == SQUAREPLUS:
            if mutant == "squareplus_factor_in_half":
                y = _hmul(fwd, F16(K_ACT))
                yy = _hmul(y, y)
                return [_hmul(g, to_half(yy.astype(F32) / to_half(yy.astype(F32) + F32(1.0)).astype(F32)))]
            y = f * F32(K_ACT)
            return [_hmul(g, to_half(y * y / (y * y + F32(1.0))))]
        if act == SOFTPLUS:
            e = np.exp(-fwd.astype(F64) * K_ACT)
            ref = 1.0 - e
            E = (2 * U * e + 2.0 ** -149 + U * np.abs(ref)) / (1 - 4 * U)
            return [_hmul(g, to_half(ref - E)), _hmul(g, to_half(ref + E))]
    raise KeyError(act)


def act_forward_check(name, got, q, act, max_loose=0.01):
    """fb[l] against the activation of the half (or the halves) the float64 sum q names. The share left to the looser check is held to
    max_loose; for softplus and squareplus on x >= 0 only. Below, logf(expf(10 x) + 1) loses expf(10 x) against 1 and s + sqrt(s^2 + 4)
    cancels: E is U / e^(10 x), respectively 2 U (s^2 + 4) / 4, of the result, no longer small against the spacing of the halves, and
    the share within E of a midpoint grows with -x (the kernel reproduces the reference's fp32 formulas and is right to do so). Those
    elements keep the bound E + 1/2 ulp; they are reported, not counted."""
    Es = np.where(q["count"] > 1, M.C * U * (q["count"] - 1) * q["mag"], 0.0)
    if act == SINE:
        lo, hi = to_half(q["ref"] - Es), to_half(q["ref"] + Es)
        differ = (lo.view(np.uint16) != hi.view(np.uint16)) & ~adjacent_halves(lo, hi)
        assert np.all(np.abs(hi[differ].astype(F64)) < 1.5) and np.all(np.abs(lo[differ].astype(F64)) < 1.5)
    return through_half(name, got, q["ref"], Es, lambda x: act_ref(act, x), max_loose, (lambda x: x >= 0) if act in (SOFTPLUS, SQUAREPLUS) else None)


def act_delta_check(name, got, q, fwd, act, mutant=None):
    """bb[k] = foc_act_backward(half(sum), fb), which numpy reproduces bit for bit given the half: where the float64 sum names one half
    the delta is that value exactly (one of two for softplus, whose factor rests on the bounded expf); where it names a run of halves
    the delta lies between the values at the run's ends (the function is monotonic in the gradient). Returns the share of the latter."""
    got = np.asarray(got, F16)
    Es = np.where(q["count"] > 1, M.C * U * (q["count"] - 1) * q["mag"], 0.0)
    cands = []
    for g in (to_half(q["ref"] - Es), to_half(q["ref"] + Es)):
        cands += [c.astype(F64) for c in act_backward_candidates(act, g, fwd, mutant)]
    gv = got.astype(F64)
    exact = np.zeros(got.shape, bool)
    for c in cands:
        exact |= (gv == c) | (np.isnan(gv) & np.isnan(c))
    with np.errstate(invalid="ignore"):
        lo, hi = np.minimum.reduce(cands), np.maximum.reduce(cands)
        ok = exact | ((gv >= lo) & (gv <= hi))
    assert ok.all(), f"{name}: {int((~ok).sum())} of {ok.size} deltas are none of the candidates; first at {np.argwhere(~ok)[:4].tolist()}: got " \
                     f"{got[~ok][:4]}, candidates {[c[~ok][:4] for c in cands]}"
    return note(name + " share with more than one candidate", float((lo != hi).mean()))


def act_case(I, H, nl, B, seed, scale=0.05, act=None):
    """A case of mlp_ref.make_case's layout for the activations: weights sqrt(3 / H) * U(-1, 1), x ~ N(0, 1), grad ~ N(0, scale). For
    the exponential the weights are a third of that: two or three exponentials in a row leave the halves at unit weights, and a layer
    with an inf among its inputs is NaN wherever a weight is 0 times it (the overflow itself is the sweep's business)."""
    c = M.make_case(f"act_{M.shape_name(I, H, nl)}_B{B}_s{scale:g}", I, H, nl, B, scale, seed)
    if act == EXP:
        c["W"] = (c["W"].astype(F32) / F32(3)).astype(F16)
    return c


def all_halves():
    """Every finite half, [3968, 16]."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(F16)
    return h[np.isfinite(h)].reshape(-1, 16)


def sweep_case(seed=7):
    """A 32 -> 64 -> 16 network with one hidden layer that hands every finite half to the activation and every gradient to its
    backward unchanged: W0 the identity on neurons 0..15 (x columns 16..31 are 0: an inf-free row), W_out the identity on them."""
    I, H, nl = 32, 64, 1
    h = all_halves()
    x = np.zeros((h.shape[0], I), F16)
    x[:, :16] = h
    W = np.zeros(M.n_params(I, H, nl), F16)
    o_out = M.offsets(I, H, nl)[-1][0]
    for n in range(16):
        W[n * I + n] = 1.0
        W[o_out + n * H + n] = 1.0
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((h.shape[0], 16)) * 10.0 ** rng.uniform(-6, 2, (h.shape[0], 16))).astype(F16)
    return dict(name="sweep", I=I, H=H, nl=nl, B=h.shape[0], x=x, W=W, grad=g)


# ---------------------------------------------------------------- selector weights for foc_nerf_field_inference
SELECTOR_TRIPLES = ((0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 0, 8))


def selector_weights(cols, nls, nlc):
    """(sigma blob of zeros, colour blob) for 32 -> 64 networks: the colour network routes SH columns `cols` to its logits 0..2
    unchanged (W0 rows 0..2 unit vectors, hidden matrices the identity on those neurons, W_out rows 0..2 likewise; activation None)."""
    ws = np.zeros(M.n_params(32, 64, nls), F16)
    wc = np.zeros(M.n_params(32, 64, nlc), F16)
    offs = M.offsets(32, 64, nlc)
    for j, k in enumerate(cols):
        wc[offs[0][0] + j * 32 + k] = 1.0
        for o, _, c in offs[1:]:
            wc[o + j * c + j] = 1.0
    return ws, wc


def blocked_rows(N, T):
    """Row -> ray of the block-interleaved order (csrc/fixedstep.hip fs_block_row): 64 rays x T depths per block, the ray fastest."""
    nblk = -(-N // 64)
    r = np.arange(nblk * 64 * T)
    return np.minimum((r // (64 * T)) * 64 + r % 64, N - 1)
