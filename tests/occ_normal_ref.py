"""Float64 statement of what the occupancy march makes of a ray's normals (csrc/occrender.hip foc_occ_render_step_normals, raymarching.hip
k_composite_rays / k_composite_rays_pre with the second payload, normals.hip foc_normal_map_finish), and the per-element bound its fp32
evaluation is held to.

(a) `composite()` — two payloads over a ray's sample list. Per ray, samples j = 0, 1, ... in march order, from zero accumulators:

        stop (nothing accumulated) if dt0_j == 0                                   the slot holds no sample
        alpha = 1 - exp(-sigma_j dt0_j);  T = 1 - W;  w = alpha T
        W += w;  t += dt1_j;  depth += w t;  A += w a_j;  B += w b_j               a: first payload (the colour), b: second (the encoded normal)
        stop (after the accumulation) if T < T_thresh                              the transmittance BEFORE the sample, as composite_rays tests it

    One set of weights, one stop: both payloads see the same w_j and end at the same sample. Arrays are [n, S(, 3)], a ray shorter than S is
    padded with dt0 = 0. `n_acc` (how many samples a ray accumulates) is an argument: the test T < T_thresh is a discontinuous decision fp32
    may take one sample earlier or later when T lies within rounding of the threshold. `stop_range()` gives per ray the decisions float64
    cannot exclude; a caller compares ALL of a ray's outputs at one of them (`best_ratio()`).

(b) `finish()` — s = 2 acc - W per component; m = max |s_d|; m == 0 or not finite -> normal = 0, else u = s / m, normal = u / sqrt(u.u)
    (unit_normal.h); normal_rgb = acc + (1 - W), the encoded map on a white background.

THE BOUND, counted from the kernels' fp32 rounding points (U = 2^-24, half an ulp of 1; C, K and the magnitude rules are ragged_ref.py's,
whose inference burst is the same recurrence with one payload):
  composite   `magnitudes()`: first-order magnitudes of W, depth, A, B after each number of samples. alpha uses __expf: a = -sigma dt0 is
              rounded, a log2(e) rounded again before the hardware exp2: exp(a) carries exp(a) (2 |a| + 1). W feeds its own next term
              through T = 1 - W: W' = W + alpha (1 - W) carries mag(W) (1 - alpha). Each accumulator: the magnitudes of its terms plus
              the absolute values of the terms once. bound = C U (T + K) mag + (T + K) 2^-126, T = the number of samples accumulated.
  s           fl(2 acc - W): 2 acc exact, one rounding:  b_s = 2 b_acc + b_W + U |s|
  normal      direction: for vectors, | a/|a| - b/|b| | <= 2 |a - b| / (|a| + |b|) (inner-product spaces; no first-order assumption), so with
              d = |b_s|_2 the computed s' has |s'| >= |s| - d and the direction moves by at most 2 d / (2 |s| - d). Where d >= |s| the
              direction is not defined at this resolution: `finish_bounds()` marks the pixel `unresolved`, it is the pixel a test may skip.
              the normalisation itself: u = s/m (1 rounding), u.u by fmaf from u0 u0 (2 U from the operands + 3 roundings on positive terms),
              sqrt (half of that + 1), the division (u's + len's + 1): 1 + (5/2 + 1) + 1 = 5.5 -> 6 U per component (|n_d| <= 1)
              b_normal = 2 d / (2 |s| - d) + 6 U
  normal_rgb  fl(acc + fl(1 - W)): b_acc + b_W + U |1 - W| + U |normal_rgb|

`mutant=` names a deliberately wrong variant (MUTANTS); test_occ_normal_ref.py shows that the bound rejects each. No reference value is ever
computed with one."""
import numpy as np
import torch

from ragged_ref import C, K, TINY, U, fast_exp

MUTANTS = ("late_weights", "stop_one_payload", "wrong_W")


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a, np.float64)).to(dtype)


def history(sigma, dt0, dt1, a, b, dtype=torch.float64, mutant=None):
    """The recurrence without its stops: W, depth [n,S+1], A, B [n,S+1,3] after each number of samples, T [n,S] the transmittance each sample's
    test sees (numpy, float64 values)."""
    sg, d0, d1, pa, pb = _t(sigma, dtype), _t(dt0, dtype), _t(dt1, dtype), _t(a, dtype), _t(b, dtype)
    n, S = sg.shape
    zero = torch.zeros(n, dtype=dtype)
    W, t, dp, A, B = zero, zero, zero, torch.zeros(n, 3, dtype=dtype), torch.zeros(n, 3, dtype=dtype)
    hist = dict(W=[W], depth=[dp], A=[A], B=[B], T=[])
    w_prev = zero
    for j in range(S):
        alpha = 1 - fast_exp(-sg[:, j] * d0[:, j])
        T = 1 - W
        w = alpha * T
        W = W + w
        t = t + d1[:, j]
        dp = dp + w * t
        A = A + w[:, None] * pa[:, j]
        B = B + (w_prev if mutant == "late_weights" else w)[:, None] * pb[:, j]
        w_prev = w
        hist["T"].append(T)
        for k, v in (("W", W), ("depth", dp), ("A", A), ("B", B)):
            hist[k].append(v)
    return {k: (torch.stack(v, 1).to(torch.float64).numpy() if v else np.zeros((n, 0))) for k, v in hist.items()}


def composite(sigma, dt0, dt1, a, b, T_thresh, n_acc=None, dtype=torch.float64, mutant=None, hist=None):
    """(a) of the module docstring. sigma, dt0, dt1 [n,S]; a, b [n,S,3]. n_acc [n] or None (this evaluation's own decisions); hist: a
    `history()` of the same arguments, to pick several decisions from one evaluation.
    -> dict: W [n], depth [n], A [n,3], B [n,3] (numpy float64 values), n_acc [n], T [n,S] the transmittance each sample's test sees."""
    hist = history(sigma, dt0, dt1, a, b, dtype, mutant) if hist is None else hist
    dt0 = np.asarray(dt0, np.float64)
    if n_acc is None:
        n_acc = own_stops(dt0, hist["T"], T_thresh)
    n_acc = np.asarray(n_acc, np.int64)
    rows = np.arange(len(n_acc))
    # the stop applied to one payload only: the second runs on to the end of the list
    sel_b = valid_counts(dt0) if mutant == "stop_one_payload" else n_acc
    return dict(W=hist["W"][rows, n_acc], depth=hist["depth"][rows, n_acc], A=hist["A"][rows, n_acc], B=hist["B"][rows, sel_b], n_acc=n_acc, T=hist["T"])


def valid_counts(dt0):
    """Samples before the first empty slot, per ray."""
    n, S = dt0.shape
    empty = dt0 == 0
    return np.where(empty.any(1), empty.argmax(1), S).astype(np.int64)


def own_stops(dt0, T, T_thresh):
    """n_acc [n] from the tests as this evaluation sees them: the first empty slot stops before it, the first T < T_thresh after it."""
    cnt = valid_counts(dt0)
    below = (T < T_thresh) & (np.arange(dt0.shape[1])[None, :] < cnt[:, None])
    return np.where(below.any(1), below.argmax(1) + 1, cnt).astype(np.int64)


def magnitudes(sigma, dt0, dt1, a, b):
    """First-order magnitudes after each number of accumulated samples: dict of [n, S + 1(, 3)] for W, depth, A, B and T [n,S] for the
    transmittance the tests see (module docstring, ragged_ref.burst_magnitudes from zero accumulators, the second payload added)."""
    sg, d0, d1, pa, pb = _t(sigma), _t(dt0), _t(dt1), _t(a), _t(b)
    n, S = sg.shape
    W, t = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    M_W, S_W, M_dp, S_dp, S_t = (torch.zeros(n, dtype=torch.float64) for _ in range(5))
    M_A, S_A, M_B, S_B = (torch.zeros(n, 3, dtype=torch.float64) for _ in range(4))
    res = dict(W=[M_W], depth=[M_dp], A=[M_A], B=[M_B], T=[])
    for j in range(S):
        x = -sg[:, j] * d0[:, j]
        ex = torch.exp(x)
        alpha = 1 - ex
        m_alpha = ex * (2 * x.abs() + 1) + alpha.abs()
        T = 1 - W
        m_T = M_W + S_W + T.abs()
        w = alpha * T
        m_w = m_alpha * T.abs() + alpha.abs() * m_T + w.abs()
        W = W + w
        M_W, S_W = M_W * (1 - alpha).abs() + m_alpha * T.abs() + alpha.abs() * T.abs() + w.abs(), S_W + w.abs()
        t = t + d1[:, j]
        S_t = S_t + d1[:, j].abs()
        M_dp, S_dp = M_dp + m_w * t.abs() + w.abs() * S_t + (w * t).abs(), S_dp + (w * t).abs()
        wa, wb = w[:, None] * pa[:, j], w[:, None] * pb[:, j]
        M_A, S_A = M_A + m_w[:, None] * pa[:, j].abs() + wa.abs(), S_A + wa.abs()
        M_B, S_B = M_B + m_w[:, None] * pb[:, j].abs() + wb.abs(), S_B + wb.abs()
        res["T"].append(m_T)
        for k, v in (("W", M_W + S_W), ("depth", M_dp + S_dp), ("A", M_A + S_A), ("B", M_B + S_B)):
            res[k].append(v)
    return {k: (torch.stack(v, 1).numpy() if v else np.zeros((n, 0))) for k, v in res.items()}


def composite_bounds(mags, n_acc):
    """name -> bound [n(,3)] of W, depth, A, B at the decisions n_acc: C U (T + K) mag + (T + K) 2^-126 with T = n_acc."""
    rows = np.arange(len(n_acc))
    T = np.asarray(n_acc, np.float64)
    out = {}
    for k in ("W", "depth", "A", "B"):
        m = mags[k][rows, n_acc]
        Tk = T[:, None] if m.ndim == 2 else T
        out[k] = C * U * (Tk + K) * m + (Tk + K) * TINY
    return out


def stop_range(dt0, T, m_T, T_thresh):
    """(lo, hi) [n]: the n_acc float64 cannot exclude. A sample's test is undecided when |T - T_thresh| <= its bound; T never increases, so
    the candidates run from the first undecided sample's j + 1 to the first clearly decided stop (the end of the list if there is none)."""
    dt0 = np.asarray(dt0, np.float64)
    S = dt0.shape[1]
    cnt = valid_counts(dt0)
    j = np.arange(S)[None, :]
    bound = C * U * (j + 1 + K) * m_T + (j + 1 + K) * TINY
    inside = j < cnt[:, None]
    undecided = inside & (T_thresh > 0) & (np.abs(T - T_thresh) <= bound)
    clear = inside & ~undecided & (T < T_thresh)
    hi = np.where(clear.any(1), clear.argmax(1) + 1, cnt).astype(np.int64)
    early = undecided & (j < hi[:, None])
    lo = np.where(early.any(1), early.argmax(1) + 1, hi).astype(np.int64)
    return lo, hi


def finish(acc, W, dtype=torch.float64, mutant=None):
    """(b) of the module docstring -> normal [n,3], normal_rgb [n,3], s [n,3] (numpy, float64 values)."""
    A, w = _t(acc, dtype), _t(W, dtype)
    ws = w * w if mutant == "wrong_W" else w            # the W of s taken wrong (W^2: the weights squared, as a transmittance mix-up would give)
    s = 2 * A - ws[:, None]
    m = s.abs().max(dim=1).values
    ok = (m > 0) & torch.isfinite(s).all(dim=1)
    u = s / torch.where(ok, m, torch.ones_like(m))[:, None]
    length = torch.sqrt(u[:, 2] * u[:, 2] + (u[:, 1] * u[:, 1] + u[:, 0] * u[:, 0]))
    normal = torch.where(ok[:, None], u / torch.where(ok, length, torch.ones_like(length))[:, None], torch.zeros_like(u))
    rgb = A + (1 - w)[:, None]
    return tuple(x.to(torch.float64).numpy() for x in (normal, rgb, s))


def finish_bounds(acc, W, b_acc, b_W):
    """Bounds of `finish()`'s outputs given those of its inputs -> b_normal [n,3], b_rgb [n,3], unresolved [n] (|s| within its own error:
    no direction to compare)."""
    normal, rgb, s = finish(acc, W)
    acc, W = np.asarray(acc, np.float64), np.asarray(W, np.float64)
    b_s = 2 * b_acc + b_W[:, None] + U * np.abs(s) + TINY
    d = np.sqrt((b_s ** 2).sum(1))
    length = np.sqrt((s ** 2).sum(1))
    unresolved = d >= length
    direction = np.where(unresolved, np.inf, 2 * d / np.where(unresolved, 1.0, 2 * length - d))
    b_normal = np.repeat((direction + 6 * U)[:, None], 3, 1)
    b_rgb = b_acc + b_W[:, None] + U * np.abs(1 - W)[:, None] + U * np.abs(rgb) + TINY
    return b_normal, b_rgb, unresolved


def render(sigma, dt0, dt1, a, b, T_thresh, n_acc=None, hist=None, mags=None):
    """composite + finish of the second payload at the decisions n_acc (None: float64's own) with every bound:
    dict W, depth, A, B, normal, normal_rgb and b_<name> for each, `unresolved` [n], n_acc. hist, mags: `history()` / `magnitudes()` of
    the same lists, when several decisions are looked at."""
    c = composite(sigma, dt0, dt1, a, b, T_thresh, n_acc=n_acc, hist=hist)
    cb = composite_bounds(magnitudes(sigma, dt0, dt1, a, b) if mags is None else mags, c["n_acc"])
    normal, rgb, _ = finish(c["B"], c["W"])
    b_normal, b_rgb, unresolved = finish_bounds(c["B"], c["W"], cb["B"], cb["W"])
    out = dict(c, normal=normal, normal_rgb=rgb, b_normal=b_normal, b_normal_rgb=b_rgb, unresolved=unresolved)
    out.update({"b_" + k: v for k, v in cb.items()})
    return out


def best_ratio(got, sigma, dt0, dt1, a, b, T_thresh, names):
    """got: name -> array of the evaluation under test. Per ray the worst |got - want| / bound over `names` at the best of the stop decisions
    float64 cannot exclude (all of a ray's outputs at ONE decision) -> (ratio [n], unresolved [n] at that decision, rays with > 1 candidate).
    An unresolved pixel's `normal` is left out of its ray's ratio (its bound is infinite)."""
    h = history(sigma, dt0, dt1, a, b)
    m = magnitudes(sigma, dt0, dt1, a, b)
    lo, hi = stop_range(dt0, h["T"], m["T"], T_thresh)
    n = len(lo)
    best, unres = np.full(n, np.inf), np.zeros(n, bool)
    for k in range(int((hi - lo).max(initial=0)) + 1):
        ref = render(sigma, dt0, dt1, a, b, T_thresh, n_acc=np.minimum(lo + k, hi), hist=h, mags=m)
        ray = np.zeros(n)
        for name in names:
            diff = np.abs(np.asarray(got[name], np.float64) - ref[name])
            with np.errstate(invalid="ignore"):
                r = np.where(np.isinf(ref["b_" + name]), 0.0, diff / ref["b_" + name])
            r = np.where(np.isfinite(np.asarray(got[name], np.float64)), r, np.inf)
            ray = np.maximum(ray, r.reshape(n, -1).max(1))
        better = ray < best
        best, unres = np.where(better, ray, best), np.where(better, ref["unresolved"], unres)
    return best, unres, hi > lo


# ---------------------------------------------------------------- cases: sample lists as a march through a soft object leaves them
def random_lists(rng, n, S, opaque=0.5, thin=False):
    """sigma, dt0, dt1 [n,S] fp32 values, a, b [n,S,3] fp32 values in [0,1]; rays of random length (some empty), densities such that about
    `opaque` of the rays reach T < 1e-4 (thin: none does), the second payload an encoded unit normal that turns slowly along the ray."""
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    count = rng.integers(0, S + 1, n)
    count[rng.random(n) < 0.2] = S
    dt = f32(rng.uniform(0.5, 1.5, (n, S)) * (2 * np.sqrt(3) / 1024))
    valid = np.arange(S)[None, :] < count[:, None]
    dt0 = np.where(valid, dt, 0.0)
    dt1 = f32(dt0 * np.where(rng.random((n, S)) < 0.1, rng.uniform(1, 30, (n, S)), 1.0))
    level = np.where(rng.random(n) < opaque, 10.0 ** rng.uniform(2, 3.5, n), 10.0 ** rng.uniform(-1, 1.5, n))
    if thin:
        level = 10.0 ** rng.uniform(-1, 0.5, n)
    sigma = f32(level[:, None] * rng.uniform(0, 2, (n, S)) * (rng.random((n, S)) < 0.7))
    a = f32(rng.random((n, S, 3)))
    base = rng.standard_normal((n, 1, 3)) + 0.15 * np.cumsum(rng.standard_normal((n, S, 3)), 1)
    unit = base / np.linalg.norm(base, axis=2, keepdims=True)
    unit[rng.random((n, S)) < 0.05] = 0.0                             # a zero normal (a flat spot of the field): encoded 0.5
    b = f32(np.float32(0.5) + np.float32(0.5) * unit.astype(np.float32))
    return sigma, dt0, dt1, a, b
