"""Float64 definition of the ray geometry and of the occupancy march, and the bands inside which an fp32 evaluation may decide otherwise:
near_far_from_aabb (raymarching.cu:92-145), sph_from_ray (:163-198), the cell lookup (mip_from_pos / mip_from_dt :42-54, the truncating
grid position :370-379, the Morton index :56-71), the training march (:348-480) and the inference burst (:700-805). Plain numpy and
Python floats; nothing of the project is imported, and no value here comes from the oracle or a kernel.

The march is a chain of discontinuous decisions, so it is not compared value by value with one float64 run. Instead a kernel's OUTPUT is
checked against the definition (`check_train`, `check_burst`), re-synchronised at every emitted sample:

    t0      = near + clamp(near dt_gamma, dt_min, dt_max) noise          (:351; the burst: from rays_t, :746)
    S_k     = t0 + sum(deltas[:k+1, 1])     the march's t after sample k (deltas[k, 1] = t - last_t, :461, :784)
    T_k     = S_k - deltas[k, 0]            the t at which sample k was looked up
    dt_min  = 2 sqrt(3) / max_steps         dt_max = 2 sqrt(3) 2^(C-1) / H

  * structure: rays[:, 0] the ray number, offsets the exclusive prefix sum of the counts from the counter's entry value, counter =
    (total, N) added, counts <= max_steps, dirs the ray's direction bit for bit;
  * values: deltas[k, 0] = clamp(T_k dt_gamma, dt_min, dt_max), xyzs[k] = clamp(o + T_k d, -bound, bound), T_k < far;
  * soundness: the cell of xyzs[k] at level(xyzs[k], deltas[k, 0]) is occupied (`soundness`, vectorised: xyzs and deltas are the very
    fp32 numbers the kernel looked up, so only the lookup's own roundings remain);
  * completeness: from S_k the float64 `walk` meets its next occupied cell at T_{k+1}; from t0 it meets sample 0; behind the last sample it
    leaves the range (t >= far) unless the ray stopped at its cap (max_steps, the burst: n_step). A ray whose fp32 near >= far has no
    sample: t0 = fl(near + something >= 0) >= near >= far exactly. A ray dropped for lack of room is counted by `count` instead.

deltas[:, 1] after a skip is t - last_t INCLUDING the skipped stretch (:461, :784; composite_rays adds it to rays_t, :871, :899): that is
what makes S_k the march's t, and what the depth integrates. A burst's unfilled slots are all zero (deltas[., 0] == 0 ends the ray in
composite_rays, :858), the filled ones a prefix; list entries < 0 leave their slots zero; the normalised form stores (x + bound) / (2 bound).

Bounds follow fixed_tail_ref.py: C 2^-24 (n + K) mag, C = 2, K = 16, n the roundings on the quantity's path, mag its first-order
magnitude. Derivations:
  near_far   a slab value v = (a - o) * (1 / d): subtraction, reciprocal, product: n = 3, mag |v|. Selecting and swapping are exact, so
             near and far carry n = 3 with mag max(|near|, |far|). A comparison a > b (hit or miss; near < min_near) is undecided when
             |a - b| <= bound(a) + bound(b); comparisons with inf or NaN are the same in both formats. A miss writes FLT_MAX twice.
  sph        mag carried through every operation by fixed_tail_ref's rules (sqrt(a): mag(a) / (2 sqrt a) + sqrt a; atan2(p, q): (|q|
             mag(p) + |p| mag(q)) / (p^2 + q^2) + |result|), n = 18 operations on the longest path. The cancellation of B^2 - A C and the
             1 / (x^2 + z^2) of both atan2 near the poles are in the magnitudes. phi / pi is compared modulo 2 within the bound of +-1.
  T_k        t0 costs 3 roundings; deltas[j, 1] = fl(S_j - S_{j-1}) errs by <= 2^-24 of ITSELF (exactly 0 unless a skip more than doubled
             t), so the whole sum errs by <= 2^-24 S_k: one more; S_k = fl(T_k + dt): one more. e_T = C 2^-24 (5 + K) S_k whatever k.
  deltas0    e_T dt_gamma + bound(n = 3: the product and the two roundings of dt_min's constant, mag the value).
  xyzs       e_T |d| + bound(n = 2, mag |o| + |T_k d|); normalised: that / (2 bound) + bound(n = 2, mag (|x| + bound) / (2 bound)).
  lookup     max|x| and its exponent are exact; dt H / 2: n = 1; the grid coordinate g = 0.5 (x / mip_bound + 1) H: reciprocal, product,
             sum, the conversion of the double product: n = 4, mag (|x| / mip_bound + 1) H / 2. `clear` is false when g is within that (plus
             what x itself is uncertain by) of a cell face 1 .. H-1, or max|x| or dt H / 2 within it of a power of two at which the
             clamped level changes (2^0 .. 2^(C-2)). level H^3 + morton is evaluated in fp32 (:378): exact below 2^24, else not clear.
  the walk   every lattice step t += clamp(t dt_gamma, dt_min, dt_max) rounds the sum (2^-24 t) and the step (<= 3 2^-24 dt, and the steps
             add up to less than t): after j steps the float64 t and the fp32 t differ by at most e_t(j) = e_0 + C 2^-24 (j + K) t.
             The skip's target tt = t + (face - x) / d does not move with t (it is the parameter at which the ray leaves the cell): it
             carries the rounding of x = fl(o + t d) divided by |d|, n = 6 on (|face| + |x|) / |d|, and its own sum.
             Decisions: a lookup that is not clear, |t - tt| <= e_t + e_tt, |t - far| <= e_t. The caps (max_steps, n_step) compare
             integers: their band has no width. Any decision inside its band ends the walk as undecided; the gap is then left out.

`PLAN` names the cases both test files use (`fields`, `burst_fields`, `near_far_cases`, `sph_cases`): H = 32 throughout, (bound, C) in
(1, 1), (2, 2), (4, 3) and, beyond what the reference derives for powers of two, (1.5, 2) where mip_bound = min(2^level, bound) clamps.

`walker_train` / `walker_burst` are a small fp32 per-ray restatement kept for test_march_ref.py alone: it shows that the checks accept a
correct fp32 march written independently of the oracle, and reject each of `MUTANTS`. No reference value ever comes from it.
"""
import math

import numpy as np

U = 2.0 ** -24
C, K = 2.0, 16
FLT_MAX = float(np.finfo(np.float32).max)
NOISE_MAX = float(np.float32(0.99999994))
INF = float("inf")
SQRT3 = math.sqrt(3.0)
MUTANTS = ("skip_ignores_sign", "level_from_pos_only", "index_rounds", "far_inclusive", "delta1_is_dt", "dt_unclamped", "noise_scales_dt_min",
           "skip_one_step_more", "skip_one_step_less", "morton_axes_swapped", "mip_bound_unclamped", "burst_keeps_stale_slot")


def bnd(n, mag):
    return C * U * (n + K) * mag


def ratios(got, want, scale):
    """|got - want| / scale elementwise (scale already holds C: the assertion is ratio <= 1). scale == 0: equal or inf. Non-finite values
    must sit where float64 has them: NaN on NaN, an infinity on the same infinity."""
    got, want, scale = np.broadcast_arrays(np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(scale, np.float64))
    fin = np.isfinite(got) & np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        err = np.abs(got - want)
        r = np.where(err == 0, 0.0, err / np.where(scale > 0, scale, 0.0))
        same = (np.isnan(got) & np.isnan(want)) | (got == want)
    return np.where(fin, np.nan_to_num(r, nan=np.inf, posinf=np.inf), np.where(same, 0.0, np.inf))


def step_range(cfg):
    """dt_min, dt_max (:345-346)."""
    return 2 * SQRT3 / cfg["max_steps"], 2 * SQRT3 * 2.0 ** (cfg["C"] - 1) / cfg["H"]


# ---------------------------------------------------------------- near_far_from_aabb, sph_from_ray
def near_far(o, d, aabb, min_near):
    """The slab test in its statement order on fp32 values o, d [N,3], aabb [6]. Returns near, far, mag, decided (module docstring)."""
    o, d, aabb = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(aabb, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rd = 1.0 / d                                                    # 1 / +-0 = +-inf
        lo, hi = (aabb[None, :3] - o) * rd, (aabb[None, 3:] - o) * rd   # 0 * inf = NaN: an origin on a slab plane, zero component
        sw = lo > hi                                                    # false on NaN: no swap, as `if (near > far) swapf`
        lo, hi = np.where(sw, hi, lo), np.where(sw, lo, hi)

        def close(a, b):
            return np.isfinite(a) & np.isfinite(b) & (np.abs(a - b) <= bnd(3, np.abs(a)) + bnd(3, np.abs(b)))
        near, far = lo[:, 0], hi[:, 0]
        miss, und = np.zeros(len(o), bool), np.zeros(len(o), bool)
        for ax in (1, 2):
            n2, f2 = lo[:, ax], hi[:, ax]
            und |= ~miss & (close(near, f2) | close(n2, far))
            miss |= (near > f2) | (n2 > far)
            near, far = np.where(n2 > near, n2, near), np.where(f2 < far, f2, far)
        und |= ~miss & close(near, np.full_like(near, min_near))
        mag = np.maximum(np.abs(near), np.abs(far))
        near = np.where(near < min_near, float(min_near), near)
    mag = np.where(miss | ~np.isfinite(mag), 0.0, mag)
    return np.where(miss, FLT_MAX, near), np.where(miss, FLT_MAX, far), mag, ~und


def near_far_ratio(got_near, got_far, o, d, aabb, min_near):
    """Per ray: the worst of near and far against the definition (bound n = 3), 0 where undecided; and the decided mask."""
    near, far, mag, decided = near_far(o, d, aabb, min_near)
    r = np.maximum(ratios(got_near, near, bnd(3, mag)), ratios(got_far, far, bnd(3, mag)))
    return np.where(decided, r, 0.0), decided


SPH_N = 18


def sph_from_ray(o, d, radius):
    """coords [N,2], their magnitudes [N,2], decided [N] (false: the discriminant's sign lies within its bound). An origin outside the
    sphere with a negative discriminant gives NaN in both coordinates."""
    o, d, r = np.asarray(o, np.float64), np.asarray(d, np.float64), float(np.float32(radius))
    ao, ad = np.abs(o), np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        A = (d * d).sum(-1); mA = 2 * A
        B = (o * d).sum(-1); mB = (ao * ad).sum(-1) + np.abs(B)
        oo = (o * o).sum(-1)
        Cc = oo - r * r; mC = 2 * oo + 2 * r * r + np.abs(Cc)
        disc = B * B - A * Cc
        mD = 2 * np.abs(B) * mB + B * B + mA * np.abs(Cc) + A * mC + np.abs(A * Cc) + np.abs(disc)
        decided = np.abs(disc) > bnd(SPH_N, mD)
        sq = np.sqrt(disc)
        mS = np.where(sq > 0, mD / (2 * sq), 0.0) + sq
        num = -B + sq; mN = mB + mS + np.abs(num)
        t = num / A; mT = mN / A + np.abs(num) * mA / (A * A) + np.abs(t)
        p = o + t[:, None] * d
        mP = mT[:, None] * ad + np.abs(t[:, None] * d) + np.abs(p)
        x, y, z, mx, my, mz = p[:, 0], p[:, 1], p[:, 2], mP[:, 0], mP[:, 1], mP[:, 2]
        rho2 = x * x + z * z
        mR2 = 2 * np.abs(x) * mx + 2 * np.abs(z) * mz + 2 * rho2
        rho = np.sqrt(rho2)
        mR = np.where(rho > 0, mR2 / (2 * rho), np.where(mR2 > 0, np.inf, 0.0)) + rho
        theta = np.arctan2(rho, y)
        den = rho2 + y * y
        mTh = np.where(den > 0, (np.abs(y) * mR + rho * my) / den, np.inf) + np.abs(theta)
        phi = np.arctan2(z, x)
        mPh = np.where(rho2 > 0, (np.abs(x) * mz + np.abs(z) * mx) / rho2, np.where((mx > 0) | (mz > 0), np.inf, 0.0)) + np.abs(phi)
        c0 = 2 * theta / np.pi - 1
        c1 = phi / np.pi
        m0 = 2 * mTh / np.pi + 2 * np.abs(2 * theta / np.pi) + np.abs(c0)
        m1 = mPh / np.pi + 2 * np.abs(c1)
    return np.stack([c0, c1], -1), np.stack([m0, m1], -1), decided


def sph_ratio(got, o, d, radius):
    """Per ray worst ratio of both coordinates (0 where undecided); phi / pi modulo 2 where the definition is within the bound of +-1."""
    want, mag, decided = sph_from_ray(o, d, radius)
    got = np.asarray(got, np.float64)
    scale = bnd(SPH_N, np.nan_to_num(mag, nan=0.0, posinf=np.inf))
    r = ratios(got, want, scale)
    wrap = np.isfinite(want[:, 1]) & (1.0 - np.abs(want[:, 1]) <= scale[:, 1])
    with np.errstate(invalid="ignore"):
        alt = np.minimum(ratios(got[:, 1] + 2.0, want[:, 1], scale[:, 1]), ratios(got[:, 1] - 2.0, want[:, 1], scale[:, 1]))
    r[:, 1] = np.where(wrap, np.minimum(r[:, 1], alt), r[:, 1])
    return np.where(decided, r.max(-1), 0.0), decided


# ---------------------------------------------------------------- the cell lookup
def morton(x, y, z):
    """Bit i of x, y, z at bits 3i, 3i + 1, 3i + 2 (:56-71), by its definition."""
    x, y, z = (np.asarray(a, np.int64) for a in (x, y, z))
    m = np.zeros(np.broadcast(x, y, z).shape, np.int64)
    for i in range(10):
        m |= (((x >> i) & 1) << (3 * i)) | (((y >> i) & 1) << (3 * i + 1)) | (((z >> i) & 1) << (3 * i + 2))
    return m


def level(x, dt, cfg, ex=0.0, edt=0.0):
    """max(mip_from_pos, mip_from_dt) of positions x [..., 3] and steps dt [...]; ex / edt: what x / dt are uncertain by. -> level, clear."""
    x, dt = np.asarray(x, np.float64), np.asarray(dt, np.float64)
    Cc, H = cfg["C"], cfg["H"]
    mx = np.abs(x).max(-1)
    exm = np.broadcast_to(np.asarray(ex, np.float64), x.shape).max(-1)
    v = dt * H * 0.5
    ev = np.asarray(edt, np.float64) * H * 0.5 + bnd(1, v)
    lev = np.maximum(np.clip(np.frexp(mx)[1], 0, Cc - 1), np.clip(np.frexp(v)[1], 0, Cc - 1))
    clear = np.ones(mx.shape, bool)
    for k in range(Cc - 1):
        clear &= ((np.abs(mx - 2.0 ** k) > exm) | (exm == 0)) & (np.abs(v - 2.0 ** k) > ev)
    return lev, clear


def cell(x, lev, cfg, ex=0.0):
    """The truncated grid position [..., 3] of x at `lev`, and clear."""
    x = np.asarray(x, np.float64)
    H = cfg["H"]
    mb = np.minimum(2.0 ** np.asarray(lev, np.float64), cfg["bound"])[..., None]
    g = 0.5 * (x / mb + 1.0) * H
    eg = np.asarray(ex, np.float64) * H / (2 * mb) + bnd(4, 0.5 * H * (np.abs(x) / mb + 1.0))
    r = np.rint(g)
    clear = ~((r >= 1) & (r <= H - 1) & (np.abs(g - r) <= eg)).any(-1)
    return np.clip(g, 0.0, H - 1.0).astype(np.int64), clear


def index(lev, n, cfg):
    return np.asarray(lev, np.int64) * cfg["H"] ** 3 + morton(n[..., 0], n[..., 1], n[..., 2])


def occupied(idx, bits):
    """Bit idx % 8 of byte idx / 8; clear: the fp32 sum that formed idx was exact."""
    idx = np.asarray(idx, np.int64)
    return ((np.asarray(bits)[idx >> 3] >> (idx & 7)) & 1).astype(bool), idx < 2 ** 24


def soundness(cfg, xyzs, dt, ex=0.0):
    """Per sample: occupied, clear — the cell of xyzs [n,3] at level(xyzs, dt)."""
    lev, c1 = level(xyzs, dt, cfg, ex=ex)
    n, c2 = cell(xyzs, lev, cfg, ex=ex)
    occ, c3 = occupied(index(lev, n, cfg), cfg["bits"])
    return occ, c1 & c2 & c3


# ---------------------------------------------------------------- the walk (one ray, Python floats: float64)
def _prepare(cfg):
    if "_bytes" not in cfg:
        cfg["_bytes"] = np.ascontiguousarray(cfg["bits"], np.uint8).tobytes()
        cfg["_spread"] = [int(morton(v, 0, 0)) for v in range(cfg["H"])]
    return cfg


def _recip(v):
    return math.copysign(INF, v) if v == 0.0 else 1.0 / v


def lookup(cfg, o, d, t, et):
    """The lookup of :361-379 at t (uncertain by et): None when not clear, else (occupied, x, dt, level, n, mip_bound, ex)."""
    b, Cc, H, g = cfg["bound"], cfg["C"], cfg["H"], cfg["dt_gamma"]
    dt_min, dt_max = step_range(cfg)
    raw = [oo + t * dd for oo, dd in zip(o, d)]
    x = [min(b, max(-b, v)) for v in raw]
    ex = [et * abs(dd) + bnd(2, abs(oo) + abs(t * dd)) for oo, dd in zip(o, d)]
    dt = min(dt_max, max(dt_min, t * g))
    edt = et * g + bnd(3, dt)
    mx, exm = max(abs(v) for v in x), max(ex)
    v = dt * H * 0.5
    ev = edt * H * 0.5 + bnd(1, v)
    for k in range(Cc - 1):
        p = 2.0 ** k
        if abs(mx - p) <= exm or abs(v - p) <= ev:
            return None
    lev = max(min(max(math.frexp(mx)[1], 0), Cc - 1), min(max(math.frexp(v)[1], 0), Cc - 1))
    mb = min(2.0 ** lev, b)
    n = []
    for xv, e in zip(x, ex):
        gg = 0.5 * (xv / mb + 1.0) * H
        eg = e * H / (2 * mb) + bnd(4, 0.5 * H * (abs(xv) / mb + 1.0))
        r = math.floor(gg + 0.5)
        if 1 <= r <= H - 1 and abs(gg - r) <= eg:
            return None
        n.append(int(min(max(gg, 0.0), H - 1.0)))
    sp = cfg["_spread"]
    idx = lev * H ** 3 + (sp[n[0]] | (sp[n[1]] << 1) | (sp[n[2]] << 2))
    if idx >= 2 ** 24:
        return None
    occ = (cfg["_bytes"][idx >> 3] >> (idx & 7)) & 1
    return bool(occ), x, dt, lev, n, mb, [bnd(2, abs(oo) + abs(t * dd)) + (et if abs(rv) >= b else 0.0) for oo, dd, rv in zip(o, d, raw)]


def walk(cfg, o, d, t, far, e0=0.0, max_iter=1000000):
    """From t (uncertain by e0) to the next occupied cell of one ray (o, d: 3 fp32 values each). Returns (status, t, e_t, steps): status
    "emit" (a sample is due at t), "left" (t >= far), or "undecided:lookup" / "undecided:tt" / "undecided:far"; steps: lattice steps taken."""
    _prepare(cfg)
    g, H = cfg["dt_gamma"], cfg["H"]
    dt_min, dt_max = step_range(cfg)
    o, d = [float(v) for v in o], [float(v) for v in d]
    rd = [_recip(v) for v in d]
    sg = [math.copysign(1.0, v) for v in d]
    t, far, j = float(t), float(far), 0
    while j < max_iter:
        et = e0 + bnd(j, abs(t))
        if abs(t - far) <= et:
            return "undecided:far", t, et, j
        if not t < far:
            return "left", t, et, j
        look = lookup(cfg, o, d, t, et)
        if look is None:
            return "undecided:lookup", t, et, j
        occ, x, dt, lev, n, mb, exr = look
        if occ:
            return "emit", t, et, j
        best, ebest, seen = INF, 0.0, False                                             # :390-394
        for a in range(3):
            face = ((n[a] + 0.5 + 0.5 * sg[a]) / H * 2 - 1) * mb
            ta = (face - x[a]) * rd[a]                                                  # +-inf, or 0 * inf = NaN
            if ta == ta:
                seen = True
                if ta < best:
                    best = ta
                    ebest = exr[a] * abs(rd[a]) + bnd(6, (abs(face) + abs(x[a])) * abs(rd[a])) if abs(rd[a]) < INF else 0.0
        adv = max(0.0, best) if seen else 0.0                                           # fminf / fmaxf drop a NaN
        tt = t + adv
        ett = ebest + bnd(1, abs(tt))
        while True:                                                                     # :396-398
            t += min(dt_max, max(dt_min, t * g))
            j += 1
            if abs(t - tt) <= e0 + bnd(j, abs(t)) + ett:
                return "undecided:tt", t, et, j
            if not t < tt:
                break
    raise RuntimeError("walk does not end")


def count(cfg, o, d, t0, far, cap, e0):
    """The number of samples a ray emits (at most cap) without any output to re-synchronise on; None when a decision is undecided."""
    t, n, e = float(t0), 0, e0
    while n < cap:
        status, t, et, _ = walk(cfg, o, d, t, far, e0=e)
        if status == "left":
            return n
        if status != "emit":
            return None
        n += 1
        dt = min(step_range(cfg)[1], max(step_range(cfg)[0], t * cfg["dt_gamma"]))
        t, e = t + dt, et + bnd(4, abs(t + dt))
    return n


# ---------------------------------------------------------------- checking a march's output
def _cfg(inp):
    cfg = inp.get("_cfg")
    if cfg is None:
        cfg = inp["_cfg"] = _prepare(dict(bound=float(np.float32(inp["bound"])), C=int(inp["C"]), H=int(inp["H"]),
                                          dt_gamma=float(np.float32(inp["dt_gamma"])), max_steps=int(inp["max_steps"]), bits=np.asarray(inp["bits"], np.uint8)))
    return cfg


def _start(cfg, t, noise):
    """t + clamp(t dt_gamma, dt_min, dt_max) noise (:351, :746)."""
    dt_min, dt_max = step_range(cfg)
    return t + min(dt_max, max(dt_min, t * cfg["dt_gamma"])) * noise


class Result(dict):
    """ratio: name -> worst error / bound; fail: the rules broken (strings); the counts behind the shares left out."""

    def __init__(self):
        super().__init__(ratio={}, fail=[], gaps=0, gaps_left_out=0, samples=0, samples_left_out=0, long_gaps=0, longest_gap=0, capped=0, left_out_by={})

    def worst(self, name, r):
        r = float(np.max(np.nan_to_num(np.asarray(r, np.float64), nan=np.inf), initial=0.0))      # a NaN is a miss, not a zero
        self["ratio"][name] = max(self["ratio"].get(name, 0.0), r)

    def failed(self, msg):
        if len(self["fail"]) < 20:
            self["fail"].append(msg)

    @property
    def ok(self):
        return not self["fail"] and all(v <= 1.0 for v in self["ratio"].values())

    @property
    def gap_share(self):
        return self["gaps_left_out"] / max(self["gaps"], 1)

    @property
    def sample_share(self):
        return self["samples_left_out"] / max(self["samples"], 1)


def _check_ray(res, cfg, tag, o, d, t0, far, cap, x, dl, normalised=False):
    """One ray's emitted samples x [n,3], dl [n,2] against the definition from t0 (values and completeness; soundness is the caller's)."""
    b, g = cfg["bound"], cfg["dt_gamma"]
    dt_min, dt_max = step_range(cfg)
    o64, d64 = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(x)
    dl = np.asarray(dl, np.float64)
    S = t0 + np.cumsum(dl[:, 1])
    T = S - dl[:, 0]
    eT = bnd(5, np.abs(S))
    if n:
        want_dt = np.clip(T * g, dt_min, dt_max)
        res.worst("deltas0", ratios(dl[:, 0], want_dt, eT * g + bnd(3, want_dt)))
        raw = o64[None, :] + T[:, None] * d64[None, :]
        want_x = np.clip(raw, -b, b)
        sx = eT[:, None] * np.abs(d64)[None, :] + bnd(2, np.abs(o64)[None, :] + np.abs(T[:, None] * d64[None, :]))
        if normalised:
            want_x, sx = (want_x + b) / (2 * b), sx / (2 * b) + bnd(2, (np.abs(want_x) + b) / (2 * b))
        res.worst("xyzs", ratios(x, want_x, sx))
        res.worst("t_below_far", np.maximum(T - far, 0.0) / eT)
    e_start = bnd(3, abs(t0))
    starts = [(t0, e_start)] + [(float(S[k]), float(eT[k])) for k in range(n)]
    for k, (t, e0) in enumerate(starts):
        if k == n and n == cap:
            res["capped"] += 1
            break
        res["gaps"] += 1
        status, tw, et, steps = walk(cfg, o, d, t, far, e0=e0)
        res["long_gaps"] += steps > 1
        res["longest_gap"] = max(res["longest_gap"], steps)
        if status.startswith("undecided"):
            res["gaps_left_out"] += 1
            res["left_out_by"][status] = res["left_out_by"].get(status, 0) + 1
        elif status == "emit":
            if k == n:
                res.failed(f"{tag}: the definition finds an occupied cell at t = {tw!r} behind the ray's last sample ({n} of at most {cap})")
            else:
                res.worst("next_sample_t", abs(tw - T[k]) / (et + eT[k]))
        elif k < n:
            res.failed(f"{tag}: sample {k} at t = {T[k]!r}, but the definition leaves the range from t = {t!r} (far = {far!r})")


def check_train(inp, xyzs, dirs, deltas, rays, counter, complete=True):
    """A training march's output against the definition (module docstring). inp: o, d [N,3], near, far, noise [N] (fp32 arrays), bits, bound,
    C, H, dt_gamma, max_steps, M, counter0 (the counter's entry values; absent: zeros) and normalised (xyzs holds (x + bound) / (2 bound)). Returns a Result; Result["written"] [M] marks
    the rows that belong to a ray that fits — every other row is the caller's to find untouched."""
    cfg = _cfg(inp)
    res = Result()
    o, d = np.asarray(inp["o"], np.float32), np.asarray(inp["d"], np.float32)
    near, far, noise = (np.asarray(inp[k], np.float32) for k in ("near", "far", "noise"))
    N, M, cap = len(o), int(inp["M"]), cfg["max_steps"]
    c0 = np.asarray(inp.get("counter0", (0, 0)), np.int64)
    rays, counter = np.asarray(rays, np.int64), np.asarray(counter, np.int64)
    xyzs, dirs, deltas = np.asarray(xyzs, np.float32), np.asarray(dirs, np.float32) if dirs is not None else None, np.asarray(deltas, np.float32)
    cnt, off = rays[:, 2], rays[:, 1]
    if not np.array_equal(rays[:, 0], np.arange(N)):
        res.failed("rays[:, 0] is not the ray number")
    if not np.array_equal(off, c0[0] + np.cumsum(cnt) - cnt):
        res.failed("offsets are not the exclusive prefix sum of the counts")
    if not np.array_equal(counter, [c0[0] + cnt.sum(), c0[1] + N]):
        res.failed(f"counter {counter.tolist()} is not ({c0[0] + cnt.sum()}, {c0[1] + N})")
    if cnt.min(initial=0) < 0 or cnt.max(initial=0) > cap:
        res.failed("a count lies outside [0, max_steps]")
    written = np.zeros(M, bool)
    res["written"] = written
    if res["fail"]:
        return res
    fits = (cnt > 0) & (off + cnt <= M)
    rows = np.concatenate([np.arange(off[r], off[r] + cnt[r]) for r in np.nonzero(fits)[0]] + [np.zeros(0, np.int64)]).astype(np.int64)
    owner = np.repeat(np.nonzero(fits)[0], cnt[fits])
    written[rows] = True
    if dirs is not None and not np.array_equal(dirs[rows].view(np.uint32), d[owner].view(np.uint32)):
        res.failed("dirs is not the ray's direction bit for bit")
    normalised, b = bool(inp.get("normalised", False)), cfg["bound"]
    xs, ex = xyzs[rows].astype(np.float64), 0.0
    if normalised:                                                     # the fused-range form stores the encoder's coordinates
        xs = xs * (2 * b) - b
        ex = bnd(3, np.abs(xs) + b)
    occ, clear = soundness(cfg, xs, deltas[rows, 0], ex=ex)
    res["samples"], res["samples_left_out"] = len(rows), int((~clear).sum())
    if (clear & ~occ).any():
        k = int(np.nonzero(clear & ~occ)[0][0])
        res.failed(f"{int((clear & ~occ).sum())} samples lie in cells that are clearly empty (first: row {rows[k]}, ray {owner[k]}, x = {xyzs[rows[k]].tolist()})")
    if not complete:
        return res
    for r in range(N):
        if near[r] >= far[r]:
            if cnt[r]:
                res.failed(f"ray {r}: {cnt[r]} samples on a ray with near >= far")
            continue
        t0 = _start(cfg, float(near[r]), float(noise[r]))
        if cnt[r] and not fits[r]:
            want = count(cfg, o[r], d[r], t0, float(far[r]), cap, bnd(3, abs(t0)))
            res["gaps"] += 1
            res["gaps_left_out"] += want is None
            if want is not None and want != cnt[r]:
                res.failed(f"ray {r} (dropped): counts {cnt[r]} samples, the definition {want}")
            continue
        sl = slice(off[r], off[r] + cnt[r])
        _check_ray(res, cfg, f"ray {r}", o[r], d[r], t0, float(far[r]), cap, xyzs[sl], deltas[sl], normalised=normalised)
    return res


def check_burst(inp, xyzs, dirs, deltas):
    """An inference burst's output: inp as for check_train plus n_step, rays_alive [n_alive], rays_t [n_rays], noise [n_alive] and
    normalised (positions stored as (x + bound) / (2 bound)). Slot rows are [n_alive, n_step]."""
    cfg = _cfg(inp)
    res = Result()
    o, d = np.asarray(inp["o"], np.float32), np.asarray(inp["d"], np.float32)
    far, rays_t, noise = (np.asarray(inp[k], np.float32) for k in ("far", "rays_t", "noise"))
    alive = np.asarray(inp["rays_alive"], np.int64)
    n_alive, n_step, b = len(alive), int(inp["n_step"]), cfg["bound"]
    normalised = bool(inp.get("normalised", False))
    X, D, L = (np.asarray(a, np.float32)[:n_alive * n_step].reshape(n_alive, n_step, -1) for a in (xyzs, dirs, deltas))
    filled = L[:, :, 0] != 0
    nf = filled.sum(1)
    if not np.array_equal(filled, np.arange(n_step)[None, :] < nf[:, None]):
        res.failed("the filled slots of a ray are not a prefix")
    if X[~filled].any() or D[~filled].any() or L[~filled].any():
        res.failed("an unfilled slot is not all zero")
    if nf[alive < 0].any():
        res.failed("a list entry < 0 has filled slots")
    live = np.nonzero(alive >= 0)[0]
    if not np.array_equal(D[filled].view(np.uint32), np.broadcast_to(d[np.where(alive >= 0, alive, 0)][:, None, :], D.shape)[filled].view(np.uint32)):
        res.failed("dirs is not the ray's direction bit for bit")
    if res["fail"]:
        return res
    xs = X[filled].astype(np.float64)
    ex = 0.0
    if normalised:
        xs = xs * (2 * b) - b
        ex = bnd(3, np.abs(xs) + b)
    occ, clear = soundness(cfg, xs, L[filled][:, 0], ex=ex)
    res["samples"], res["samples_left_out"] = int(filled.sum()), int((~clear).sum())
    if (clear & ~occ).any():
        res.failed(f"{int((clear & ~occ).sum())} samples lie in cells that are clearly empty")
    for r in live:
        i = alive[r]
        if rays_t[i] >= far[i]:
            if nf[r]:
                res.failed(f"entry {r}: samples on a ray with rays_t >= far")
            continue
        t0 = _start(cfg, float(rays_t[i]), float(noise[r]))
        _check_ray(res, cfg, f"entry {r} (ray {i})", o[i], d[i], t0, float(far[i]), n_step, X[r, :nf[r]], L[r, :nf[r]], normalised=normalised)
    return res


# ---------------------------------------------------------------- the named cases
H = 32
AABB = lambda b: np.array([-b, -b, -b, b, b, b], np.float32)
BLOB_RADIUS = 0.45

# name: bound, C, dt_gamma, max_steps, N, occupancy, ray kinds (ray r is of kind r % len), noise, min_near, seed (fields())
PLAN = {
    "blob-b1":       dict(bound=1, C=1, dt_gamma=0.0, max_steps=1024, N=64, occ="blob", kinds=("through", "axis", "miss", "corner", "graze"), noise="random", seed=9),
    "blob-b2":       dict(bound=2, C=2, dt_gamma=1 / 128, max_steps=1024, N=257, occ="blob", kinds=("through", "inside", "graze", "through"), noise="zero", seed=0),
    "blob-b4":       dict(bound=4, C=3, dt_gamma=0.013, max_steps=64, N=64, occ="blob", kinds=("through", "axis", "inside"), noise="max", seed=2),
    "one-ray":       dict(bound=1, C=1, dt_gamma=1 / 128, max_steps=1024, N=1, occ="blob", kinds=("through",), noise="max", seed=6),
    "rand10-b2":     dict(bound=2, C=2, dt_gamma=1 / 128, max_steps=64, N=64, occ=0.1, kinds=("through", "inside", "axis", "miss"), noise="random", seed=2),
    "rand50-b1":     dict(bound=1, C=1, dt_gamma=0.0, max_steps=1024, N=5, occ=0.5, kinds=("through", "axis"), noise="random", seed=8),
    "rand50-b4-g.3": dict(bound=4, C=3, dt_gamma=0.3, max_steps=64, N=64, occ=0.5, kinds=("inside", "through", "inside", "axis"), noise="random", min_near=0.05, seed=10),
    "rand90-b2-cap": dict(bound=2, C=2, dt_gamma=0.013, max_steps=7, N=64, occ=0.9, kinds=("through", "inside", "corner"), noise="random", seed=11),
    "rand50-b1.5":   dict(bound=1.5, C=2, dt_gamma=1 / 128, max_steps=64, N=64, occ=0.5, kinds=("through", "inside", "graze"), noise="random", seed=9),
    "full-b4-cap":   dict(bound=4, C=3, dt_gamma=0.0, max_steps=64, N=64, occ="full", kinds=("through", "inside", "axis"), noise="zero", seed=5),
    "full-b1-g.3":   dict(bound=1, C=1, dt_gamma=0.3, max_steps=1024, N=5, occ="full", kinds=("through", "corner"), noise="max", seed=4),
    "empty-b2":      dict(bound=2, C=2, dt_gamma=1 / 128, max_steps=7, N=257, occ="empty", kinds=("through", "axis", "inside", "miss"), noise="random", seed=3),
}
# what a case is meant to show (test_march_ref.py asserts it on the oracle's output): samples, gaps of more than one lattice step, rays at the cap
MEANT = {"blob-b1": "sg", "blob-b2": "sg", "blob-b4": "sg", "one-ray": "sg", "rand10-b2": "sg", "rand50-b1": "sg", "rand50-b4-g.3": "sg",
         "rand90-b2-cap": "sgc", "rand50-b1.5": "sg", "full-b4-cap": "sc", "full-b1-g.3": "s", "empty-b2": "g"}


# (case, n_step, normalised) of the burst tests: every case at every burst length. A burst has few gaps, so its rays_t (burst_fields) starts
# shortly before the blob where the case has one: the way from the box to the first sample is 150 to 570 lattice steps at max_steps = 1024,
# which the band of the walk leaves undecided too often for the caps.
BURSTS = [(n, s, s == 8) for s in (1, 4, 8) for n in PLAN]


def occupancy(kind, bound, Cc, seed):
    """Packed bits [C H^3 / 8]: "blob" (cells whose centre lies within BLOB_RADIUS of the origin, at every level), a fill share, "empty", "full"."""
    n = Cc * H ** 3
    if kind == "empty":
        return np.zeros(n // 8, np.uint8)
    if kind == "full":
        return np.full(n // 8, 255, np.uint8)
    if kind == "blob":
        flat = np.zeros(n, bool)
        ar = np.arange(H)
        c = np.stack(np.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(-1, 3)
        for lev in range(Cc):
            centre = ((c + 0.5) / H * 2 - 1) * min(2.0 ** lev, bound)
            flat[lev * H ** 3 + morton(c[:, 0], c[:, 1], c[:, 2])] = (centre ** 2).sum(-1) < BLOB_RADIUS ** 2
    else:
        flat = np.random.default_rng(1000 + seed).random(n) < kind
    return np.packbits(flat.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)


def _unit(v):
    return v / np.linalg.norm(v)


def make_ray(kind, bound, rng, dt_min):
    """One ray of a kind (module PLAN). Values are rounded to fp32 by the caller."""
    b = float(bound)
    if kind == "through":                                             # from outside the box at a point inside the blob
        o = _unit(rng.normal(size=3)) * b * rng.uniform(1.8, 2.5)
        return o, _unit(_unit(rng.normal(size=3)) * rng.uniform(0, 0.4) - o)
    if kind == "axis":                                                # axis-parallel, the zero components +0.0 and -0.0
        a, s = int(rng.integers(3)), float(rng.choice([-1.0, 1.0]))
        o = rng.uniform(-0.4, 0.4, 3)
        o[a] = -s * b * 1.5
        d = np.array([0.0, -0.0, 0.0]) if rng.random() < 0.5 else np.array([-0.0, 0.0, -0.0])
        d[a] = s
        return o, d
    if kind == "miss":
        o = _unit(rng.normal(size=3)) * b * 3
        return o, _unit(np.cross(o, rng.normal(size=3)))
    if kind == "inside":                                              # near = min_near
        return rng.uniform(-0.3, 0.3, 3), _unit(rng.normal(size=3))
    if kind == "graze":                                               # along a face, inside the outermost layer of cells
        a, f = int(rng.integers(3)), int(rng.integers(1, 3))
        o = rng.uniform(-0.5, 0.5, 3) * b
        o[a] = -1.5 * b
        o[(a + f) % 3] = b * (1 - rng.uniform(0.002, 0.02)) * float(rng.choice([-1.0, 1.0]))
        d = rng.normal(size=3) * 0.002
        d[a] = 1.0
        return o, _unit(d)
    if kind == "corner":                                              # cuts an edge of the box: far - near < dt_min
        a = int(rng.integers(3))
        e = dt_min * rng.uniform(0.05, 0.3)
        p = np.array([b - e, b - e, b - e])
        p[a] = rng.uniform(-0.5, 0.5) * b
        d = np.ones(3)
        d[(a + 1) % 3] = -1.0
        d[a] = rng.uniform(-0.1, 0.1)
        d = _unit(d)
        return p - d * b * 0.7, d
    raise KeyError(kind)


def fields(name):
    """The arrays of a named case: o, d [N,3], near, far, noise [N] (fp32; near / far are the definition's, rounded), bits, and the scalars."""
    p = PLAN[name]
    seed = p["seed"]                                                 # chosen so that the definition alone meets the caps (test_march_ref.py)
    rng = np.random.default_rng(seed)
    N, b, Cc = p["N"], p["bound"], p["C"]
    min_near = p.get("min_near", 0.2)
    dt_min = 2 * SQRT3 / p["max_steps"]
    rays = [make_ray(p["kinds"][r % len(p["kinds"])], b, rng, dt_min) for r in range(N)]
    o, d = np.array([r[0] for r in rays], np.float32), np.array([r[1] for r in rays], np.float32)
    near, far, _, decided = near_far(o, d, AABB(b), np.float32(min_near))
    noise = dict(zero=np.zeros(N), max=np.full(N, NOISE_MAX), random=rng.random(N))[p["noise"]].astype(np.float32)
    if p["noise"] == "random":
        noise[::7], noise[3::7] = 0.0, NOISE_MAX
    return dict(name=name, o=o, d=d, near=near.astype(np.float32), far=far.astype(np.float32), noise=noise, bits=occupancy(p["occ"], b, Cc, seed),
                bound=float(b), C=Cc, H=H, dt_gamma=float(p["dt_gamma"]), max_steps=p["max_steps"], N=N, M=N * p["max_steps"], min_near=float(min_near),
                occ=p["occ"], aabb=AABB(b), kinds=[p["kinds"][r % len(p["kinds"])] for r in range(N)], near_far_decided=decided)


def burst_fields(inp, n_step, dead=True, normalised=False, seed=0):
    """A first burst on a case's rays: a shuffled list (with entries < 0 when `dead`), rays_t = near (blob cases: see BURSTS), noise per list entry."""
    rng = np.random.default_rng(77 + seed)
    N = inp["N"]
    alive = rng.permutation(N).astype(np.int32)
    if dead and N > 2:
        alive[rng.random(N) < 0.2] = -1
        alive[1] = -1
    out = {k: v for k, v in inp.items() if not k.startswith("_") or k == "_cfg"}
    rays_t = inp["near"].copy()
    if inp["occ"] == "blob":                                          # from shortly before the blob; a ray that passes it by: shortly before far
        o, d = inp["o"].astype(np.float64), inp["d"].astype(np.float64)
        dn = np.linalg.norm(d, axis=1)
        tc = -(o * d).sum(1) / dn ** 2
        passes = np.linalg.norm(o + tc[:, None] * d, axis=1) < BLOB_RADIUS + 0.15
        start = np.where(passes, tc - (BLOB_RADIUS + 0.15) / dn, inp["far"] - 0.1 / dn)
        hit = inp["near"] < inp["far"]
        rays_t = np.where(hit, np.maximum(inp["near"], np.minimum(start, inp["far"] - 0.1 / dn)), inp["near"]).astype(np.float32)
    hits = [int(i) for i in alive if i >= 0 and inp["near"][i] < inp["far"][i]]
    if len(hits) > 1:                                                 # one ray stands exactly at its far: t < far is false, no sample
        rays_t[hits[0]] = inp["far"][hits[0]]
    out.update(n_step=n_step, rays_alive=alive, rays_t=rays_t, noise=inp["noise"][np.where(alive >= 0, alive, 0)].copy(), normalised=normalised)
    return out


def first_rays(inp, n):
    """The case cut to its first n rays (the fp32 walker takes 64)."""
    out = {k: (v[:n] if k in ("o", "d", "near", "far", "noise", "kinds", "near_far_decided") else v) for k, v in inp.items() if k != "_cfg"}
    out.update(N=min(n, inp["N"]), M=min(n, inp["N"]) * inp["max_steps"])
    return out


def next_burst(b, deltas):
    """The list and rays_t after a burst, as composite_rays leaves them for rays that filled every slot (:871, :894-899): t += deltas[:, 1]
    slot by slot in fp32; a ray with an unfilled slot is finished (-1). No noise in a later burst."""
    n_alive, n_step = len(b["rays_alive"]), b["n_step"]
    L = np.asarray(deltas, np.float32)[:n_alive * n_step].reshape(n_alive, n_step, 2)
    alive, t = b["rays_alive"].copy(), b["rays_t"].copy()
    for r in range(n_alive):
        if alive[r] < 0:
            continue
        if (L[r, :, 0] == 0).any():
            alive[r] = -1
            continue
        for k in range(n_step):
            t[alive[r]] = np.float32(t[alive[r]] + L[r, k, 1])
    return dict(b, rays_alive=alive, rays_t=t, noise=np.zeros(n_alive, np.float32))


def near_far_cases():
    """name -> (o, d, aabb, min_near): every PLAN case's rays, and constructed ones: zero components of both signs, origins exactly on a
    slab plane with a zero component (0 * inf = NaN), rays through an edge (near == far: undecided), rays starting inside."""
    out = {name: (f["o"], f["d"], f["aabb"], np.float32(f["min_near"])) for name, f in ((n, fields(n)) for n in PLAN)}
    z, nz = 0.0, -0.0
    o = np.array([[-3, 0.25, 0.5], [-3, 0.25, 0.5], [3, 1.0, 0.5], [3, -1.0, 0.5], [0.5, 1.0, -3], [0.5, 0.25, 1.0], [-3, 1.5, 0.5], [-3, 1.5, 0.5],
                  [0.1, 0.2, 0.3], [-2, -2, 0.3], [-3, 1.0, 1.0], [1.0, 1.0, 1.0], [0.25, -3, 0.5], [-2, 0, 0.3]], np.float32)
    d = np.array([[1, z, z], [1, nz, nz], [-1, z, z], [-1, nz, z], [z, z, 1], [z, nz, -1], [1, z, z], [1, nz, z],
                  [z, z, 1], [1, 1, z], [1, z, nz], [nz, z, -1], [nz, 1, nz], [1, 1, z]], np.float32)      # the last: through the edge x = -1, y = 1
    out["constructed"] = (o, d, AABB(1), np.float32(0.2))
    return out


def sph_cases():
    """o, d, radius: origins at the centre and near the sphere, directions through both poles and along phi = +-pi, an origin outside."""
    rng = np.random.default_rng(5)
    r = 3.0
    o, d = [], []
    for dv in ([0, 1, 0], [0, -1, 0], [-1, 0, 0], [-1, 0, 1e-7], [-1, 0, -1e-7], [-1, 1e-4, 0], [1, 0, 0], [0, 0, 1], [1e-4, 1, 0], [0, -1, 1e-5]):
        o.append([0, 0, 0]); d.append(dv)
    for _ in range(12):                                               # near the sphere, aimed at a pole / at phi = +-pi
        p = _unit(rng.normal(size=3)) * r * rng.uniform(0.9, 0.999)
        target = np.array([[0, r, 0], [0, -r, 0], [-r, 0, 0]][len(o) % 3], float) + rng.normal(size=3) * 1e-3
        o.append(p); d.append(_unit(target - p))
    for _ in range(30):                                               # ordinary
        o.append(rng.uniform(-1, 1, 3)); d.append(_unit(rng.normal(size=3)) * rng.uniform(0.5, 2.0))
    o.append([5, 0, 0]); d.append([0, 1, 0])                          # outside, negative discriminant: NaN
    o.append([0, 4, 0]); d.append(_unit(np.array([1.0, 0.3, 0.2])))   # outside, misses: NaN
    o.append([4, 0, 0]); d.append([-1, 0, 0])                         # outside, hits: the far intersection
    return np.array(o, np.float32), np.array(d, np.float32), r


# ---------------------------------------------------------------- the fp32 walker of the CPU test (never a reference value)
def _march32(cfg, o, d, t, far, cap, mutant=None):
    """One ray in np.float32 arithmetic, every operation rounded on its own: the samples [(x, y, z, dt, delta1)] from t, at most cap."""
    f = np.float32
    H, Cc = cfg["H"], cfg["C"]
    b, g = f(cfg["bound"]), f(cfg["dt_gamma"])
    dt_min = f(2) * f(SQRT3) / f(cfg["max_steps"])
    dt_max = f(2) * f(SQRT3) * f(1 << (Cc - 1)) / f(H)
    rH = f(1) / f(H)
    o, d = [f(v) for v in o], [f(v) for v in d]
    sp = cfg["_spread"]
    out = []
    with np.errstate(all="ignore"):
        rd = [f(1) / v for v in d]
        clamp = lambda v, lo, hi: min(hi, max(lo, v))
        if mutant == "dt_unclamped":
            step = lambda tv: max(tv * g, dt_min)
        else:
            step = lambda tv: clamp(tv * g, dt_min, dt_max)
        t = f(t)
        last = t
        looks = 0
        while (t <= far if mutant == "far_inclusive" else t < far) and len(out) < cap and looks < 20000:    # (a mutant may never end)
            looks += 1
            x = [clamp(oo + t * dd, -b, b) for oo, dd in zip(o, d)]
            dt = step(t)
            l1 = min(Cc - 1, max(0, int(np.frexp(max(abs(v) for v in x))[1])))
            l2 = min(Cc - 1, max(0, int(np.frexp(f(dt * f(H)) * f(0.5))[1])))
            lev = l1 if mutant == "level_from_pos_only" else max(l1, l2)
            mb = f(2.0 ** lev) if mutant == "mip_bound_unclamped" else min(f(2.0 ** lev), b)
            rb = f(1) / mb
            n = []
            for v in x:
                gg = clamp(f(0.5 * float(f(v * rb) + f(1)) * H), f(0), f(H - 1))
                n.append(int(np.rint(gg)) if mutant == "index_rounds" else int(gg))
            m = n if mutant != "morton_axes_swapped" else [n[1], n[0], n[2]]
            idx = lev * H ** 3 + (sp[m[0]] | (sp[m[1]] << 1) | (sp[m[2]] << 2))
            if (cfg["_bytes"][idx >> 3] >> (idx & 7)) & 1:
                t_new = f(t + dt)
                out.append((x[0], x[1], x[2], dt, dt if mutant == "delta1_is_dt" else f(t_new - last)))
                t = last = t_new
                continue
            ts = []
            for a in range(3):
                s = f(1) if mutant == "skip_ignores_sign" else f(math.copysign(1.0, float(d[a])))
                ts.append(f(f(f(f(f(f(n[a]) + f(0.5)) + f(0.5) * s) * rH * f(2) - f(1)) * mb - x[a]) * rd[a]))
            tt = f(t + np.fmax(f(0), np.fmin(ts[0], np.fmin(ts[1], ts[2]))))
            while True:
                t = f(t + step(t))
                if mutant == "skip_one_step_less":
                    if not f(t + step(t)) < tt:
                        break
                elif not t < tt:
                    break
            if mutant == "skip_one_step_more":
                t = f(t + step(t))
    return out


def _start32(cfg, t, noise, mutant=None):
    f = np.float32
    dt_min = f(2) * f(SQRT3) / f(cfg["max_steps"])
    dt_max = f(2) * f(SQRT3) * f(1 << (cfg["C"] - 1)) / f(cfg["H"])
    with np.errstate(all="ignore"):
        first = dt_min if mutant == "noise_scales_dt_min" else min(dt_max, max(dt_min, f(t) * f(cfg["dt_gamma"])))
        return f(f(t) + first * f(noise))


def walker_train(inp, mutant=None):
    """march_rays_train by the fp32 walker: xyzs, dirs, deltas [M, .], rays [N,3], counter [2], slots in ray order."""
    cfg = _cfg(inp)
    N, M = len(inp["o"]), int(inp["M"])
    xyzs, dirs, deltas = np.zeros((M, 3), np.float32), np.zeros((M, 3), np.float32), np.zeros((M, 2), np.float32)
    rays = np.zeros((N, 3), np.int32)
    total = int(np.asarray(inp.get("counter0", (0, 0)))[0])
    base = total
    for r in range(N):
        s = _march32(cfg, inp["o"][r], inp["d"][r], _start32(cfg, inp["near"][r], inp["noise"][r], mutant), inp["far"][r], cfg["max_steps"], mutant)
        rays[r] = (r, total, len(s))
        if s and total + len(s) <= M:
            a = np.array(s, np.float32)
            xyzs[total:total + len(s)], deltas[total:total + len(s)], dirs[total:total + len(s)] = a[:, :3], a[:, 3:], inp["d"][r]
        total += len(s)
    return xyzs, dirs, deltas, rays, np.array([total, int(np.asarray(inp.get("counter0", (0, 0)))[1]) + N], np.int32)


def walker_burst(inp, mutant=None):
    """march_rays by the fp32 walker: xyzs, dirs, deltas [n_alive * n_step, .]."""
    cfg = _cfg(inp)
    alive, n_step = inp["rays_alive"], inp["n_step"]
    n = len(alive)
    xyzs, dirs, deltas = np.zeros((n, n_step, 3), np.float32), np.zeros((n, n_step, 3), np.float32), np.zeros((n, n_step, 2), np.float32)
    b = np.float32(cfg["bound"])
    for r in range(n):
        i = int(alive[r])
        if i < 0:
            continue
        s = _march32(cfg, inp["o"][i], inp["d"][i], _start32(cfg, inp["rays_t"][i], inp["noise"][r], mutant), inp["far"][i], n_step, mutant)
        if s:
            a = np.array(s, np.float32)
            x = a[:, :3]
            if inp.get("normalised"):
                x = ((x + b) * (np.float32(1) / (np.float32(2) * b))).astype(np.float32)
            xyzs[r, :len(s)], deltas[r, :len(s)], dirs[r, :len(s)] = x, a[:, 3:], inp["d"][i]
            if mutant == "burst_keeps_stale_slot" and len(s) < n_step:
                xyzs[r, len(s)], dirs[r, len(s)] = x[-1], inp["d"][i]
    return xyzs.reshape(-1, 3), dirs.reshape(-1, 3), deltas.reshape(-1, 2)
