"""Float64 reference of the hash-grid encoder's forward, its dy_dx and the total-variation gradient (csrc/ge_common.h: ge_forward_one,
ge_forward_hash3, k_grid_fwd_lbc / _bl / _pl, csrc/gridencoder.hip k_grid_fwd_counted, k_grad_tv), a bound per element, the cases, and a
numpy fp32 / fp16 model of the arithmetic with deliberately wrong variants (MUTANTS). Definition: gridencoder.cu:87-245 and :506-610 of
the reference, restated here from the formulas (`index()` is get_grid_index, :66-84); nothing below calls oracle.grid_encode_forward.

    out[l, b, c]      = sum over the 2^D corners k of the cell:  w_k(b, l) * table[off_l + row_k, c]
    dy_dx[b, l, d, c] = scale_l * f'(frac_d) * sum over the 2^(D-1) corners k of the other axes:  w_k^(-d) * (table[right] - table[left])
    grad_tv[off_l + row, c] += sum over the in-range points whose cell has that row:  (weight / 2D) * R_c / sqrt(Q_c + 1e-9)
        R the sum, Q the sum of squares, of centre - neighbour over the existing neighbours of the cell: the right one along axis d exists
        if cell_d < resolution, the left one if cell_d > 0.
A point with a coordinate outside [0, 1] gives exact zeros in out and dy_dx and adds nothing to grad_tv.

Operands
--------
The position is the kernels' own: pos32 = fmaf(x, scale32, align_corners ? 0 : 0.5) (grid_backward_ref._fma32: exact, no double rounding),
cell = floor(pos32), frac = pos32 - cell, which is exact in fp32. The reference is taken AT that fp32 fraction: an exact operand of
magnitude 0 (grid_backward_ref carries |pos| instead, about 1e-4 per weight at level 15, which would hide every forward error below that;
here the fp32 forward is bounded at a few 1e-7). That pos32 is the correctly rounded float64 position is a CPU assertion of its own
(test_grid_forward_ref.py). scale32 and the resolution come from oracle.grid_level_params; against the float64 2^(l S) H - 1 the scale
may differ by the three fp32 roundings of exp2f((float)l * S) * H - 1 (`scale_allowance()`), and resolution == ceil(scale32) + 1. Table
values, half or fp32, are exact operands. k_grad_tv reads the positions in the table's type; a half position converts to float exactly.

Bound
-----
grid_backward_ref's magnitude rules: an exact operand carries 0; one rounding of a result r carries |r|; a sum or difference carries its
operands' magnitudes plus |result|; a product a b carries mag(a)|b| + |a|mag(b) + |a b| (`_mul`). U = 2^-24, C = 2, K = 16: an fp32
chain ending in a reduction over T terms is within C U (T + K) mag, plus (T + K) 2^-126 (TINY) for products that underflow.
h = 2^-11, q = 2^-25: rounding v to half costs at most h|v| + q, so subnormal halves must come through unflushed.
  weights  1 - f carries |1 - f|; smoothstep v v fma(-2, v, 3): the fma one rounding, the two products by the rule; the D-fold product in
           the kernels' order (w = 1; w *= u_d for d = 0 ..), first factor exact.
  forward  E = C U (2^D + K) sum_k (mag(w_k)|v_k| + |w_k v_k|) + (2^D + K) TINY.
  dy_dx    terms (w (vr - vl)) f' with w starting at scale32 (exact), vr - vl one rounding, f' = 6 v (1 - v) by the rules (1 for the linear
           interpolation, exact), a chain of T = 2^(D-1) terms: C U (T + K) sum (mag(p)|f'| + |p|mag(f') + |p f'|) + (T + K) TINY.
  half     outputs add h (|ref| + E) + q.
  zeros    an element none of whose products is nonzero has bound 0 and must be exactly 0.
  grad_tv  per addend a = (w R) r: w = weight / (float)(2 D) carries |w| (one division); every centre - neighbour one rounding; R the
           running sum and Q the running fma over at most 2 D neighbours, by the rules; s = Q + 1e-9f (the fp32 constant, an exact operand);
           ASSUMED: sqrtf and the fp32 division are within 2 ulp each (the build keeps -fhip-fp32-correctly-rounded-divide-sqrt, under
           which both are correctly rounded: 1), so sqrt carries mag(s) / (2 sqrt s) + 2 sqrt s and r = 1 / sqrt s carries mag(sqrt) / s + 2 r;
           the two products by the rule: m_a. The n addends of one element meet in atomics, bounded as route (f) of grid_backward_ref:
           fp32 tables C U (n + K) (sum m_a + sum |a|) + (n + K) TINY; half tables per addend f = C U K m_a and its half rounding
           hb = h (|a| + f) + q, and each of the n packed half atomics rounds the running sum: sum f + sum hb + n (h E + q), E = sum (|a| + f + hb).
           An element whose addends are all exactly 0 (a constant table: every difference 0) has bound 0.

A cell never equals the resolution on a point of [0, 1]^D: pos32 <= round(scale32 + 0.5) < ceil(scale32) + 1 = resolution, and with
align_corners pos32 <= scale32. The right-neighbour test of grad_tv is therefore true on every input a kernel can see, and a stencil that
tests `cur <= resolution` computes the same as one that tests `cur <`: that mutant is told apart only on `tv_face`, a CPU-only case that
hands the stencil its cells directly (cell == resolution on one face), as the definition above is stated on cells.

`model()` / `tv_model()` restate the kernels' fp32 arithmetic in numpy (fmaf through _fma32, the corner order, half rounding of the
result, sequential atomics in point order); a reference value is never computed with a mutant.
"""
import numpy as np

import oracle
from fixed_tail_ref import U
from grid_backward_ref import H16, M32, PRIMES, Q16, _axis_weights, _fma32, _mul, _seq_add, _weights, level, level_offsets, make_case
from ragged_ref import C as CC, K as KK, TINY

F32 = np.float32
EPS_TV = float(F32(1e-9))

MUTANTS = ("drop_corner", "half_accumulation", "no_half_offset", "ac_stride_plus_one", "smooth_deriv_6v", "smooth_deriv_linear",
           "primes_swapped", "dense_index_on_hashed", "subnormal_flush", "dy_without_scale", "tv_right_le", "tv_weight_over_d", "tv_no_eps")

# D, C, L, H, log2_hashmap_size, finest resolution, gridtype, align_corners, interpolation (, B)
SPECS = {
    # every row of CASES in tests/test_gpu_gridencoder.py (test_grid_forward_ref.py asserts that none is missing)
    "foc19": (3, 2, 16, 16, 19, 2048, 0, False, 0),
    "foc19_bound2": (3, 2, 16, 16, 19, 4096, 0, False, 0),
    "D3_C1": (3, 1, 8, 16, 15, 512, 0, False, 0),
    "D3_C4_tiled": (3, 4, 8, 16, 15, 512, 1, False, 0),
    "D3_C8_ac_smooth": (3, 8, 4, 8, 14, 128, 0, True, 1),
    "D2_smooth": (2, 2, 12, 16, 17, 2048, 0, False, 1),
    "D4": (4, 2, 8, 8, 14, 64, 0, False, 0),
    "D4_tiled_ac_smooth": (4, 4, 5, 4, 12, 20, 1, True, 1),
    "D5": (5, 2, 6, 4, 13, 24, 0, False, 0),
    "D5_C1_smooth": (5, 1, 4, 4, 12, 12, 0, False, 1),
    "D4_L9": (4, 2, 9, 4, 12, 32, 0, False, 0, 257),
    "D5_L9": (5, 2, 9, 4, 12, 32, 0, False, 0, 257),
    # and
    "D2_tiled_ac": (2, 2, 6, 16, 12, 256, 1, True, 0),
    "D3_C1_smooth": (3, 1, 4, 8, 12, 64, 0, False, 1),
    "D3_C4_smooth": (3, 4, 4, 8, 12, 64, 0, False, 1),
    "D3_C8_smooth": (3, 8, 4, 8, 12, 64, 0, False, 1),
    # level sizes 216 (27 eights), 1728, 13824, 2^14; the scales are whole numbers (5, 11, 23, 47), so x = 1 has a corner at cell == resolution
    # whose dense index lies beyond the level: rows taken `% size` where the size is no power of two
    "mod_tiled_ac": (3, 2, 4, 6, 14, 48, 1, True, 0),
    "focs": (3, 2, 16, 16, 15, 2048, 0, False, 0),              # FOC's grid with 2^15-row levels: dense, hashed, eight levels in the shared workgroup
}
TV_SPECS = {
    "tv_D2_hash": (2, 2, 6, 16, 12, 256, 0, False, 0),
    "tv_D2_tiled_ac": (2, 2, 6, 16, 12, 256, 1, True, 0),
    "tv_D3_hash_ac": (3, 2, 6, 8, 13, 128, 0, True, 0),
    "tv_D3_tiled": (3, 4, 6, 8, 13, 128, 1, False, 0),
    "tv_D4_hash_L9": (4, 2, 9, 4, 12, 32, 0, False, 0),
    "tv_D4_tiled_ac": (4, 4, 5, 4, 12, 20, 1, True, 0),
    "tv_D5_hash_L9": (5, 2, 9, 4, 12, 32, 0, False, 0),
    "tv_D5_C1_tiled_ac": (5, 1, 4, 4, 12, 12, 1, True, 0),
}
BATCHES = (1, 255, 256, 257, 513)
FUSE_SMALL_RES = 160                                           # csrc/ge_common.h ge_small_levels: the default threshold of FOC_GRID_FUSE_SMALL
TV_WEIGHT = 0.25


# ---------------------------------------------------------------- index, levels
def index(case, pg, size, res, primes=PRIMES, force_dense=False, r1=None, raw=False):
    """get_grid_index (gridencoder.cu:66-84) in uint32 arithmetic: pg [..., D] grid positions -> row (`raw`: before `% size`)."""
    D = case["D"]
    pg = pg.astype(np.uint64) & np.uint64(M32)
    r1 = (res if case["ac"] else res + 1) if r1 is None else r1
    stride, idx = 1, np.zeros(pg.shape[:-1], np.uint64)
    for d in range(D):
        if stride <= size:
            idx = (idx + pg[..., d] * np.uint64(stride)) & np.uint64(M32)
            stride = (stride * r1) & M32
    if case["gridtype"] == 0 and stride > size and not force_dense:
        idx = np.zeros(pg.shape[:-1], np.uint64)
        for d in range(D):
            idx ^= (pg[..., d] * np.uint64(primes[d])) & np.uint64(M32)
    return (idx if raw else idx % np.uint64(size)).astype(np.int64)


def corners(cell, D):
    """[n, 2^D, D]: bit d of the corner index set = +1 along axis d."""
    k = np.arange(1 << D)
    return cell[:, None, :] + ((k[:, None] >> np.arange(D)[None]) & 1)[None]


def flevel(case, l):
    """grid_backward_ref.level() with the fp32 fraction as an exact operand: frac64 = frac32, magnitude 0."""
    lv = level(case, l)
    if "fwd" not in lv:
        lv["fwd"] = dict(lv, frac64=lv["frac32"].astype(np.float64), mpos=np.zeros(lv["frac32"].shape))
    return lv["fwd"]


def scale64(case, l):
    return 2.0 ** (l * case["S"]) * case["H"] - 1.0


def scale_allowance(case, l):
    """|scale32 - (2^(l S) H - 1)| allowed by the three fp32 roundings of exp2f((float)l * S) * H - 1 (S the fp32 value the library is
    handed): the product l S rounds once, U |l S|, which the exponential turns into a relative ln 2 U |l S|; exp2f itself is taken as
    within 2 ulp (libm's is within 1), the product with H rounds once and so does the difference: (ln 2 |l S| + 2 + 1) U e H + U |scale|."""
    S32 = float(F32(case["S"]))
    e = 2.0 ** (l * S32) * case["H"]
    drift = abs(2.0 ** (l * S32) - 2.0 ** (l * case["S"])) * case["H"]          # S itself handed over as fp32
    return (np.log(2.0) * abs(l * S32) + 3.0) * U * e * (1 + 4 * U) + U * abs(e - 1.0) + drift


def small_levels(case, fuse_small=1):
    """ge_small_levels: the leading levels one workgroup per chunk encodes (0: plain walk), from the option's value."""
    if not fuse_small:
        return 0
    finest = fuse_small if fuse_small > 1 else FUSE_SMALL_RES
    lc = 0
    while lc < case["L"] // 2 and level(case, lc)["res"] <= finest:
        lc += 1
    return lc if lc >= 2 else 0


def forms(case, half, dy, out_bl, pairs=1, fast=1, fuse_small=1, table_aligned=True, index_path=None):
    """The launch a forward call takes and the per-level arithmetic inside it, restated from ge_forward_launch / ge_pairs_mode /
    ge_forward_level: (kernel, shared levels, [per level 'hash3' | 'pairs' | 'one']). index_path(size, res, off) is the library's
    foc_grid_forward_index_path where it is at hand, else its restatement here."""
    D, C, L = case["D"], case["C"], case["L"]
    if D >= 4:
        return "k_grid_fwd_pl", 0, ["one"] * L
    if out_bl:
        return "k_grid_fwd_bl", 0, ["one"] * L
    mode = 0 if (not pairs or not table_aligned or dy) else (2 if fast and half and D == 3 and C == 2 and case["gridtype"] == 0 and not case["ac"] and case["interp"] == 0 else 1)
    per = []
    for l in range(L):
        lv = level(case, l)
        off = int(case["off"][l])
        if not (half and D == 3 and C == 2) or ((off | lv["size"]) & 1) or not mode:
            per.append("one")
            continue
        if index_path is None:
            admits = (not lv["hashed"] or lv["pow2"]) and lv["size"] <= 1 << 30
        else:
            admits = index_path(lv["size"], lv["res"], off) != 0
        per.append("hash3" if mode == 2 and admits else "pairs")
    return "k_grid_fwd_lbc", small_levels(case, fuse_small), per


# ---------------------------------------------------------------- float64 reference and bound
def forward64(case, table, fp32_fraction=False):
    """float64 forward out [L, B, C] and dy_dx [B, L, D, C] of `table` [rows, C] (out-of-range points: zeros), without a bound; at the
    float64 position, or at the kernels' fp32 fraction."""
    D, C, L, B = case["D"], case["C"], case["L"], case["B"]
    out, dy = np.zeros((L, B, C)), np.zeros((B, L, D, C))
    k = np.arange(1 << D)
    for l in range(L):
        lv = flevel(case, l) if fp32_fraction else level(case, l)
        u, _, du = _axis_weights(case, lv)
        w, _ = _weights(case, lv)
        vals = table[lv["rows"] + int(case["off"][l])].astype(np.float64)          # [n, K, C]
        out[l, lv["idx"]] = (w[:, :, None] * vals).sum(axis=1)
        for d in range(D):
            wd = np.ones_like(w)
            for dd in range(D):
                if dd != d:
                    wd = wd * u[:, dd, :][:, (k >> dd) & 1]
            sign = np.where((k >> d) & 1, 1.0, -1.0)[None]
            dy[lv["idx"], l, d] = lv["scale"] * du[:, d:d + 1] * ((wd * sign)[:, :, None] * vals).sum(axis=1)
    return out, dy


def reference(case, table):
    """dict(out, out_b [L, B, C], dy, dy_b [B, L, D, C]) float64: the forward of `table` (float16 or float32: also the outputs' type) at the
    fp32 fraction, and the docstring's bound on |kernel - reference| per element."""
    key = ("fwd", id(table))
    if key in case["_bound"]:
        return case["_bound"][key]
    half = table.dtype == np.float16
    D, C, L, B = case["D"], case["C"], case["L"], case["B"]
    out, ob, dy, db = np.zeros((L, B, C)), np.zeros((L, B, C)), np.zeros((B, L, D, C)), np.zeros((B, L, D, C))
    K, T = 1 << D, 1 << (D - 1)
    kk = np.arange(T)

    def close(val, mag, terms, nz):
        e = CC * U * (terms + KK) * mag + (terms + KK) * TINY
        if half:
            e = e + H16 * (np.abs(val) + e) + Q16
        return np.where(nz, e, 0.0)

    for l in range(L):
        lv = flevel(case, l)
        if lv["idx"].size == 0:
            continue
        vals = table[lv["rows"] + int(case["off"][l])].astype(np.float64)          # [n, K, C]
        w, mw = _weights(case, lv)
        prod = w[:, :, None] * vals
        o = prod.sum(axis=1)
        out[l, lv["idx"]] = o
        ob[l, lv["idx"]] = close(o, (mw[:, :, None] * np.abs(vals) + np.abs(prod)).sum(axis=1), K, (prod != 0).any(axis=1))
        u, mu, du = _axis_weights(case, lv)
        mdu = np.zeros_like(du)
        if case["interp"] == 1:
            v = lv["frac64"]
            du, mdu = _mul(6.0 * v, np.abs(6.0 * v), 1.0 - v, np.abs(1.0 - v))
        for d in range(D):
            wd, mwd = np.full((lv["idx"].size, T), float(lv["scale"])), np.zeros((lv["idx"].size, T))
            for j, dd in enumerate([a for a in range(D) if a != d]):
                bit = (kk >> j) & 1
                wd, mwd = _mul(wd, mwd, u[:, dd, :][:, bit], mu[:, dd, :][:, bit])
            left = (kk & ((1 << d) - 1)) | ((kk >> d) << (d + 1))
            diff = vals[:, left | (1 << d)] - vals[:, left]                        # [n, T, C]
            p, mp = _mul(wd[:, :, None], mwd[:, :, None], diff, np.abs(diff))
            t, mt = _mul(p, mp, du[:, d, None, None], mdu[:, d, None, None])
            g = t.sum(axis=1)
            dy[lv["idx"], l, d] = g
            db[lv["idx"], l, d] = close(g, mt.sum(axis=1), T, (t != 0).any(axis=1))
    case["_bound"][key] = dict(out=out, out_b=ob, dy=dy, dy_b=db, table=table)      # keeps `table` alive: its id is the key
    return case["_bound"][key]


def tv_positions(case, half):
    """The case as k_grad_tv sees it: positions in the table's type (a half position converts to float exactly)."""
    if not half:
        return case
    key = "_tv16"
    if key not in case:
        case[key] = dict(case, x=case["x"].astype(np.float16).astype(np.float32), _lv={}, _bound={})
    return case[key]


def _tv_levels(case, cells=None):
    """Per level (lv, cell [n, D]); `cells`: a dict level -> cells handed to the stencil directly (the CPU-only case tv_face)."""
    for l in range(case["L"]):
        lv = level(case, l)
        yield l, lv, (lv["cell"] if cells is None or l not in cells else cells[l])


def _tv_neighbours(case, lv, cell, right_le=False):
    """For every axis and side: (exists [n], local rows of the neighbour [n]) in the kernel's order (right, then left, per axis)."""
    for d in range(case["D"]):
        cur = cell[:, d]
        for exists, step in (((cur <= lv["res"]) if right_le else (cur < lv["res"]), 1), (cur > 0, -1)):
            nb = cell.copy()
            nb[:, d] = np.where(exists, cur + step, cur)
            yield exists, index(case, nb, lv["size"], lv["res"])


def tv_reference(case, table, weight=TV_WEIGHT, cells=None, literal_half=False):
    """(grad_tv [rows, C] float64, bound [rows, C]) of one call on a zeroed gradient. literal_half: the bound of the REFERENCE's own
    arithmetic on half tables instead (kernel_grad_tv keeps w, the differences, R, Q and the addend in half, which oracle.c restates with a
    rounding to half after each; the addends of an element summed exactly and rounded once): the same rules with h in place of U and q
    per operation in place of TINY. k_grad_tv computes in fp32 and rounds each addend once; it is held to the tighter bound."""
    half = table.dtype == np.float16
    c = tv_positions(case, half)
    key = ("tv", id(table), weight, cells is None, literal_half)
    if key in c["_bound"]:
        return c["_bound"][key][:2]
    D, C = c["D"], c["C"]
    n_rows = int(c["off"][-1])
    w = float(F32(weight)) / (2 * D)
    mw = abs(w)
    ref, M, A, N, F, Hb, E = (np.zeros((n_rows, C)) for _ in range(7))
    for l, lv, cell in _tv_levels(c, cells):
        if lv["idx"].size == 0:
            continue
        o = int(c["off"][l])
        row = index(c, cell, lv["size"], lv["res"])
        centre = table[o + row].astype(np.float64)                                 # [n, C]
        R, mR, Q, mQ = (np.zeros_like(centre) for _ in range(4))
        for exists, rows_nb in _tv_neighbours(c, lv, cell):
            ex = exists[:, None]
            gv = np.where(ex, centre - table[o + rows_nb].astype(np.float64), 0.0)
            R = R + gv
            mR = np.where(ex, mR + np.abs(gv) + np.abs(R), mR)
            sq, msq = _mul(gv, np.abs(gv), gv, np.abs(gv))
            Q = Q + sq
            mQ = np.where(ex, mQ + msq + np.abs(Q), mQ)
        s = Q + EPS_TV
        ms = mQ + np.abs(s)
        root = np.sqrt(s)
        mroot = ms / (2 * root) + 2 * root
        r = 1.0 / root
        mr = mroot / s + 2 * r
        t1, mt1 = _mul(w, mw, R, mR)
        a, ma = _mul(t1, mt1, r, mr)
        f = CC * (H16 if literal_half else U) * KK * ma + (KK * Q16 if literal_half else 0.0)
        hb = H16 * (np.abs(a) + f) + Q16
        for c_ in range(C):
            for tgt, v in ((ref, a), (M, ma), (A, np.abs(a)), (N, np.ones_like(a)), (F, f), (Hb, hb), (E, np.abs(a) + f + hb)):
                tgt[:, c_] += np.bincount(o + row, weights=v[:, c_], minlength=n_rows)
    if literal_half:
        assert half
        b = F + H16 * (np.abs(ref) + F) + Q16
    elif half:
        b = F + Hb + N * (H16 * E + Q16)
    else:
        b = CC * U * (N + KK) * (M + A) + (N + KK) * TINY
    b = np.where(M + A > 0, b, 0.0)
    c["_bound"][key] = (ref, b, table)
    return ref, b


# ---------------------------------------------------------------- numpy fp32 / fp16 model
def fma32(a, b, c):
    """fmaf on float32 arrays."""
    a, b, c = np.broadcast_arrays(a, b, c)
    return _fma32(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, np.float64), np.ascontiguousarray(c, np.float64))[0]


def _flush16(v):
    return np.where(np.abs(v.astype(np.float32)) < 2.0 ** -14, np.float16(0), v)


def model(case, table, mutant=None):
    """(out [L, B, C], dy_dx [B, L, D, C]) in the table's type as the forward kernels compute them."""
    assert mutant is None or mutant in MUTANTS
    half = table.dtype == np.float16
    D, C, L, B = case["D"], case["C"], case["L"], case["B"]
    out, dy = np.zeros((L, B, C), table.dtype), np.zeros((B, L, D, C), table.dtype)
    K, T = 1 << D, 1 << (D - 1)
    x = case["x"]
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    idx = np.nonzero(inside)[0]
    one = F32(1)

    def store(v):
        with np.errstate(over="ignore"):
            v = v.astype(table.dtype)
        return _flush16(v) if half and mutant == "subnormal_flush" else v

    for l in range(L):
        scale, res = oracle.grid_level_params(l, case["S"], case["H"])
        size, o = int(case["off"][l + 1] - case["off"][l]), int(case["off"][l])
        add = 0.0 if case["ac"] or mutant == "no_half_offset" else 0.5
        pos32, _ = _fma32(x[idx], scale, add)
        cellf = np.floor(pos32)
        f = (pos32 - cellf).astype(F32)
        cell = cellf.astype(np.int64)
        deriv = np.ones_like(f)
        if case["interp"] == 1:
            v = f
            deriv = {"smooth_deriv_6v": F32(6) * v, "smooth_deriv_linear": np.ones_like(v)}.get(mutant, F32(6) * v * (one - v))
            f = v * v * fma32(F32(-2), v, F32(3))
        kw = {}
        if mutant == "ac_stride_plus_one":
            kw["r1"] = res + 1
        if mutant == "primes_swapped":
            kw["primes"] = (PRIMES[0], PRIMES[2], PRIMES[1]) + PRIMES[3:]
        if mutant == "dense_index_on_hashed":
            kw["force_dense"] = True
        rows = index(case, corners(cell, D), size, res, **kw)                     # [n, K]
        vals = table[o + rows]
        if half and mutant == "subnormal_flush":
            vals = _flush16(vals)
        vals = vals.astype(F32)                                                    # [n, K, C]
        k = np.arange(K)
        w = np.ones((idx.size, K), F32)
        for d in range(D):
            w = w * np.where(((k >> d) & 1)[None] == 1, f[:, d:d + 1], one - f[:, d:d + 1])
        acc = np.zeros((idx.size, C), F32)
        for c_ in range(K):
            if mutant == "drop_corner" and c_ == K - 1:
                continue
            acc = fma32(w[:, c_:c_ + 1], vals[:, c_], acc)
            if half and mutant == "half_accumulation":
                acc = acc.astype(np.float16).astype(F32)
        out[l, idx] = store(acc)
        kk = np.arange(T)
        for d in range(D):
            wd = np.full((idx.size, T), one if mutant == "dy_without_scale" else F32(scale), F32)
            for j, dd in enumerate([a for a in range(D) if a != d]):
                wd = wd * np.where(((kk >> j) & 1)[None] == 1, f[:, dd:dd + 1], one - f[:, dd:dd + 1])
            left = (kk & ((1 << d) - 1)) | ((kk >> d) << (d + 1))
            rg = np.zeros((idx.size, C), F32)
            for t in range(T):
                p = wd[:, t:t + 1] * (vals[:, left[t] | (1 << d)] - vals[:, left[t]])
                rg = fma32(p, deriv[:, d:d + 1], rg)
            dy[idx, l, d] = store(rg)
    return out, dy


def tv_model(case, table, weight=TV_WEIGHT, mutant=None, cells=None):
    """grad_tv [rows, C] in the table's type as k_grad_tv leaves it on a zeroed gradient, atomics in point order."""
    assert mutant is None or mutant in MUTANTS
    half = table.dtype == np.float16
    c = tv_positions(case, half)
    D, C = c["D"], c["C"]
    n_rows = int(c["off"][-1])
    w = F32(weight) / F32(D if mutant == "tv_weight_over_d" else 2 * D)
    eps = F32(0) if mutant == "tv_no_eps" else F32(1e-9)
    elems, addends = [], []
    for l, lv, cell in _tv_levels(c, cells):
        if lv["idx"].size == 0:
            continue
        o = int(c["off"][l])
        row = index(c, cell, lv["size"], lv["res"])
        centre = table[o + row].astype(F32)
        R, Q = np.zeros_like(centre), np.zeros_like(centre)
        for exists, rows_nb in _tv_neighbours(c, lv, cell, right_le=mutant == "tv_right_le"):
            ex = exists[:, None]
            gv = np.where(ex, centre - table[o + rows_nb].astype(F32), F32(0))
            R = np.where(ex, R + gv, R)
            Q = np.where(ex, fma32(gv, gv, Q), Q)
        with np.errstate(divide="ignore", invalid="ignore"):
            a = (w * R * (F32(1) / np.sqrt(Q + eps))).astype(F32)
        elems.append(((o + row)[:, None] * C + np.arange(C)[None]).reshape(-1))
        addends.append(a.reshape(-1))
    elem, a = np.concatenate(elems), np.concatenate(addends)
    if half:
        a = a.astype(np.float16)
    return _seq_add(elem, a, np.float16 if half else F32, n_rows * C).reshape(n_rows, C)


# ---------------------------------------------------------------- cases
def _whole_position(case_probe, l, rng):
    """An x of (0, 1) whose pos32 at level l is a whole number k >= 1."""
    lv_scale, res = oracle.grid_level_params(l, case_probe["S"], case_probe["H"])
    add = 0.0 if case_probe["ac"] else 0.5
    for _ in range(64):
        k = int(rng.integers(1, max(2, int(lv_scale))))
        x = F32((k - add) / lv_scale)
        for cand in (x, np.nextafter(x, F32(1)), np.nextafter(x, F32(0))):
            if 0 < cand < 1 and _fma32(np.array([cand], F32), lv_scale, add)[0][0] == k:
                return cand
    raise AssertionError("no point on a cell boundary found")


def points(spec, B, seed=0):
    """B points of [0, 1]^D with, from B = 64 on, the deliberate ones (the docstring of test_grid_forward_ref.test_case_promises lists
    them); `special` names their rows."""
    D, L = spec[0], spec[2]
    rng = np.random.default_rng(7000 + 31 * B + D + seed)
    x = rng.random((B, D)).astype(F32)
    special = {}
    if B < 64:
        return x, special
    x[0], x[1], x[2], x[3] = 0.0, 1.0, F32(1) - F32(2.0 ** -24), -0.0
    x[4, 0] = -F32(2.0 ** -126)                       # just below 0
    x[5, D - 1] = np.nextafter(F32(1), F32(2))        # just above 1
    probe = make_case("probe", spec[:9], x[:1], np.zeros((L, 1, spec[1]), np.float16))
    whole = []
    for i, l in enumerate(sorted({0, L // 2, L - 1})):
        for j in range(2):
            r = 6 + 2 * i + j
            x[r, (i + j) % D] = _whole_position(probe, l, rng)
            whole.append((r, l, (i + j) % D))
    # ten points in one cell of the coarse levels (grad_tv's atomics meet there)
    x[20:30] = F32(0.3137) + (rng.random((10, D)) * 1e-3).astype(F32)
    special.update(zero=0, one=1, below_one=2, neg_zero=3, below_zero=4, above_one=5, whole=whole, cluster=np.arange(20, 30))
    return x, special


_TABLES = {}


def n_rows_of(spec):
    D, C, L, H, lh, desired, gridtype, ac = spec[:8]
    return int(level_offsets(D, L, np.exp2(np.log2(desired / H) / (L - 1)), H, lh, ac)[-1])


def table(sname, kind, half):
    """The table of a spec: 'uniform' in +-1, 'subnormal' (half subnormals), 'constant', 'cancel' (focs: +-1 by the parity of the vertex
    on the dense levels, slightly perturbed). float16 or float32 (the same values where they fit)."""
    key = (sname, kind, half)
    if key in _TABLES:
        return _TABLES[key]
    spec = {**SPECS, **TV_SPECS}[sname]
    n, C = n_rows_of(spec), spec[1]
    rng = np.random.default_rng(sum(map(ord, sname + kind)))
    if kind == "uniform":
        t = rng.random((n, C), np.float32) * 2 - 1
        t16 = t.astype(np.float16)
        t = t16 if half else t
    elif kind == "subnormal":
        t16 = (rng.integers(-1023, 1024, (n, C)) * 2.0 ** -24).astype(np.float16)
        t = t16 if half else t16.astype(np.float32)
    elif kind == "constant":
        t = np.full((n, C), 0.37, np.float16 if half else np.float32)
    else:
        assert kind == "cancel"
        t = (rng.random((n, C), np.float32) * 2 - 1)
        probe = make_case("probe", spec[:9], np.zeros((1, spec[0]), F32), np.zeros((spec[2], 1, C), np.float16))
        for l in range(spec[2]):
            lv = level(probe, l)
            if lv["hashed"]:
                continue
            r1 = lv["res"] + 1
            row = np.arange(lv["size"])
            parity = (row % r1 + (row // r1) % r1 + row // (r1 * r1)) & 1
            o = int(probe["off"][l])
            t[o:o + lv["size"]] = np.where(parity[:, None] == 1, -1.0, 1.0) * (1 + 2.0 ** -8 * t[o:o + lv["size"]])
        t16 = t.astype(np.float16)
        t = t16 if half else t16.astype(np.float32)
    _TABLES[key] = t
    return t


CANCEL_LEVEL = 1


def _build(name):
    if name == "tv_face":
        return _tv_face()
    sname, B, kind = PLAN[name]
    spec = {**SPECS, **TV_SPECS}[sname]
    D, C, L = spec[:3]
    x, special = points(spec, B)
    if kind == "cancel":
        # points next to the cell centres of a dense level: equal weights on +-1 neighbours
        probe = make_case("probe", spec[:9], x[:1], np.zeros((L, 1, C), np.float16))
        lv = level(probe, CANCEL_LEVEL)
        rng = np.random.default_rng(5)
        n = B - 64
        cells = rng.integers(0, lv["res"] - 1, (n, D))
        x[64:] = ((cells + 0.5 + (rng.random((n, D)) - 0.5) * 2e-3 - 0.5) / lv["scale"]).astype(F32)
        special["centred"] = np.arange(64, B)
    return make_case(name, spec[:9], x, np.zeros((L, B, C), np.float16), sname=sname, kind=kind, special=special)


def _tv_face():
    """CPU only: cells handed to the stencil directly, one face at cell == resolution (no position of [0, 1] gives that cell)."""
    spec = TV_SPECS["tv_D2_hash"]
    c = make_case("tv_face", spec, np.full((4, 2), 0.5, F32), np.zeros((spec[2], 4, spec[1]), np.float16), sname="tv_D2_hash", kind="uniform", special={})
    cells = {}
    for l in range(c["L"]):
        res = level(c, l)["res"]
        cells[l] = np.array([[res, 1], [1, res], [res, res], [0, 0]], np.int64)
    c["cells"] = cells
    return c


PLAN = {}
for _n, _s in SPECS.items():
    PLAN[_n] = (_n, _s[9] if len(_s) == 10 else 257, "uniform")
for _b in BATCHES:
    for _n in ("focs", "D2_smooth", "D4_tiled_ac_smooth"):
        PLAN[f"{_n}_B{_b}" if _b != 257 else _n] = (_n, _b, "uniform")
PLAN["focs_subnormal"] = ("focs", 257, "subnormal")
PLAN["focs_cancel"] = ("focs", 513, "cancel")
PLAN["D4_subnormal"] = ("D4", 257, "subnormal")
TV_PLAN = {n: (n, 257, "uniform") for n in TV_SPECS}
TV_PLAN["tv_D3_tiled_B513"] = ("tv_D3_tiled", 513, "uniform")
TV_PLAN["tv_D2_hash_B1"] = ("tv_D2_hash", 1, "uniform")
TV_PLAN["tv_D3_hash_ac_constant"] = ("tv_D3_hash_ac", 257, "constant")
PLAN.update(TV_PLAN)
_BUILT = {}


def case(name):
    """The case of that name, built once."""
    if name not in _BUILT:
        _BUILT[name] = _build(name)
    return _BUILT[name]


def case_table(name, half):
    c = case(name)
    return table(c["sname"], c["kind"], half)
