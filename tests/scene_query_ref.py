"""Numpy statement of the scene point query (csrc/mesh.hip: foc_points_cull, foc_surface_frame, foc_scene_select; focnerf_amd/query.py).

Point cull. The lattice cull of mesh_ref.lattice_cull for a list: point i in place of lattice point i. With a placement the point is mapped
by mesh_ref.to_object (fp32, the kernel's order) and is empty outside the object's box — every comparison with a NaN fails, so a NaN
coordinate is never inside; with a bitfield the cell (fixed_cull_ref.cell_index) of a point STILL IN QUESTION must be set. Bit i % 64 of
mask[i // 64], offsets = exclusive prefix sum of the words' popcounts, the compact lists in list order: pos = the point in the object's
frame, xn = (pos + bound) / (2 bound) in fp32, one addition and one division.

Select. At every set point v = fp32(gain * sigma_c[slot]); v > best_sigma (strict: a tie keeps the earlier object, a NaN v never wins)
takes the point: best_sigma = v, best_id = k, best_rgb / best_normal = the slot's rows. Unset points are not touched. MUTANTS are
deliberately wrong variants the tests must tell apart.

Surface frame, float64 with a bound per component counted from the kernel's fp32 operations, the way normal_ref counts its normalise
and rotate stages (U = 2^-24; C = 2: first order, and an adder that truncates):
    n_obj    from an exact g: u = g / m (1 rounding), the sum of squares (a product and two fmaf: 3), sqrt (1), the division (1), and what
             the rounded u carry into the length (1): 7 roundings of values of magnitude at most 1 -> C U 7 absolute.
    normal   R n_obj, per row a product and two fmaf: sum_j |R_ij| bound(n_obj) carried + C U 3 sum_j |R_ij n_j|.
    dirs     NORMAL: -n_obj, exact: bound(n_obj). EYE: d = pos - eye, one rounding per component (U |d_d| carried, C U |d_d| counted), then
             the same normalise of the rounded d: by normal_ref's Jacobian argument 2 max_d bound(d_d) / |d| + C U 7.
The decisions are the kernel's, taken on fp32 values: n = 0 where max |g_d| is 0 or a component is not finite; the fallback direction
(0, 0, -1) where n_obj = 0 (NORMAL) or where the fp32 difference pos - eye is zero or not finite (EYE).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402
import fixed_cull_ref                                                    # noqa: E402
from fixed_tail_ref import U                                             # noqa: E402
from ragged_ref import C as CC                                           # noqa: E402

MUTANTS = ("ge", "nan_wins", "gain_after")
N_NORMALISE = 7                                                          # roundings of the normalise stage (see above)
FALLBACK = np.array([0.0, 0.0, -1.0])


# ---------------------------------------------------------------- point cull
def pack(keep):
    """bool [M] -> (mask uint64 [R], offsets uint32 [R + 1]), R = ceil(M / 64)."""
    keep = np.asarray(keep, dtype=bool)
    R = -(-len(keep) // 64)
    rows = np.zeros(R * 64, dtype=bool)
    rows[:len(keep)] = keep
    rows = rows.reshape(R, 64)
    mask = (rows.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(rows.sum(-1))]).astype(np.uint32)
    return mask, offsets


def unpack(mask, n):
    m = np.asarray(mask).view(np.uint64)
    return ((m[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:n]


def points_cull(points, w2o=None, obj_aabb=None, bound=None, bitfield=None, cascade=None, H=None):
    """points fp32 [M,3] -> (mask, offsets, pos fp32 [m,3], xn fp32 [m,3] or None without a bound)."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    keep = np.ones(len(p), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if w2o is not None:
            p = mesh_ref.to_object(w2o, p)
            box = np.asarray(obj_aabb, dtype=np.float32)
            keep &= ((p >= box[:3]) & (p <= box[3:])).all(-1)            # False for a NaN
        if bitfield is not None:
            idx = np.nonzero(keep)[0]                                    # the bitfield is read for the points still in question only
            index, _, _ = fixed_cull_ref.cell_index(p[idx], bound, cascade, H)
            index = np.minimum(index, cascade * H ** 3 - 1)
            keep[idx] = fixed_cull_ref.occupied(index, bitfield)
        mask, offsets = pack(keep)
        pos = p[keep]
        xn = None
        if bound is not None:
            b = np.float32(bound)
            xn = ((pos + b).astype(np.float32) / (np.float32(2) * b)).astype(np.float32)
    return mask, offsets, pos, xn


# ---------------------------------------------------------------- select
def scene_select(sigma_c, rgb_c, normal_c, keep, gain, k, best_sigma, best_id, best_rgb=None, best_normal=None, mutant=None):
    """One foc_scene_select call on copies of the best_* arrays: keep bool [n] (the mask's bits), the compact rows in list order.
    -> (best_sigma, best_id, best_rgb, best_normal)."""
    keep = np.asarray(keep, dtype=bool)
    bs, bi = np.array(best_sigma, dtype=np.float32), np.array(best_id, dtype=np.int32)
    br = None if best_rgb is None else np.array(best_rgb, dtype=np.float32)
    bn = None if best_normal is None else np.array(best_normal, dtype=np.float32)
    idx = np.nonzero(keep)[0]
    s = np.asarray(sigma_c, dtype=np.float32)[:len(idx)]
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.float32(gain) * s).astype(np.float32)
        if mutant == "gain_after":
            win = s > bs[idx]
        elif mutant == "ge":
            win = v >= bs[idx]
        else:
            win = v > bs[idx]
        if mutant == "nan_wins":
            win = win | np.isnan(v)
    at = idx[win]
    bs[at], bi[at] = v[win], k
    if br is not None:
        br[at] = np.asarray(rgb_c, dtype=np.float32).reshape(-1, 3)[:len(idx)][win]
    if bn is not None:
        bn[at] = np.asarray(normal_c, dtype=np.float32).reshape(-1, 3)[:len(idx)][win]
    return bs, bi, br, bn


def select_case():
    """Three objects over 130 points: exact ties, NaN, +-0, +inf candidates, a gain that rounds, points no object sets (pre-filled with a
    bit pattern). -> (n, keeps [3] bool [n], sigma [3] fp32 [n], gains [3], rgbs [3] [m_k,3], normals [3] [m_k,3], (best_sigma, best_id,
    best_rgb, best_normal) to start from)."""
    rng = np.random.default_rng(3)
    n = 130
    keeps = [rng.random(n) < 0.7 for _ in range(3)]
    for k in keeps:
        k[:12] = True
        k[64:67] = False                                                 # nobody sets these
    sig = [rng.random(n).astype(np.float32) * 4 for _ in range(3)]
    sig[1][0] = sig[0][0] * np.float32(2)                                # with gains (1, 0.5, ...): an exact tie at point 0 -> object 0 stays
    sig[1][1] = np.nan                                                   # a NaN candidate
    sig[2][1] = np.nan
    sig[0][2], sig[1][2], sig[2][2] = 0.0, -0.0, 0.0                     # +-0 against the initial 0: nobody wins
    sig[1][3] = np.inf
    sig[2][3] = np.inf                                                   # inf ties inf: object 1 stays
    sig[0][4], sig[1][4], sig[2][4] = 1.0, 3.0, 2.0                      # gained 1, 1.5, 0.6: object 1; a compare before the gain lets 2 > 1.5 in
    sig[2][5] = np.float32(1.0000001)                                    # a gain that rounds: fp32(0.3 * s) ties object 0 exactly
    sig[0][5], sig[1][5] = np.float32(0.3) * sig[2][5], 0.0
    gains = [np.float32(1.0), np.float32(0.5), np.float32(0.3)]
    prng = np.random.default_rng(9)
    rgbs, nrms = [], []
    for k in range(3):
        m = int(keeps[k].sum())
        rgbs.append(prng.random((m, 3)).astype(np.float32))
        nrms.append(prng.standard_normal((m, 3)).astype(np.float32))
    none = ~(keeps[0] | keeps[1] | keeps[2])
    bs, bi = np.zeros(n, np.float32), np.full(n, -1, np.int32)
    br, bn = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    bs.view(np.uint32)[none] = 0xDEADBEEF                                # what no call may touch
    bi.view(np.uint32)[none] = 0x5A5A5A5A
    br.view(np.uint32)[none] = 0x7FC12345
    bn.view(np.uint32)[none] = 0xFFFFFFFF
    return n, keeps, sig, gains, rgbs, nrms, (bs, bi, br, bn)


def run_select(mutant=None, payload=(True, True), calls=3):
    """The three successive calls of `select_case` -> (best_sigma, best_id, best_rgb, best_normal); payload: which of rgb / normal travel."""
    n, keeps, sig, gains, rgbs, nrms, (bs, bi, br, bn) = select_case()
    br, bn = (br if payload[0] else None), (bn if payload[1] else None)
    for k in range(calls):
        bs, bi, br, bn = scene_select(sig[k][keeps[k]], rgbs[k], nrms[k], keeps[k], gains[k], k, bs, bi, br, bn, mutant=mutant)
    return bs, bi, br, bn


# ---------------------------------------------------------------- surface frame
def _unit(g32):
    """(-g / |g| float64 [m,3], ok bool [m]) of fp32 rows g32: ok where the largest component is > 0 and every component finite."""
    g32 = np.asarray(g32, dtype=np.float32).reshape(-1, 3)
    g = g32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(np.abs(g), axis=-1, keepdims=True)
        ok = np.isfinite(g).all(axis=-1, keepdims=True) & (m > 0)
        u = g / np.where(ok, m, 1.0)
        n = -u / np.where(ok, np.sqrt((u * u).sum(axis=-1, keepdims=True)), 1.0)
    return np.where(ok, n, 0.0), ok[:, 0]


def surface_frame(grad_raw_c, pos_c=None, rot9=None, eye_obj=None, grad_bound=0.0):
    """-> dict(normal, normal_bound, dirs, dirs_bound), float64 [m,3] each. rot9 / eye_obj: the fp32 values the kernel was given (exact
    inputs). grad_bound [m,3] or a scalar: what the gradient itself is known to (0: exact), carried into n by normal_ref's Jacobian
    argument, 2 max_d bound / |g| (inf where that exceeds 1: a gradient that is all rounding)."""
    n, ok = _unit(grad_raw_c)
    g = np.asarray(grad_raw_c, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    bg = np.max(np.broadcast_to(np.asarray(grad_bound, dtype=np.float64), g.shape), axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rel = np.where(bg == 0, 0.0, 2.0 * bg / np.sqrt((g * g).sum(axis=-1)))
    rel = np.where(np.isfinite(rel) & (rel <= 1.0), rel, np.inf)
    bn = np.where(ok, rel + CC * U * N_NORMALISE, np.where(bg == 0, 0.0, np.inf))[:, None] * np.ones(3)
    if rot9 is None:
        normal, normal_bound = n, bn
    else:
        R = np.asarray(rot9, dtype=np.float32).astype(np.float64).reshape(3, 3)
        normal = n @ R.T
        normal_bound = bn @ np.abs(R).T + CC * U * 3 * (np.abs(n) @ np.abs(R).T)
    if eye_obj is None:
        dirs = np.where(ok[:, None], -n, FALLBACK)
        dirs_bound = bn
    else:
        p32 = np.asarray(pos_c, dtype=np.float32).reshape(-1, 3)
        e32 = np.asarray(eye_obj, dtype=np.float32).reshape(3)
        with np.errstate(invalid="ignore", over="ignore"):
            d32 = (p32 - e32).astype(np.float32)                         # the decision is taken on the kernel's own difference
        d = p32.astype(np.float64) - e32.astype(np.float64)
        _, dok = _unit(d32)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            length = np.sqrt((d * d).sum(axis=-1))
            exact = _neg_unit64(d)
            rel_d = 2.0 * np.max(CC * U * np.abs(d), axis=-1) / length
        dirs = np.where(dok[:, None], exact, FALLBACK)
        dirs_bound = np.where(dok, rel_d + CC * U * N_NORMALISE, 0.0)[:, None] * np.ones(3)
    return dict(normal=normal, normal_bound=normal_bound, dirs=dirs, dirs_bound=dirs_bound)


def _neg_unit64(d):
    """d / |d| in float64, scaled by the largest component first; rows that are zero or not finite come out as they may (masked by the caller)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.max(np.abs(d), axis=-1, keepdims=True)
        u = d / m
        return u / np.sqrt((u * u).sum(axis=-1, keepdims=True))
