"""NOT a test module: the float64 statement of per-object attribution in the combined render (include/focnerf.h,
foc_combine_select_composite_attr), shared by tests/test_attribution_ref.py, tests/test_attribution_gloo.py and
tests/test_gpu_attribution.py. The CPU oracle has no attribution, so the reference lives here.

    winner       the id travelling with the rgb the strict-'>' select keeps (COMBINED.py:247-251): field 0's id to begin with, field k's
                 id exactly where `dens_k > running max` at k's turn; the first object keeps ties, a NaN density never takes the sample
                 and — torch.maximum's propagation — nothing takes it after a NaN either.
    w_i          alpha_i * prod_{j<i}(1 - alpha_j + 1e-15) on the sample positions oracle.composite_fixed_steps uses (float32 linspace in
                 symmetric halves, float32 z and deltas), alpha and the products in float64.
    obj_weights  [N, n_obj]  sum of w_i over the samples object k won;   obj_depth  the same sum of w_i * oz_i (oz = clamped (z-near)/span)
    instance     [N] int32   first index of the largest obj_weights entry, -1 when no entry is > 0 (NaN entries are never the largest)
"""
from collections import namedtuple

import numpy as np

Ref = namedtuple("Ref", "winner weights obj_weights obj_depth instance merged_sigma")


def fields(K, N, T, seed):
    """The generator of tests/test_gpu_combine.py (half the densities exactly 0, exact non-zero ties between objects 0 / 1 and 2 / K-1),
    with a third of the rays thinned by 0.01 so that weights do not all saturate, and a few rays with no density at all."""
    rng = np.random.default_rng(seed)
    dens = (rng.random((K, N, T)) ** 4 * 40).astype(np.float32)
    dens[rng.random((K, N, T)) < 0.5] = 0
    if K > 1:
        dens[1, :, :8] = dens[0, :, :8]
    if K > 3:
        dens[K - 1, :, 8:12] = dens[2, :, 8:12]
    dens[:, 1::3] *= np.float32(0.01)
    dens[:, 2::11] = 0                                  # rays 2, 13, 24, ...: empty
    rgb = rng.random((K, N, T, 3)).astype(np.float32)
    nears = (rng.random(N) * 0.5 + 0.2).astype(np.float32)
    fars = nears + (rng.random(N) * 2 + 0.5).astype(np.float32)
    return dens, rgb, nears, fars


def empty_rays(N):
    return np.arange(N) % 11 == 2


def winner(dens, ids=None):
    """dens [K,N,T] float32, ids: per field an int or a uint8 [N,T] plane (default: field k is object k) -> (winner uint8 [N,T], index of
    the field whose rgb survives [N,T], merged density [N,T] as torch.maximum leaves it)."""
    K = dens.shape[0]
    ids = list(range(K)) if ids is None else list(ids)
    plane = lambda v: np.broadcast_to(np.asarray(v, np.uint8), dens.shape[1:]).copy()
    m = dens[0].copy()
    win, src = plane(ids[0]), np.zeros(dens.shape[1:], np.int64)
    for k in range(1, K):
        with np.errstate(invalid="ignore"):
            take = dens[k] > m                          # False for a NaN on either side
        win = np.where(take, plane(ids[k]), win)
        src = np.where(take, k, src)
        m = np.where(np.isnan(dens[k]) | np.isnan(m), np.float32(np.nan), np.where(take, dens[k], m)).astype(np.float32)
    return win.astype(np.uint8), src, m


def sample_positions(nears, fars, T):
    """(deltas [N,T], oz [N,T]) in float32, operation for operation what oracle/oracle.c orc_composite_fixed_steps evaluates."""
    one = np.float32(1.0)
    step = one / np.float32(T - 1)
    i = np.arange(T)
    lin = np.where(i < T // 2, step * i.astype(np.float32), one - step * (T - 1 - i).astype(np.float32)).astype(np.float32)
    near, far = nears.astype(np.float32)[:, None], fars.astype(np.float32)[:, None]
    span = far - near
    z = (near + span * lin[None, :]).astype(np.float32)
    deltas = np.empty_like(z)
    deltas[:, :-1] = z[:, 1:] - z[:, :-1]
    deltas[:, -1:] = span / np.float32(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        oz = ((z - near) / span).astype(np.float32)
    oz = np.where(oz < 0, np.float32(0), np.where(oz > 1, one, oz)).astype(np.float32)
    return deltas, oz


def weights(sigma, nears, fars):
    """float64 w [N,T] of a merged density field [N,T]."""
    deltas, oz = sample_positions(nears, fars, sigma.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = 1.0 - np.exp(-deltas.astype(np.float64) * sigma.astype(np.float64))
        trans = np.cumprod(1.0 - alpha + 1e-15, axis=1)
    trans = np.concatenate([np.ones_like(trans[:, :1]), trans[:, :-1]], axis=1)
    return alpha * trans, oz.astype(np.float64)


def instance_of(obj_weights):
    """First index of the largest entry per row; -1 where no entry is > 0. NaN entries never count."""
    w = np.where(np.isnan(obj_weights), -np.inf, obj_weights)
    inst = np.argmax(w, axis=1).astype(np.int32)
    inst[~(w.max(axis=1) > 0)] = -1
    return inst


def attribution(dens, nears, fars, n_obj, ids=None):
    """dens [K,N,T] float32 -> Ref. An id >= n_obj (possible only in a plane) is counted in no column."""
    win, _, merged = winner(dens, ids)
    w, oz = weights(merged, nears, fars)
    N = dens.shape[1]
    ow, od = np.zeros((N, n_obj)), np.zeros((N, n_obj))
    for k in range(n_obj):
        mine = win == k
        ow[:, k] = np.where(mine, w, 0.0).sum(axis=1)
        od[:, k] = np.where(mine, w * oz, 0.0).sum(axis=1)
    return Ref(win, w, ow, od, instance_of(ow), merged)


def top_two_gap(obj_weights):
    """Per ray: largest minus second largest entry (the largest itself when there is one column)."""
    s = np.sort(np.nan_to_num(obj_weights, nan=0.0), axis=1)
    return s[:, -1] - (s[:, -2] if s.shape[1] > 1 else 0.0)
