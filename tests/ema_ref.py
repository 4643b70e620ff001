"""The parameter EMA's rule (include/focnerf.h, focnerf_amd/ema.py; torch_ema 0.3's update), stated twice. numpy only.

    n        <- n + 1                                   (only with use_num_updates; n starts at 0)
    decay_t   = min(decay, (1 + n) / (10 + n))          in double; plain `decay` without use_num_updates
    omd       = float32(1.0 - decay_t)
    s        <- fl32( s - fl32( fl32(s - p) * omd ) )

`update_f64` is the statement in float64 (omd is the fp32 number of the contract, promoted exactly); `update_f32` is the fp32 operation
sequence: three roundings, no contraction (numpy rounds every fp32 operation once). `bound` is what three roundings can put between the
two: with U = 2^-24 the relative error of one rounding, fl(s - p) = (s - p)(1 + e1), its product with omd (1 + e2), the last subtraction
(1 + e3), so |s32 - s64| <= U |s64| + 2 U |(s - p) omd| to first order; the factor (1 + 4 U) covers the second-order terms. Checked by
tests/test_ema_ref.py."""
import numpy as np

U = 2.0 ** -24          # one fp32 rounding: relative error at most U


def decay_at(decay, n):
    """decay_t for the count n AFTER the advance (None: constant decay), in Python's double arithmetic"""
    return float(decay) if n is None else min(float(decay), (1 + n) / (10 + n))


def omd(decay, n):
    """float32(1 - decay_t) as a numpy float32"""
    return np.float32(1.0 - decay_at(decay, n))


def omd_bits(decay, n):
    return int(np.float32(omd(decay, n)).view(np.uint32))


def update_f64(s, p, one_minus_decay):
    s, p = np.asarray(s, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return s - (s - p) * float(one_minus_decay)


def update_f32(s, p, one_minus_decay):
    s, p, o = np.asarray(s, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(one_minus_decay)
    d = (s - p).astype(np.float32)
    t = (d * o).astype(np.float32)
    return (s - t).astype(np.float32)


def bound(s, p, one_minus_decay):
    s, p = np.asarray(s, dtype=np.float64), np.asarray(p, dtype=np.float64)
    return U * (np.abs(update_f64(s, p, one_minus_decay)) + 2.0 * np.abs((s - p) * float(one_minus_decay))) * (1.0 + 4.0 * U)


def run(shadows, params_per_update, decay, n0=0, use_num_updates=True):
    """`shadows` (list of fp32 arrays) through one fp32 update per entry of `params_per_update` (each a list of arrays) -> (shadows, n)"""
    shadows = [np.asarray(s, dtype=np.float32).copy() for s in shadows]
    n = n0 if use_num_updates else None
    for params in params_per_update:
        if n is not None:
            n += 1
        o = omd(decay, n)
        shadows = [update_f32(s, p, o) for s, p in zip(shadows, params)]
    return shadows, n
