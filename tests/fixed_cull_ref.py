"""Numpy float32 restatement of the occupancy cull of the fixed-step path (csrc/fixedcull.hip): the grid cell of a sample position,
its occupancy bit, and the mask / offsets / compact order of the occupied samples.

Cell of a position (include/focnerf.h, foc_fixed_cull; csrc/occ_cell.h): level = clamp(frexp exponent of max |x|, 0, cascade - 1),
mip_bound = min(2^level, bound), n = (int)clamp(0.5 * (x / mip_bound + 1) * H, 0, H - 1) per axis, index = level * H^3 + morton3D(n).
The kernel forms x / mip_bound + 1 as fmaf(x, 1 / mip_bound, 1). For a power-of-two `bound` every mip_bound is a power of two: its
reciprocal and the product are exact, the fused and the unfused form round the same single time, and the fp32 expression below IS the
kernel's. `cell_index` therefore refuses other bounds. The product with 0.5 * H runs in double and narrows to float, as in the kernel.

Rows (the block-interleaved sample order, fixedstep.fixed_sample(ray_block=64)): R = ceil(N/64) * T, row (n // 64) * T + i holds sample
i of the 64 rays of block n // 64, ray n on bit n % 64; sample (n, i) stands at row `blocked_row(n, i, T)` of the per-sample arrays.
The compact list holds the occupied samples in that order: slot = offsets[row] + popcount(mask[row] & ((1 << (n % 64)) - 1)).
"""
import numpy as np


def morton3d(n):
    """int [...,3] -> Morton index (csrc/occ_cell.h rm_morton3D)."""
    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    n = np.asarray(n).astype(np.int64)
    return expand(n[..., 0]) | (expand(n[..., 1]) << 1) | (expand(n[..., 2]) << 2)


def cell_index(xyz, bound, cascade, H):
    """fp32 positions [...,3] inside [-bound, bound]^3 -> (index int64 [...], level, n [...,3])."""
    assert float(bound) in (1.0, 2.0, 4.0, 8.0), "the unfused fp32 form equals the kernel's fmaf only at power-of-two bounds"
    xyz = np.asarray(xyz, dtype=np.float32)
    mx = np.abs(xyz).max(-1)
    level = np.clip(np.frexp(mx)[1], 0, cascade - 1).astype(np.int64)
    mip_bound = np.minimum(np.float32(2.0) ** level.astype(np.float32), np.float32(bound)).astype(np.float32)
    t = (xyz / mip_bound[..., None]).astype(np.float32) + np.float32(1.0)            # exact quotient, one fp32 rounding in the sum
    f = (0.5 * t.astype(np.float64) * float(H)).astype(np.float32)
    n = np.clip(f, np.float32(0), np.float32(H - 1)).astype(np.int64)
    return level * H ** 3 + morton3d(n), level, n


def occupied(index, bitfield):
    """Bit index & 7 of byte index >> 3."""
    bitfield = np.asarray(bitfield, dtype=np.uint8)
    return ((bitfield[index >> 3] >> (index & 7).astype(np.uint8)) & 1).astype(bool)


def blocked_row(n, i, T):
    return (n // 64) * 64 * T + i * 64 + n % 64


def cull(occ):
    """occ bool [N,T] (sample i of ray n occupied) -> mask uint64 [R], offsets uint32 [R + 1], order int64 [M_occ,2] = the (n, i) of the
    compact list's slots."""
    occ = np.asarray(occ, dtype=bool)
    N, T = occ.shape
    nblk = -(-N // 64)
    pad = np.zeros((nblk * 64, T), dtype=bool)
    pad[:N] = occ                                                     # the padding lanes never set a bit
    rows = pad.reshape(nblk, 64, T).transpose(0, 2, 1).reshape(nblk * T, 64)          # [R, 64]: lane = n % 64
    mask = (rows.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    counts = rows.sum(-1)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    r, lane = np.nonzero(rows)                                        # row-major: rows ascending, lanes ascending inside a row
    order = np.stack([(r // T) * 64 + lane, r % T], -1).astype(np.int64)
    return mask, offsets, order
