"""Numpy statement of the connected-component labelling (csrc/components.hip, include/focnerf.h foc_cc_label / foc_cc_select) and of what
focnerf_amd/components.py and Occupancy.pruned build on it.

Definition. Lattice point i of u[nx, ny, nz] (fp32, z fastest) is inside iff u[i] >= thr in fp32 (a NaN is outside). Two inside points are
connected when they differ by at most 1 in every coordinate (26-connectivity) — stated here as a plain union-find over the 13 forward
neighbours of every inside point, written out in full (tests/test_components_ref.py pins it against scipy.ndimage.label). A component's
root is the smallest linear index among its points; dense ids 0..K-1 number the components by root, ascending.

Keep order. Components sorted by (size descending, root ascending); keep_largest=k keeps the first k of that order, min_voxels=m the
sizes >= m, both given: both must hold.

Occupancy bitfield. Cell (x, y, z) of cascade c is bit (index & 7) of byte (index >> 3), index = c * H^3 + morton3d(x, y, z)
(fixed_cull_ref.morton3d). Each cascade is a 0/1 volume [H,H,H] labelled at threshold 0.5 on its own.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_cull_ref                                                    # noqa: E402

NONE = 0xFFFFFFFF

# the 13 forward directions: the first non-zero component is +1
FORWARD_26 = [(dx, dy, dz) for dx in (0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) > (0, 0, 0)]
FORWARD_18 = [d for d in FORWARD_26 if abs(d[0]) + abs(d[1]) + abs(d[2]) <= 2]       # mutant: no corner diagonals
FORWARD_6 = [d for d in FORWARD_26 if abs(d[0]) + abs(d[1]) + abs(d[2]) == 1]         # mutant: faces only
assert len(FORWARD_26) == 13 and len(FORWARD_18) == 9 and len(FORWARD_6) == 3


def inside(u, thr, strict=False, nan_inside=False):
    """bool like u: u >= thr in fp32. strict / nan_inside are the MUTANTS `>` and NaN-counts-as-inside (test_components_ref.py)."""
    u = np.asarray(u, dtype=np.float32)
    thr = np.float32(thr)
    with np.errstate(invalid="ignore"):
        m = (u > thr) if strict else (u >= thr)
    return (m | np.isnan(u)) if nan_inside else m


def _pairs(mask, directions):
    """Linear index pairs (i, i + d) of inside points adjacent along each direction."""
    nx, ny, nz = mask.shape
    lin = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    out = []
    for dx, dy, dz in directions:
        def cut(a, d, n):
            return slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d))
        (ax, bx), (ay, by), (az, bz) = cut(None, dx, nx), cut(None, dy, ny), cut(None, dz, nz)
        both = mask[ax, ay, az] & mask[bx, by, bz]
        out.append(np.stack([lin[ax, ay, az][both], lin[bx, by, bz][both]], -1))
    return np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)


def roots_of(mask, directions=FORWARD_26):
    """int64 like mask: the smallest linear index of each inside point's component, -1 outside. Union-find, the smaller root wins."""
    mask = np.asarray(mask, dtype=bool)
    parent = list(range(mask.size))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:                                            # compress the walked path
            parent[a], a = r, parent[a]
        return r
    for a, b in _pairs(mask, directions).tolist():
        ra, rb = find(a), find(b)
        if ra < rb:
            parent[rb] = ra
        elif rb < ra:
            parent[ra] = rb
    flat = mask.reshape(-1)
    out = np.full(mask.size, -1, dtype=np.int64)
    for i in np.flatnonzero(flat).tolist():
        out[i] = find(i)
    return out.reshape(mask.shape)


def label(u, thr, directions=FORWARD_26, strict=False, nan_inside=False):
    """-> (labels int32 like u: -1 outside else the dense id, sizes int64 [K], first int64 [K], roots int64 like u)."""
    roots = roots_of(inside(u, thr, strict, nan_inside), directions)
    first, inverse, sizes = np.unique(roots[roots >= 0], return_inverse=True, return_counts=True)
    labels = np.full(roots.shape, -1, dtype=np.int32)
    labels[roots >= 0] = inverse.astype(np.int32)
    return labels, sizes.astype(np.int64), first.astype(np.int64), roots


def kernel_outputs(u, thr):
    """What foc_cc_label writes: (labels uint32 [n] with NONE outside, sizes uint32 [n], counts [K, inside, largest, 0])."""
    _, sizes, first, roots = label(u, thr)
    lab = np.where(roots.reshape(-1) >= 0, roots.reshape(-1), NONE).astype(np.uint32)
    sz = np.zeros(roots.size, dtype=np.uint32)
    sz[first] = sizes
    return lab, sz, [len(first), int(sizes.sum()), int(sizes.max()) if len(sizes) else 0, 0]


def keep_order(sizes, first):
    """The components' dense ids sorted by (size descending, first point ascending)."""
    return np.lexsort((np.asarray(first), -np.asarray(sizes, dtype=np.int64)))


def keep_mask(sizes, first, keep_largest=None, min_voxels=None):
    if keep_largest is None and min_voxels is None:
        raise ValueError("give keep_largest and / or min_voxels")
    keep = np.ones(len(sizes), dtype=bool)
    if keep_largest is not None:
        top = np.zeros(len(sizes), dtype=bool)
        top[keep_order(sizes, first)[:int(keep_largest)]] = True
        keep &= top
    if min_voxels is not None:
        keep &= np.asarray(sizes) >= int(min_voxels)
    return keep


def filter(u, thr, keep_largest=None, min_voxels=None, fill=0.0):
    """u (fp32) with every point of a component that is not kept set to fill."""
    u = np.asarray(u, dtype=np.float32)
    labels, sizes, first, _ = label(u, thr)
    keep = keep_mask(sizes, first, keep_largest, min_voxels)
    drop = (labels >= 0) & ~keep[np.maximum(labels, 0)]
    return np.where(drop, np.float32(fill), u)


# ---------------------------------------------------------------- occupancy bitfields
def _cell_codes(H):
    x, y, z = np.meshgrid(np.arange(H), np.arange(H), np.arange(H), indexing="ij")
    return fixed_cull_ref.morton3d(np.stack([x, y, z], -1))              # [H,H,H] -> Morton code


def unpack_bitfield(bits, cascade, H):
    """uint8 [cascade * H^3 / 8] -> bool [cascade, H, H, H] indexed (x, y, z)."""
    bits = np.asarray(bits, dtype=np.uint8)
    cells = np.unpackbits(bits, bitorder="little").astype(bool).reshape(cascade, H ** 3)
    return cells[:, _cell_codes(H)]


def pack_bitfield(grid):
    """bool [cascade, H, H, H] -> uint8 [cascade * H^3 / 8]."""
    C, H = grid.shape[0], grid.shape[1]
    cells = np.zeros((C, H ** 3), dtype=bool)
    cells[:, _cell_codes(H).reshape(-1)] = grid.reshape(C, -1)
    return np.packbits(cells.reshape(-1), bitorder="little")


def pruned(bits, cascade, H, keep_largest=1, min_cells=None):
    """Occupancy.pruned: every cascade filtered on its own as a 0/1 volume at threshold 0.5."""
    grid = unpack_bitfield(bits, cascade, H)
    out = np.stack([filter(g.astype(np.float32), 0.5, keep_largest, min_cells, 0.0) >= 0.5 for g in grid])
    return pack_bitfield(out)


# ---------------------------------------------------------------- test volumes (shared by the CPU and the GPU tests)
def random_volume(shape, fraction, seed=0):
    """Uniform noise; with threshold 1 - fraction about `fraction` of the points are inside."""
    return np.random.default_rng(seed).random(shape).astype(np.float32)


def corner_pattern(case):
    """The (2,2,2) 0/1 volume with corner c (at (c & 1, (c >> 1) & 1, (c >> 2) & 1)) inside iff bit c of `case` is set."""
    return np.array([(case >> c) & 1 for c in range(8)], dtype=np.float32).reshape(2, 2, 2).transpose(2, 1, 0).copy()


def special_volume():
    """Threshold 0.5. A value EQUAL to the threshold (inside), a NaN (outside) that separates it from a +inf (inside), a -inf (outside),
    and a 1 that touches the first through a corner diagonal only: two components, {(0,0,0), (1,1,1)} and {(1,1,3)}."""
    vol = np.zeros((4, 5, 6), dtype=np.float32)
    vol[1, 1, 1], vol[1, 1, 2], vol[1, 1, 3], vol[3, 3, 5], vol[0, 0, 0] = 0.5, np.nan, np.inf, -np.inf, 1.0
    return vol


def diagonal_pair(shape, t, d, rest=5):
    """A 0/1 volume with the isolated pair p, p + d: p's coordinates along the non-zero components of d stand at t - 1 (+1) or t (-1), so
    that the pair straddles the plane between index t - 1 and t on each of them. -> (volume, p linear, q linear)."""
    p = [t - 1 if c == 1 else t if c == -1 else rest for c in d]
    q = [a + c for a, c in zip(p, d)]
    vol = np.zeros(shape, dtype=np.float32)
    vol[tuple(p)] = vol[tuple(q)] = 1.0
    return vol, int(np.ravel_multi_index(p, shape)), int(np.ravel_multi_index(q, shape))


def serpentine(shape=(33, 9, 70)):
    """One single-voxel-wide boustrophedon path: full z rows at even (x, y), turned round through one voxel at odd y, layers of even x
    joined through one voxel at odd x. -> (0/1 volume, path length)."""
    nx, ny, nz = shape
    vol = np.zeros(shape, dtype=np.float32)
    end = 0                                                              # the z at which the current row ends
    y_up = True
    for x in range(0, nx, 2):
        ys = list(range(0, ny, 2))
        ys = ys if y_up else ys[::-1]
        for k, y in enumerate(ys):
            vol[x, y, :] = 1.0
            end = nz - 1 - end                                           # the row was walked to its other end
            if k + 1 < len(ys):
                vol[x, (y + ys[k + 1]) // 2, end] = 1.0
        if x + 2 < nx:
            vol[x + 1, ys[-1], end] = 1.0
        y_up = not y_up
    return vol, int(vol.sum())


def two_balls(n=28, r1=6.3, r2=3.2):
    """max of two `mesh_ref.sphere_volume`-style fields r - |x - c| with distant centres: two balls at threshold 0, the first larger."""
    ax = np.arange(n, dtype=np.float64)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")

    def ball(c, r):
        return r - np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
    return np.maximum(ball((9.13, 9.21, 9.37), r1), ball((21.4, 20.7, 21.1), r2)).astype(np.float32)
