"""Numpy float64 statement of the mesh extraction (csrc/mesh.hip, include/focnerf.h foc_mc_count / foc_lattice_cull): marching cubes on a
float32 volume u[nx, ny, nz] (z fastest), and the cull of a lattice slab against an object's box and occupancy grid.

Marching cubes. A corner is inside iff u >= thr. Corner c of a cube sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); the 12 edges are
axis-major (x, y, z), within an axis by lower corner. A vertex belongs to the lattice edge it lies on, owned by the edge's lower
endpoint p: t = (thr - u[p]) / (u[p + e] - u[p]), position = index of p plus t along the axis (here in float64 from the fp32 values).
Vertices are numbered by (linear index of the owner, axis), triangles by (linear index of the cube, table order); the table is the one
tools/make_mc_table.py generates. Normals: the gradient by central differences (one-sided on the border) at both endpoints, mixed with
t, divided per axis by the spacing, negated and normalised; a zero gradient gives (0, 0, 0).

Lattice cull. Point i of the lattice (linear, z fastest) stands at (xs[ix], ys[iy], zs[iz]) in fp32. With a placement the point is mapped
by q_k = ((A_k0 x + A_k1 y) + A_k2 z) + b_k in fp32, this order, and is empty outside the object's box; with a bitfield its cell
(fixed_cull_ref.cell_index) must be set. Bit i % 64 of mask[i // 64], offsets = exclusive prefix sum of the words' popcounts, the
compact list in lattice order.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_mc_table                                                     # noqa: E402
import fixed_cull_ref                                                    # noqa: E402

TABLE = make_mc_table.build_table()
NTRI = np.array([len(t) for t in TABLE], dtype=np.int64)
TRI = np.full((256, 15), -1, dtype=np.int64)
for _case, _tris in enumerate(TABLE):
    _flat = [e for t in _tris for e in t]
    TRI[_case, :len(_flat)] = _flat
EDGE_CORNER = np.array([a for a, _ in make_mc_table.EDGES], dtype=np.int64)       # lower corner of edge e; axis = e // 4


def _shift(a, axis):
    """a[p + e_axis] where it exists, shaped like a (the last layer along the axis repeats: never used, the edge does not exist)."""
    idx = np.minimum(np.arange(a.shape[axis]) + 1, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def _gradient(u):
    """float64 [nx,ny,nz,3]: central differences, one-sided on the border, lattice units."""
    g = np.zeros(u.shape + (3,))
    for axis in range(3):
        n = u.shape[axis]
        hi = np.take(u, np.minimum(np.arange(n) + 1, n - 1), axis=axis)
        lo = np.take(u, np.maximum(np.arange(n) - 1, 0), axis=axis)
        shape = [1, 1, 1]
        shape[axis] = n
        width = np.full(n, 2.0)
        width[0] = width[-1] = 1.0
        g[..., axis] = (hi - lo) / width.reshape(shape)
    return g


def marching_cubes(u, thr, origin=(0, 0, 0), spacing=(1, 1, 1), normals=False):
    """-> (vertices float64 [V,3], triangles int64 [F,3][, normals float64 [V,3]]). ValueError for a non-finite value on a crossed edge."""
    u32 = np.ascontiguousarray(u, dtype=np.float32)
    assert u32.ndim == 3 and min(u32.shape) >= 2
    thr = np.float32(thr)
    u = u32.astype(np.float64)
    nx, ny, nz = u.shape
    inside = u32 >= thr
    cross = np.zeros(u.shape + (3,), dtype=bool)
    tpar = np.zeros(u.shape + (3,))
    for axis in range(3):
        exists = np.arange(u.shape[axis]) < u.shape[axis] - 1
        shape = [1, 1, 1]
        shape[axis] = -1
        cross[..., axis] = (inside != _shift(inside, axis)) & exists.reshape(shape)
        u1 = _shift(u, axis)
        if (cross[..., axis] & ~(np.isfinite(u) & np.isfinite(u1))).any():
            raise ValueError("marching_cubes: a non-finite value on an edge the surface crosses")
        with np.errstate(all="ignore"):
            tpar[..., axis] = np.where(cross[..., axis], (float(thr) - u) / (u1 - u), 0.0)
    flat = cross.reshape(-1)                                             # (linear point, axis): the vertex numbering
    vid = (np.cumsum(flat) - 1).reshape(u.shape + (3,))
    px, py, pz, pa = np.nonzero(cross)
    base = np.stack([px, py, pz], -1).astype(np.float64)
    t = tpar[px, py, pz, pa]
    base[np.arange(len(pa)), pa] += t
    org, spc = np.asarray(origin, dtype=np.float64), np.asarray(spacing, dtype=np.float64)
    vertices = org + base * spc

    cx, cy, cz = nx - 1, ny - 1, nz - 1
    case = np.zeros((cx, cy, cz), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[ox:ox + cx, oy:oy + cy, oz:oz + cz].astype(np.int64) << c
    qx, qy, qz = np.nonzero(NTRI[case] > 0)                             # cubes in lattice order
    tris = []
    for x, y, z in zip(qx, qy, qz):
        k = case[x, y, z]
        for j in range(NTRI[k]):
            tri = []
            for e in TRI[k, 3 * j:3 * j + 3]:
                c = EDGE_CORNER[e]
                tri.append(vid[x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1), e // 4])
            tris.append(tri)
    triangles = np.array(tris, dtype=np.int64).reshape(-1, 3)
    if not normals:
        return vertices, triangles
    g = _gradient(u)
    g0 = g[px, py, pz]
    qq = [px.copy(), py.copy(), pz.copy()]
    for axis in range(3):
        qq[axis] = qq[axis] + (pa == axis)
    g1 = g[qq[0], qq[1], qq[2]]
    gm = ((1.0 - t)[:, None] * g0 + t[:, None] * g1) / spc
    length = np.linalg.norm(gm, axis=-1, keepdims=True)
    nrm = np.where(length > 0, -gm / np.where(length > 0, length, 1.0), 0.0)
    return vertices, triangles, nrm


# ---------------------------------------------------------------- properties of an indexed mesh
def directed_edge_counts(triangles):
    """{(a, b): how many triangles run a -> b}."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    pairs, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(pairs, counts)}


def is_closed(triangles):
    """Every directed edge a -> b appears as often as b -> a: closed and consistently oriented."""
    d = directed_edge_counts(triangles)
    return all(d.get((b, a), 0) == c for (a, b), c in d.items())


def is_manifold(triangles):
    """Every directed edge exactly once, with its reverse."""
    d = directed_edge_counts(triangles)
    return all(c == 1 and d.get((b, a), 0) == 1 for (a, b), c in d.items())


def euler_characteristic(n_vertices, triangles):
    d = directed_edge_counts(triangles)
    return int(n_vertices) - len({(min(a, b), max(a, b)) for a, b in d}) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---------------------------------------------------------------- test volumes (shared by the CPU and the GPU tests)
def noise_volume(n, seed=0):
    vol = np.zeros((n, n, n), dtype=np.float32)
    vol[1:-1, 1:-1, 1:-1] = np.random.default_rng(seed).random((n - 2,) * 3)
    return vol


def _centred_grid(n, offset):
    ax = [np.arange(n, dtype=np.float64) - (n - 1) / 2 - o for o in offset]
    return np.meshgrid(*ax, indexing="ij")


def sphere_volume(n=20, r=6.3, offset=(0.13, 0.21, 0.37)):
    """r - |x - c|: inside (>= 0) the ball; threshold 0. Analytic volume 4/3 pi r^3."""
    x, y, z = _centred_grid(n, offset)
    return (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def torus_volume(n=20, R=6.0, r=2.5, offset=(0.13, 0.21, 0.37)):
    """r - distance to the circle of radius R in the xy plane; threshold 0. Analytic volume 2 pi^2 R r^2."""
    x, y, z = _centred_grid(n, offset)
    return (r - np.sqrt((np.sqrt(x * x + y * y) - R) ** 2 + z * z)).astype(np.float32)


# ---------------------------------------------------------------- lattice cull
def lattice_points(xs, ys, zs, first=0, count=None):
    """fp32 [count,3]: the lattice points first .. first + count in linear order (z fastest)."""
    xs, ys, zs = (np.asarray(a, dtype=np.float32) for a in (xs, ys, zs))
    n = len(xs) * len(ys) * len(zs)
    count = n - first if count is None else count
    i = np.arange(first, first + count)
    return np.stack([xs[i // (len(ys) * len(zs))], ys[(i // len(zs)) % len(ys)], zs[i % len(zs)]], -1)


def to_object(w2o, p):
    """q_k = ((A_k0 x + A_k1 y) + A_k2 z) + b_k in fp32, in this order."""
    w = np.asarray(w2o, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((w[3 * k] * x + w[3 * k + 1] * y).astype(np.float32) + w[3 * k + 2] * z).astype(np.float32) + w[9 + k] for k in range(3)], -1).astype(np.float32)


def lattice_cull(xs, ys, zs, first=0, count=None, w2o=None, obj_aabb=None, bound=None, bitfield=None, cascade=None, H=None):
    """-> (mask uint64 [R], offsets uint32 [R + 1], positions fp32 [M,3]) of the slab, R = ceil(count / 64)."""
    p = lattice_points(xs, ys, zs, first, count)
    keep = np.ones(len(p), dtype=bool)
    if w2o is not None:
        p = to_object(w2o, p)
        box = np.asarray(obj_aabb, dtype=np.float32)
        keep &= ((p >= box[:3]) & (p <= box[3:])).all(-1)
    if bitfield is not None:
        index, _, _ = fixed_cull_ref.cell_index(p, bound, cascade, H)
        index = np.minimum(index, cascade * H ** 3 - 1)
        keep &= fixed_cull_ref.occupied(index, bitfield)
    R = -(-len(p) // 64)
    rows = np.zeros(R * 64, dtype=bool)
    rows[:len(p)] = keep
    rows = rows.reshape(R, 64)
    mask = (rows.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(rows.sum(-1))]).astype(np.uint32)
    return mask, offsets, p[keep]
