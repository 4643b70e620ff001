"""Numpy statement of the vertex clustering (csrc/simplify.hip, include/focnerf.h foc_simplify_count / foc_simplify_emit). It is the
definition: the kernels are held to it bit for bit. fp32 steps are numpy float32 operations (each rounded on its own), sums are int64,
means float64.

Grid: origin[3], cell[3] fp32, dims (gx, gy, gz) each >= 1 with gx * gy * gz <= 2^30, inv = fp32(1) / cell.
  1. Per axis t = (v - origin) * inv (one fp32 subtraction, one fp32 multiplication), c = clamp(floor(t), 0, g - 1),
     r = clamp(t - float(c), 0, 1), cell number k = (cx * gy + cy) * gz + cz.
  2. A triangle survives iff its three corners lie in three different cells.
  3. A cell is kept iff a surviving triangle has a corner in it; kept cells are numbered in rising k; vertex_map[v] is the number of
     v's cell or -1.
  4. The vertex of a kept cell: q = (int64)(r * 2^30) per member and axis, S = sum q, m = (double)S / (double)count / 2^30,
     x = fp32(origin + (c + m) * cell) in float64 operations; members = count. ALL input vertices of the cell are members.
  5. Normal: sum of (int64)(clamp(n, -1, 1) * 2^30) (a non-finite component counts 0), s / sqrt(sx sx + sy sy + sz sz) in float64, 0 for
     length 0. Colour: the mean of clamp(c, 0, 1) (a NaN counts 0) through the same fixed point. Object id: that of the member with the
     smallest vertex index.
  6. Output triangles: the survivors in input order, renumbered, rotated so that the smallest number stands first. unique=True: the
     distinct rows in lexicographic order.
  7. ValueError: a non-finite vertex, an index outside [0, V), a non-finite or non-positive cell, a grid beyond the limit.

`mutant` switches ONE rule to a plausible wrong reading (tests/test_simplify_ref.py proves that its cases tell them apart).
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402

MAX_CELLS = 1 << 30
FIX = np.float32(2.0 ** 30)
MUTANTS = ("round", "divide", "noclamp", "kept_by_vertices", "mean_of_corners", "norotate")


def grid(origin, cell, dims):
    """-> (origin fp32 [3], cell fp32 [3], inv fp32 [3], dims (gx, gy, gz)) after rule 7's refusals."""
    origin = np.asarray(origin, dtype=np.float32).reshape(3)
    cell = np.broadcast_to(np.asarray(cell, dtype=np.float32), (3,)).copy()
    dims = tuple(int(g) for g in dims)
    if not np.isfinite(origin).all():
        raise ValueError("simplify: non-finite origin")
    if not (np.isfinite(cell).all() and (cell > 0).all()):
        raise ValueError("simplify: cell must be finite and > 0")
    with np.errstate(all="ignore"):
        inv = (np.float32(1) / cell).astype(np.float32)
    if not np.isfinite(inv).all():
        raise ValueError("simplify: cell is too small (1 / cell is not finite)")
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > MAX_CELLS:
        raise ValueError("simplify: dims must be three integers >= 1 with a product of at most 2^30")
    return origin, cell, inv, dims


def lattice_grid(origin, spacing, resolution, k):
    """The grid of `simplify=k` on a lattice: its origin, cell = fp32(k) * spacing, dims = ceil((R - 1) / k)."""
    r = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(v) for v in resolution)
    spacing = np.broadcast_to(np.asarray(spacing, dtype=np.float32), (3,))
    return np.asarray(origin, dtype=np.float32), (np.float32(k) * spacing).astype(np.float32), tuple(-(-(n - 1) // int(k)) for n in r)


def cells(vertices, origin, cell, inv, dims, mutant=None):
    """Rule 1 -> (c int64 [V,3], r fp32 [V,3], k int64 [V])."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = (v - origin).astype(np.float32)
        t = (d / cell).astype(np.float32) if mutant == "divide" else (d * inv).astype(np.float32)
        f = (np.rint(t) if mutant == "round" else np.floor(t)).astype(np.float64)
        g = np.asarray(dims, dtype=np.float64)
        c = (f if mutant == "noclamp" else np.clip(f, 0.0, g - 1.0)).astype(np.int64)
        r = (t - c.astype(np.float32)).astype(np.float32)
        r = np.clip(r, np.float32(0), np.float32(1))
    k = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    return c, r, k


def _fixed(a):
    return (np.asarray(a, dtype=np.float32) * FIX).astype(np.float32).astype(np.int64)      # exact product, truncated


def _sum_by(index, values, n):
    out = np.zeros((n,) + values.shape[1:], dtype=np.int64)
    np.add.at(out, index, values)
    return out


def simplify(vertices, triangles, origin, cell, dims, normals=None, colors=None, object_id=None, unique=False, mutant=None):
    """-> namespace(vertices fp32 [Vc,3], triangles int32 [Fc,3], vertex_map int32 [V], members int32 [Vc], normals, colors fp32 [Vc,3]
    or None, object_id int32 [Vc] or None, cell_number int64 [Vc])."""
    assert mutant is None or mutant in MUTANTS
    origin, cell, inv, dims = grid(origin, cell, dims)
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = len(v)
    if not np.isfinite(v).all():
        raise ValueError("simplify: a non-finite vertex coordinate")
    if len(tri) and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("simplify: a triangle index outside [0, V)")
    c, r, k = cells(v, origin, cell, inv, dims, mutant)
    tk = k[tri]
    survive = (tk[:, 0] != tk[:, 1]) & (tk[:, 1] != tk[:, 2]) & (tk[:, 0] != tk[:, 2])
    kept = np.unique(k if mutant == "kept_by_vertices" else tk[survive])                   # rising k
    slot = np.searchsorted(kept, k)
    mapped = (slot < len(kept)) & (kept[np.minimum(slot, max(len(kept) - 1, 0))] == k) if len(kept) else np.zeros(V, dtype=bool)
    vertex_map = np.where(mapped, slot, -1).astype(np.int32)
    Vc = len(kept)
    member = mapped.copy()
    if mutant == "mean_of_corners":
        used = np.zeros(V, dtype=bool)
        used[tri[survive].reshape(-1)] = True
        member &= used
    idx = vertex_map[member]
    count = np.bincount(idx, minlength=Vc).astype(np.int64)
    first = np.full(Vc, V, dtype=np.int64)
    np.minimum.at(first, idx, np.nonzero(member)[0])
    S = _sum_by(idx, _fixed(r[member]), Vc)
    cc = c[np.minimum(first, max(V - 1, 0))] if Vc else np.zeros((0, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        m = S.astype(np.float64) / count.astype(np.float64)[:, None] / 2.0 ** 30
        out_v = (origin.astype(np.float64) + (cc.astype(np.float64) + m) * cell.astype(np.float64)).astype(np.float32)
    res = SimpleNamespace(vertices=out_v, vertex_map=vertex_map, members=count.astype(np.int32), normals=None, colors=None, object_id=None,
                          cell_number=kept)
    if normals is not None:
        n = np.asarray(normals, dtype=np.float32).reshape(V, 3)
        n = np.where(np.isfinite(n), np.clip(n, np.float32(-1), np.float32(1)), np.float32(0)).astype(np.float32)
        s = _sum_by(idx, _fixed(n[member]), Vc).astype(np.float64)
        length = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        with np.errstate(all="ignore"):
            res.normals = np.where(length[:, None] > 0, s / length[:, None], 0.0).astype(np.float32)
    if colors is not None:
        col = np.asarray(colors, dtype=np.float32).reshape(V, 3)
        col = np.where(np.isnan(col), np.float32(0), np.clip(col, np.float32(0), np.float32(1))).astype(np.float32)
        s = _sum_by(idx, _fixed(col[member]), Vc).astype(np.float64)
        with np.errstate(all="ignore"):
            res.colors = (s / count.astype(np.float64)[:, None] / 2.0 ** 30).astype(np.float32)
    if object_id is not None:
        ids = np.asarray(object_id, dtype=np.int32).reshape(V)
        res.object_id = ids[np.minimum(first, max(V - 1, 0))] if Vc else np.zeros(0, dtype=np.int32)
    t = vertex_map[tri[survive]].astype(np.int64).reshape(-1, 3)
    if mutant != "norotate" and len(t):
        t = np.take_along_axis(t, (np.argmin(t, axis=1)[:, None] + np.arange(3)) % 3, axis=1)
    if unique and len(t):
        t = np.unique(t, axis=0)
    res.triangles = t.astype(np.int32).reshape(-1, 3)
    return res


def brute_force(vertices, triangles, origin, cell, dims, normals=None, colors=None, object_id=None):
    """The same rules a second way: Python loops over cells and triangles, the cell by float32 scalars, the means as exact fractions
    rounded once to float64. For small meshes."""
    from fractions import Fraction
    origin, cell, inv, dims = grid(origin, cell, dims)
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    f32 = np.float32
    key, frac, coord = [], [], []
    for p in v:
        cs, rs = [], []
        for a in range(3):
            t = f32(f32(p[a] - origin[a]) * inv[a])
            ci = min(max(int(np.floor(np.float64(t))), 0), dims[a] - 1)
            rr = f32(t - f32(ci))
            rs.append(f32(0) if rr < 0 else f32(1) if rr > 1 else rr)
            cs.append(ci)
        key.append((cs[0] * dims[1] + cs[1]) * dims[2] + cs[2])
        frac.append(rs)
        coord.append(cs)
    tris, touched = [], set()
    for a, b, c in np.asarray(triangles, dtype=np.int64).reshape(-1, 3):
        if len({key[a], key[b], key[c]}) == 3:
            tris.append((a, b, c))
            touched |= {key[a], key[b], key[c]}
    order = sorted(touched)
    number = {k: j for j, k in enumerate(order)}
    vertex_map = np.array([number.get(k, -1) for k in key], dtype=np.int32)
    out_v, members, out_n, out_c, out_id = [], [], [], [], []
    for k in order:
        mem = [i for i in range(len(v)) if key[i] == k]
        members.append(len(mem))
        row = []
        for a in range(3):
            S = sum(int(Fraction(float(frac[i][a])) * 2 ** 30) for i in mem)
            m = float(Fraction(S, len(mem) * 2 ** 30))
            row.append(f32(np.float64(origin[a]) + (np.float64(coord[mem[0]][a]) + np.float64(m)) * np.float64(cell[a])))
        out_v.append(row)
        if normals is not None:
            s = []
            for a in range(3):
                tot = 0
                for i in mem:
                    x = float(normals[i][a])
                    x = 0.0 if not np.isfinite(x) else min(max(x, -1.0), 1.0)
                    tot += int(Fraction(x) * 2 ** 30)                    # int() truncates toward zero
                s.append(np.float64(tot))
            length = np.sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2])
            out_n.append([f32(x / length) if length > 0 else f32(0) for x in s])
        if colors is not None:
            row = []
            for a in range(3):
                tot = 0
                for i in mem:
                    x = float(colors[i][a])
                    x = 0.0 if np.isnan(x) else min(max(x, 0.0), 1.0)
                    tot += int(Fraction(x) * 2 ** 30)
                row.append(f32(float(Fraction(tot, len(mem) * 2 ** 30))))
            out_c.append(row)
        if object_id is not None:
            out_id.append(int(object_id[min(mem)]))
    out_t = []
    for tri in tris:
        n = [int(vertex_map[i]) for i in tri]
        j = n.index(min(n))
        out_t.append(n[j:] + n[:j])
    return SimpleNamespace(vertices=np.array(out_v, dtype=np.float32).reshape(-1, 3), triangles=np.array(out_t, dtype=np.int32).reshape(-1, 3),
                           vertex_map=vertex_map, members=np.array(members, dtype=np.int32),
                           normals=None if normals is None else np.array(out_n, dtype=np.float32).reshape(-1, 3),
                           colors=None if colors is None else np.array(out_c, dtype=np.float32).reshape(-1, 3),
                           object_id=None if object_id is None else np.array(out_id, dtype=np.int32))


def same(a, b, normal_tol=None):
    """Every output of two results agrees: floats by their bits (normals within normal_tol when given), integers as integers."""
    def bits(x, y):
        return (x is None and y is None) or (x is not None and y is not None and x.shape == y.shape and x.dtype == y.dtype
                                             and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)))
    ok = bits(a.vertices, b.vertices) and bits(a.colors, b.colors) and bits(a.object_id, b.object_id)
    ok = ok and bits(a.triangles, b.triangles) and bits(a.vertex_map, b.vertex_map) and bits(a.members, b.members)
    if normal_tol is None or a.normals is None or b.normals is None:
        return ok and bits(a.normals, b.normals)
    return ok and a.normals.shape == b.normals.shape and bool((np.abs(a.normals.astype(np.float64) - b.normals.astype(np.float64)) <= normal_tol).all())


# ---------------------------------------------------------------- the shared meshes (marching cubes of mesh_ref's volumes, computed once)
_MESHES = {}


def mesh(name):
    """-> (vertices fp32 [V,3] in lattice units, triangles int32 [F,3], n) of "sphere" / "torus" / "noise40" / "noise12"."""
    if name not in _MESHES:
        if name == "sphere":
            vol, thr = mesh_ref.sphere_volume(32, 11.3), 0.0
        elif name == "torus":
            vol, thr = mesh_ref.torus_volume(40, 12.0, 5.0), 0.0
        elif name in ("noise40", "noise12"):
            vol = mesh_ref.noise_volume(int(name[5:]))
            thr = float(np.median(vol))
        else:
            raise KeyError(name)
        v, t = mesh_ref.marching_cubes(vol, thr)
        _MESHES[name] = (v.astype(np.float32), t.astype(np.int32), vol.shape[0])
    return _MESHES[name]


def attributes(V, seed=0, wild=False):
    """Per-vertex normals, colours and object ids for V vertices; wild: NaN, infinities and out-of-range values among them."""
    rng = np.random.default_rng(seed)
    n = rng.normal(size=(V, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    c = rng.random((V, 3)).astype(np.float32)
    ids = rng.integers(0, 5, V).astype(np.int32)
    if wild and V:
        pick = rng.integers(0, V, max(V // 7, 1))
        c[pick, 0] = np.nan
        c[rng.integers(0, V, max(V // 7, 1)), 1] = 1.75
        c[rng.integers(0, V, max(V // 7, 1)), 2] = -0.5
        n[rng.integers(0, V, max(V // 9, 1)), 0] = np.inf
        n[rng.integers(0, V, max(V // 9, 1)), 1] = np.nan
        n[rng.integers(0, V, max(V // 9, 1)), 2] = -3.0
    return n, c, ids
