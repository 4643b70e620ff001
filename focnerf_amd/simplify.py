"""Meshes with fewer triangles, on the device (csrc/simplify.hip): vertex clustering on a cell grid.

The marching cubes give two or three vertices per crossed cell, whatever the curvature. The reference hands its arrays to trimesh, where
a user decimates on the host (`simplify_vertex_clustering` / `simplify_quadric_decimation`); here the mesh never leaves the device:

    s = simplify_mesh(vertices, triangles, cell=0.02)                  # a `SimplifiedMesh`: + vertex_map [V], members [Vc]
    s = simplify_mesh(mesh, cell=(0.02, 0.02, 0.04))                   # a `Mesh` with its normals, colours and object ids
    v, f = extract_geometry(model, 256, 10.0, simplify=2)              # mesh.py: cells of 2 x 2 x 2 lattice steps
    save_mesh(model, "object.ply", keep_largest=1, simplify=4)

Every vertex falls into a cell of the grid, the vertices of a cell merge into their mean, and a triangle that loses a corner to a merge
disappears. include/focnerf.h (foc_simplify_count) states the rule exactly and tests/simplify_ref.py states it in numpy; the result is
the same bits on every run and in both deterministic modes (integer atomics only).

What this is not: no quadric-error placement, no edge collapse, no smoothing; oppositely oriented triangle pairs that a merge creates
stay (a closed input stays closed counted with multiplicity, it need not stay manifold); clusters are not split by object.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import lib, ptr, stream_of, check
from .backend import _scratch
from .mesh import Mesh

MAX_CELLS = 1 << 30


@dataclass
class SimplifiedMesh(Mesh):
    """A `Mesh` that came out of `simplify_mesh`, with vertex_map int32 [V] (for every INPUT vertex the output vertex it merged into, -1
    where its cell was not kept) and members int32 [Vc] (how many input vertices each output vertex is the mean of)."""
    vertex_map: Optional[torch.Tensor] = None
    members: Optional[torch.Tensor] = None


def check_simplify(k, who="extract_geometry"):
    """The `simplify=` keyword of the extractors: None (nothing runs) or an integer >= 2, the cell's edge in lattice steps."""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2:
        raise ValueError(f"{who}: simplify must be None or an integer >= 2 (got {k!r})")
    return int(k)


def lattice_grid(origin, spacing, resolution, k):
    """The grid of `simplify=k` on a lattice of `resolution` points per axis: the lattice's origin, cell = fp32(k) * spacing,
    dims = ceil((R - 1) / k). -> (origin, cell, dims)"""
    r = (int(resolution),) * 3 if np.isscalar(resolution) else tuple(int(v) for v in resolution)
    cell = (np.float32(k) * np.asarray(spacing, dtype=np.float32)).astype(np.float32)
    return np.asarray(origin, dtype=np.float32), cell, tuple(-(-(n - 1) // int(k)) for n in r)


def _cell3(cell):
    if cell is None:
        raise ValueError("simplify_mesh: cell (a float or three floats, in the vertices' units) is required")
    c = np.asarray(cell.detach().cpu().numpy() if torch.is_tensor(cell) else cell, dtype=np.float64).reshape(-1)
    if c.size == 1:
        c = np.repeat(c, 3)
    c32 = c.astype(np.float32)
    with np.errstate(all="ignore"):
        if c.size != 3 or not (np.isfinite(c32).all() and (c32 > 0).all() and np.isfinite(np.float32(1) / c32).all()):
            raise ValueError(f"simplify_mesh: cell must be one or three finite values > 0, with a finite fp32 reciprocal (got {cell!r})")
    return c32


def _attribute(name, a, V, dtype, width, dev):
    if a is None:
        return None
    shape = (V, 3) if width == 3 else (V,)
    if not torch.is_tensor(a) or a.dtype != dtype or tuple(a.shape) != shape or a.device != dev:
        raise ValueError(f"simplify_mesh: {name} must be a {dtype} tensor {list(shape)} on {dev}")
    return a.contiguous()


def simplify_mesh(vertices, triangles=None, cell=None, origin=None, dims=None, normals=None, colors=None, object_id=None, unique=False):
    """Vertex clustering of an indexed mesh on the grid (origin, cell, dims) -> `SimplifiedMesh` on the device.

    vertices fp32 [V,3] and triangles int32 [F,3] CUDA tensors, or a `Mesh` in place of both (its attributes are taken unless given).
    cell: a float or three floats, the cell's edges in the vertices' units. normals / colors fp32 [V,3], object_id int32 [V]: optional.
    origin (3 floats) / dims (3 ints >= 1, product <= 2^30): the grid; a vertex outside it belongs to the border cell. When either is
    omitted it is derived from `vertices.amin(0)` / `amax(0)` (the grid then covers the mesh) — that costs a SECOND host read; with both
    given the call synchronises once (the sizes of the result).

    Each output vertex is the mean of ALL input vertices of its cell (`members` of them); a triangle survives iff its corners lie in three
    different cells, and only cells a surviving triangle touches give a vertex, so the output has no unreferenced vertex. Normals are the
    normalised sum, colours the mean of clamp(c, 0, 1), and the object id is that of the cell's member with the smallest index: a cell
    that straddles two objects of a scene mesh merges them under the first one's id — clusters are not split by object. Triangles keep
    their input order and orientation, each rotated so that its smallest index stands first; a closed input gives a closed output
    counted with multiplicity. unique=True additionally returns `torch.unique(triangles, dim=0)`: duplicates leave, rows come in
    lexicographic order, and that invariant no longer holds.

    An empty result (every triangle collapsed, or F = 0) returns empty tensors and a vertex_map of -1.
    ValueError: wrong dtypes, shapes or devices; a cell that is not finite and > 0; a grid beyond 2^30 cells; a non-finite vertex
    coordinate or a triangle index outside [0, V) (both found on the device, by a counted flag in the one host read)."""
    if isinstance(vertices, Mesh):
        m = vertices
        if triangles is not None:
            raise ValueError("simplify_mesh: give a Mesh, or vertices and triangles")
        vertices, triangles = m.vertices, m.triangles
        normals = m.normals if normals is None else normals
        colors = m.colors if colors is None else colors
        object_id = m.object_id if object_id is None else object_id
    cell = _cell3(cell)
    if not torch.is_tensor(vertices) or not vertices.is_cuda or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("simplify_mesh: vertices must be a float32 CUDA tensor [V,3]")
    dev = vertices.device
    if not torch.is_tensor(triangles) or triangles.device != dev or triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise ValueError(f"simplify_mesh: triangles must be an int32 tensor [F,3] on {dev}")
    V, F = vertices.shape[0], triangles.shape[0]
    normals = _attribute("normals", normals, V, torch.float32, 3, dev)
    colors = _attribute("colors", colors, V, torch.float32, 3, dev)
    object_id = _attribute("object_id", object_id, V, torch.int32, 1, dev)
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    if origin is None or dims is None:                                   # the second host read
        lo, hi = (np.zeros(3), np.zeros(3)) if V == 0 else (a.astype(np.float64) for a in torch.stack([vertices.amin(0), vertices.amax(0)]).cpu().numpy())
        if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise ValueError("simplify_mesh: a non-finite vertex coordinate")
        if origin is None:
            origin = lo
        if dims is None:
            dims = np.floor(np.maximum(hi - np.asarray(origin, dtype=np.float64).reshape(3), 0.0) / cell.astype(np.float64)) + 1
            if dims.max() > MAX_CELLS:
                raise ValueError(f"simplify_mesh: cells of {cell.tolist()} over this mesh give a grid beyond 2^30 cells")
    origin = np.asarray(origin.detach().cpu().numpy() if torch.is_tensor(origin) else origin, dtype=np.float32).reshape(-1)
    if origin.size != 3 or not np.isfinite(origin).all():
        raise ValueError("simplify_mesh: origin must be three finite values")
    dims = [int(g) for g in np.asarray(dims).reshape(-1)]
    if len(dims) != 3 or min(dims) < 1 or dims[0] * dims[1] * dims[2] > MAX_CELLS:
        raise ValueError(f"simplify_mesh: dims must be three integers >= 1 with a product of at most 2^30 (got {dims})")
    import ctypes
    org, cel = (ctypes.c_float * 3)(*origin.tolist()), (ctypes.c_float * 3)(*cell.tolist())
    nbytes = lib.foc_simplify_workspace_bytes(V, F, *dims)
    if nbytes == 0:
        raise ValueError("simplify_mesh: " + lib.foc_last_error().decode("utf-8", "replace"))
    workspace = _scratch.get("simplify", nbytes, dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    st = stream_of(vertices)
    check(lib.foc_simplify_count(ptr(vertices), V, ptr(triangles), F, org, cel, *dims, ptr(workspace), nbytes, ptr(counts), st), "simplify_count")
    Vc, Fc, bad_v, bad_i = (int(v) & 0xFFFFFFFF for v in counts.tolist())    # the host read: sizes the outputs, carries the flags
    if bad_v:
        raise ValueError(f"simplify_mesh: {bad_v} vertices hold a non-finite coordinate")
    if bad_i:
        raise ValueError(f"simplify_mesh: {bad_i} triangles hold an index outside [0, {V})")
    out_v = torch.empty(Vc, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(Fc, 3, dtype=torch.int32, device=dev)
    members = torch.empty(Vc, dtype=torch.int32, device=dev)
    out_n = None if normals is None else torch.empty(Vc, 3, dtype=torch.float32, device=dev)
    out_c = None if colors is None else torch.empty(Vc, 3, dtype=torch.float32, device=dev)
    out_id = None if object_id is None else torch.empty(Vc, dtype=torch.int32, device=dev)
    if Vc == 0 or Fc == 0:                                               # both or neither: a kept cell has a surviving triangle
        return SimplifiedMesh(out_v, out_t, out_n, out_c, out_id, torch.full((V,), -1, dtype=torch.int32, device=dev), members)
    vertex_map = torch.empty(V, dtype=torch.int32, device=dev)
    abytes = lib.foc_simplify_accum_bytes(Vc, int(normals is not None), int(colors is not None))
    accum = _scratch.get("simplify_accum", abytes, dev)
    check(lib.foc_simplify_emit(ptr(vertices), V, ptr(triangles), F, ptr(normals), ptr(colors), ptr(object_id), org, cel, *dims, ptr(workspace), ptr(accum),
                                abytes, Vc, Fc, ptr(out_v), ptr(out_n), ptr(out_c), ptr(out_id), ptr(vertex_map), ptr(members), ptr(out_t), st), "simplify_emit")
    if unique:
        out_t = torch.unique(out_t, dim=0)
    return SimplifiedMesh(out_v, out_t, out_n, out_c, out_id, vertex_map, members)
