"""csrc/simplify.hip against tests/simplify_ref.py, the numpy statement of the vertex clustering: every output with np.array_equal —
vertices, colours and normals by their fp32 bits, vertex_map, members, triangles and object ids as integers. For the normals one fp32
rounding (2^-23 absolute per component) would be the bound that reasoning gives; the build's float64 division and square root are
correctly rounded and give numpy's bits in every case here (no component differed on an MI355X), so the bits are asserted."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as sr                                                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(m):
    """A SimplifiedMesh as simplify_ref's namespace."""
    h = lambda t: None if t is None else t.cpu().numpy()               # noqa: E731
    return sr.SimpleNamespace(vertices=h(m.vertices), triangles=h(m.triangles), vertex_map=h(m.vertex_map), members=h(m.members),
                              normals=h(m.normals), colors=h(m.colors), object_id=h(m.object_id))


def _run(v, t, grid, normals=None, colors=None, object_id=None, unique=False):
    from focnerf_amd import simplify_mesh
    origin, cell, dims = grid
    return simplify_mesh(_dev(v), _dev(t), cell=cell, origin=origin, dims=dims, normals=_dev(normals), colors=_dev(colors), object_id=_dev(object_id),
                         unique=unique)


def _check(v, t, grid, normals=None, colors=None, object_id=None, unique=False):
    want = sr.simplify(v, t, *grid, normals=normals, colors=colors, object_id=object_id, unique=unique)
    got = _host(_run(v, t, grid, normals, colors, object_id, unique))
    for name in ("vertices", "triangles", "vertex_map", "members", "colors", "object_id"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert (got.normals is None) == (want.normals is None)
    if want.normals is not None:
        err = np.abs(got.normals.astype(np.float64) - want.normals.astype(np.float64))
        print("normals: max error %.3g, %d of %d components differ in their bits" % (err.max() if err.size else 0.0,
              int((got.normals.view(np.uint32) != want.normals.view(np.uint32)).sum()), err.size))
        assert got.normals.shape == want.normals.shape and np.array_equal(got.normals.view(np.uint32), want.normals.view(np.uint32))
    return want


@functools.lru_cache(maxsize=None)
def _world_sphere():
    v, t, n = sr.mesh("sphere")
    spacing = np.float32(2 / 31)
    return (np.float32(-1) + v * spacing).astype(np.float32), t, n, spacing


# ---------------------------------------------------------------- the four meshes of the table, lattice units
TABLE = {("sphere", 2): (538, 1072), ("sphere", 3): (247, 490), ("sphere", 4): (133, 262),
         ("torus", 2): (774, 1548), ("torus", 3): (374, 778), ("torus", 4): (222, 444),
         ("noise40", 2): (7991, 38184), ("noise40", 3): (2197, 16306), ("noise40", 4): (1000, 9288),
         ("noise12", 2): (212, 514), ("noise12", 3): (64, 188), ("noise12", 4): (27, 86)}


@pytest.mark.parametrize("name,k", sorted(TABLE))
def test_table_meshes(name, k):
    v, t, n = sr.mesh(name)
    want = _check(v, t, sr.lattice_grid((0, 0, 0), (1, 1, 1), n, k))
    assert (len(want.vertices), len(want.triangles)) == TABLE[name, k]


# ---------------------------------------------------------------- world-unit grids
@pytest.mark.parametrize("k", [2, 3, 4])
def test_sphere_in_world_units(k):
    v, t, n, spacing = _world_sphere()
    want = _check(v, t, sr.lattice_grid((-1, -1, -1), (spacing,) * 3, n, k))
    assert (len(want.vertices), len(want.triangles)) == TABLE["sphere", k]


def test_grid_with_origin_three_cells_three_dims():
    v, t, _, _ = _world_sphere()
    want = _check(v, t, ((-0.93, -1.07, -0.81), (0.137, 0.093, 0.211), (14, 23, 9)))
    assert len(want.triangles) > 0


def test_grid_smaller_than_the_mesh_clamps_on_both_sides():
    v, t, _, _ = _world_sphere()
    grid = ((-0.4, -0.35, -0.3), (0.11, 0.13, 0.09), (7, 5, 6))
    c, _, _ = sr.cells(v, *sr.grid(*grid), mutant="noclamp")
    assert (c < 0).any() and (c >= np.array(grid[2])).any()             # the clamp acts below and above
    _check(v, t, grid)


def test_sparse_grid_of_more_than_1024_scan_groups():
    v, t, _, _ = _world_sphere()
    dims = (164, 164, 164)
    assert -(-(164 ** 3) // 4096) > 1024
    want = _check(v, t, ((-15.5, -15.5, -15.5), (0.19,) * 3, dims))
    assert len(want.vertices) > 0


# ---------------------------------------------------------------- sizes that are not multiples of 64
def _fan(F):
    """F triangles around vertex 0, every vertex in a cell of its own on a grid of unit cells."""
    ang = np.linspace(0.0, 1.5, F + 1)
    ring = np.stack([4 + 3 * np.cos(ang) * (1 + np.arange(F + 1) % 3), 4 + 3 * np.sin(ang) * (1 + np.arange(F + 1) % 3), np.arange(F + 1) * 1.0], -1)
    v = np.concatenate([[[0.5, 0.5, 0.5]], ring]).astype(np.float32)
    t = np.stack([np.zeros(F, dtype=np.int32), np.arange(1, F + 1, dtype=np.int32), np.arange(2, F + 2, dtype=np.int32)], -1)
    return v, t, ((0, 0, 0), (1.0,) * 3, (16, 16, F + 2))


def test_fewer_than_64_triangles():
    v, t, grid = _fan(37)
    want = _check(v, t, grid)
    assert 0 < len(want.triangles) <= 37


def test_one_triangle_kept():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5]], dtype=np.float32)
    want = _check(v, np.array([[2, 0, 1]], dtype=np.int32), ((0, 0, 0), 1.0, (2, 2, 1)))
    assert len(want.triangles) == 1 and want.members.tolist() == [2, 1, 1] and want.triangles.tolist() == [[0, 2, 1]]


def test_one_triangle_collapsed_is_an_empty_result():
    v = np.array([[0.5, 0.5, 0.5], [0.7, 0.5, 0.5], [0.5, 1.5, 0.5]], dtype=np.float32)
    n, c, ids = sr.attributes(3)
    want = _check(v, np.array([[0, 1, 2]], dtype=np.int32), ((0, 0, 0), 1.0, (2, 2, 1)), n, c, ids)
    assert len(want.vertices) == 0 and len(want.triangles) == 0 and (want.vertex_map == -1).all()


def test_no_triangles():
    v, _, _, _ = _world_sphere()
    want = _check(v[:100], np.zeros((0, 3), dtype=np.int32), ((-1, -1, -1), 0.25, (8, 8, 8)))
    assert len(want.vertices) == 0
    _check(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32), ((-1, -1, -1), 0.25, (8, 8, 8)))


# ---------------------------------------------------------------- attributes
@pytest.mark.parametrize("which", ["all", "normals", "colors", "object_id", "wild"])
def test_attributes(which):
    v, t, n = sr.mesh("noise12")
    nrm, col, ids = sr.attributes(len(v), seed=5, wild=which == "wild")
    if which == "wild":
        assert np.isnan(col).any() and (col > 1).any() and (col < 0).any() and not np.isfinite(nrm).all()
    kw = {"normals": nrm, "colors": col, "object_id": ids}
    if which not in ("all", "wild"):
        kw = {which: kw[which]}
    for k in (2, 3):
        _check(v, t, sr.lattice_grid((0, 0, 0), (1, 1, 1), n, k), **kw)


def test_attributes_across_the_group_edge():
    v, t, n = sr.mesh("noise40")
    nrm, col, ids = sr.attributes(len(v), seed=6)
    _check(v, t, sr.lattice_grid((0, 0, 0), (1, 1, 1), n, 4), nrm, col, ids)     # up to 116 members per cell


def test_a_mesh_argument_carries_its_attributes():
    from focnerf_amd import Mesh, simplify_mesh
    v, t, n = sr.mesh("noise12")
    nrm, col, ids = sr.attributes(len(v), seed=7)
    origin, cell, dims = sr.lattice_grid((0, 0, 0), (1, 1, 1), n, 2)
    got = _host(simplify_mesh(Mesh(_dev(v), _dev(t), _dev(nrm), _dev(col), _dev(ids)), cell=cell, origin=origin, dims=dims))
    assert sr.same(got, sr.simplify(v, t, origin, cell, dims, nrm, col, ids))


def test_unique():
    v, t, n = sr.mesh("noise12")
    want = _check(v, t, sr.lattice_grid((0, 0, 0), (1, 1, 1), n, 3), unique=True)
    assert len(want.triangles) == 186


def test_derived_grid_covers_the_mesh():
    from focnerf_amd import simplify_mesh
    v, t, _, _ = _world_sphere()
    got = _host(simplify_mesh(_dev(v), _dev(t), cell=0.17))
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    dims = tuple(int(g) for g in np.floor((hi - lo) / np.float64(np.float32(0.17))) + 1)
    assert sr.same(got, sr.simplify(v, t, v.min(0), 0.17, dims))


# ---------------------------------------------------------------- refusals: the device's counted flags
def test_refusals_found_on_the_device():
    v, t, _, _ = _world_sphere()
    grid = ((-1, -1, -1), 0.25, (8, 8, 8))
    bad = v.copy()
    bad[1234, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        _run(bad, t, grid)
    bad[1234, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        _run(bad, t, grid)
    for index in (len(v), -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min):
        tt = t.copy()
        tt[len(tt) // 2, 2] = index
        with pytest.raises(ValueError, match="outside"):
            _run(v, tt, grid)
    _check(v, t, grid)                                                   # and the library serves the next call


def test_raw_entry_points_count_the_flags():
    import ctypes
    from focnerf_amd._lib import lib, ptr, stream_of, check
    v, t, _, _ = _world_sphere()
    v, t = v.copy(), t.copy()
    v[[5, 700], 0] = np.nan
    t[[3, 64, 4811]] = [[0, 1, len(v)], [-1, 2, 3], [4, 5, 6]]
    dv, dt = _dev(v), _dev(t)
    org, cel = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(0.25, 0.25, 0.25)
    nbytes = lib.foc_simplify_workspace_bytes(len(v), len(t), 8, 8, 8)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    counts = torch.full((4,), 77, dtype=torch.int32, device=DEV)
    check(lib.foc_simplify_count(ptr(dv), len(v), ptr(dt), len(t), org, cel, 8, 8, 8, ptr(ws), nbytes, ptr(counts), stream_of(dv)))
    assert counts.tolist()[2:] == [2, 2]
    # refused before any launch, the message names the argument
    assert lib.foc_simplify_workspace_bytes(10, 10, 1 << 11, 1 << 10, 1 << 10) == 0
    for args, word in (((org, (ctypes.c_float * 3)(0.25, 0.0, 0.25), 8, 8, 8, ptr(ws), nbytes), "cell3"),
                       ((org, cel, 8, 0, 8, ptr(ws), nbytes), "dims"),
                       ((org, cel, 8, 8, 8, ptr(ws), nbytes - 1), "workspace")):
        assert lib.foc_simplify_count(ptr(dv), len(v), ptr(dt), len(t), *args, ptr(counts), stream_of(dv)) == 1
        assert word in lib.foc_last_error().decode()


# ---------------------------------------------------------------- determinism
def test_two_calls_and_the_deterministic_mode_give_the_same_bits():
    import focnerf_amd
    v, t, n = sr.mesh("noise40")
    nrm, col, ids = sr.attributes(len(v), seed=8)
    grid = sr.lattice_grid((0, 0, 0), (1, 1, 1), n, 3)
    a, b = _run(v, t, grid, nrm, col, ids), _run(v, t, grid, nrm, col, ids)
    with focnerf_amd.deterministic():
        c = _run(v, t, grid, nrm, col, ids)
    for other in (b, c):
        for name in ("vertices", "triangles", "vertex_map", "members", "normals", "colors", "object_id"):
            x, y = getattr(a, name), getattr(other, name)
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ---------------------------------------------------------------- the simplify= keyword
RES = 24


@pytest.fixture(scope="module")
def model():
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(3)
    m = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


@pytest.fixture(scope="module")
def threshold(model):
    from focnerf_amd import mesh
    return float(mesh.density_volume(model, RES).median())


def test_extract_geometry_simplify_is_simplify_mesh_on_the_lattice_grid(model, threshold):
    from focnerf_amd import mesh, simplify_mesh
    from focnerf_amd.simplify import lattice_grid
    v, f, n = mesh.extract_geometry(model, RES, threshold, normals=True)
    assert f.shape[0] > 64
    origin, cell, dims = lattice_grid(*mesh.world_map(model.aabb_infer, RES), RES, 2)
    want = simplify_mesh(v, f, cell=cell, origin=origin, dims=dims, normals=n)
    got = mesh.extract_geometry(model, RES, threshold, normals=True, simplify=2)
    assert 0 < want.triangles.shape[0] < f.shape[0]
    for a, b in zip(got, (want.vertices, want.triangles, want.normals)):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the same grid in the numpy statement, from the lattice's own numbers
    ref = sr.simplify(v.cpu().numpy(), f.cpu().numpy(), *sr.lattice_grid(*mesh.world_map(model.aabb_infer, RES), RES, 2))
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref.vertices.view(np.uint32)) and np.array_equal(got[1].cpu().numpy(), ref.triangles)
    # without normals, and with the field's own at the new vertices
    v2, f2 = mesh.extract_geometry(model, RES, threshold, simplify=2)
    assert torch.equal(v2, got[0]) and torch.equal(f2, got[1])
    v3, f3, n3 = mesh.extract_geometry(model, RES, threshold, normals="field", simplify=2)
    from focnerf_amd.normals import density_gradient
    assert torch.equal(v3, got[0]) and torch.equal(f3, got[1])
    assert torch.equal(n3, mesh.unit_normals(density_gradient(model, v3)[1]))


def test_simplify_none_is_todays_output(model, threshold):
    from focnerf_amd import mesh
    a = mesh.extract_geometry(model, RES, threshold, normals=True)
    b = mesh.extract_geometry(model, RES, threshold, normals=True, simplify=None)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for bad in (1, 0, -2, 2.0, "2", True):
        with pytest.raises(ValueError, match="simplify"):
            mesh.extract_geometry(model, RES, threshold, simplify=bad)


def test_extract_mesh_simplify_carries_the_query_at_the_new_vertices(model, threshold):
    from focnerf_amd import mesh, query_scene
    v, f = mesh.extract_geometry(model, RES, threshold, simplify=2)
    m = mesh.extract_mesh(model, RES, threshold, simplify=2)
    assert torch.equal(m.vertices, v) and torch.equal(m.triangles, f)
    s = query_scene([model], [None], v)
    assert torch.equal(m.normals, s.normal) and torch.equal(m.colors, s.rgb) and torch.equal(m.object_id, s.object_id)


def test_scene_extractors_take_simplify(model, threshold):
    from focnerf_amd import mesh, Placement, simplify_mesh
    from focnerf_amd.simplify import lattice_grid
    box = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    P = [Placement.rotated((0, 0, 1), 90, translation=(0.4, -0.2, 0.1), scale=0.5)]
    v, f = mesh.extract_scene_geometry([model], P, box, RES, threshold)
    origin, cell, dims = lattice_grid(*mesh.world_map(box, RES), RES, 3)
    want = simplify_mesh(v, f, cell=cell, origin=origin, dims=dims)
    got = mesh.extract_scene_geometry([model], P, box, RES, threshold, simplify=3)
    assert torch.equal(got[0], want.vertices) and torch.equal(got[1], want.triangles) and want.triangles.shape[0] > 0
    m = mesh.extract_scene_mesh([model], P, box, RES, threshold, simplify=3)
    assert torch.equal(m.vertices, want.vertices) and torch.equal(m.triangles, want.triangles) and m.object_id.shape[0] == want.vertices.shape[0]


def test_save_mesh_simplify_round_trips(model, threshold, tmp_path):
    from focnerf_amd import mesh
    v, f = mesh.extract_geometry(model, RES, threshold, simplify=2)
    path = str(tmp_path / "small.ply")
    assert mesh.save_mesh(model, path, RES, threshold, simplify=2) == (v.shape[0], f.shape[0])
    rv, rf, _ = mesh.read_ply(path)
    assert np.array_equal(rv.view(np.uint32), v.cpu().numpy().view(np.uint32)) and np.array_equal(rf, f.cpu().numpy())
    assert mesh.save_mesh(model, path, RES, threshold, colors=True, simplify=2) == (v.shape[0], f.shape[0])
    assert mesh.read_ply(path)[0].shape[0] == v.shape[0] and "colors" in mesh.read_ply_attributes(path)
