"""Pins tests/simplify_ref.py, the numpy statement of the vertex clustering that csrc/simplify.hip is held to (tests/test_gpu_simplify.py):
against a second formulation with exact fractions, against six plausible misreadings of the rule, and against the invariants the rule
promises. CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402
import simplify_ref as sr                                                # noqa: E402

UNIT = ((0, 0, 0), (1, 1, 1))
SPACING = np.float32(2 / 31)


def _lattice(name, k):
    v, t, n = sr.mesh(name)
    return v, t, sr.lattice_grid(*UNIT, n, k)


def _world_sphere():
    v, t, n = sr.mesh("sphere")
    return (np.float32(-1) + v * SPACING).astype(np.float32), t, n


# the cases the mutants are run on: name -> (vertices, triangles, grid)
def _cases():
    w, t, n = _world_sphere()
    out = {"sphere_k3": _lattice("sphere", 3), "noise12_k2": _lattice("noise12", 2), "torus_k4": _lattice("torus", 4),
           "world_k2": (w, t, sr.lattice_grid((-1, -1, -1), (SPACING,) * 3, n, 2)),
           "three_cells": (w, t, ((-0.93, -1.07, -0.81), (0.137, 0.093, 0.211), (14, 23, 9))),
           "small_grid": (w, t, ((-0.4, -0.35, -0.3), (0.11, 0.13, 0.09), (7, 5, 6)))}
    return out


# ---------------------------------------------------------------- a second formulation
@pytest.mark.parametrize("case", ["noise12_k2", "sphere_k3", "three_cells", "small_grid"])
def test_brute_force_with_exact_fractions(case):
    v, t, grid = _cases()[case]
    nrm, col, ids = sr.attributes(len(v), seed=3, wild=True)
    a, b = sr.simplify(v, t, *grid, nrm, col, ids), sr.brute_force(v, t, *grid, nrm, col, ids)
    assert len(a.triangles) > 0 and sr.same(a, b)


def test_brute_force_on_tiny_meshes():
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.6, 0.4, 0.5], [9.0, -3.0, 0.25]], dtype=np.float32)
    for tris in ([[2, 0, 1]], [[0, 3, 2]], [[2, 0, 1], [1, 3, 2], [4, 1, 2]], []):
        t = np.array(tris, dtype=np.int32).reshape(-1, 3)
        assert sr.same(sr.simplify(v, t, (0, 0, 0), 1.0, (2, 2, 1)), sr.brute_force(v, t, (0, 0, 0), 1.0, (2, 2, 1)))
    one = sr.simplify(v, np.array([[2, 0, 1]], dtype=np.int32), (0, 0, 0), 1.0, (2, 2, 1))
    assert one.triangles.tolist() == [[0, 2, 1]] and one.members.tolist() == [2, 1, 2] and one.vertex_map.tolist() == [0, 2, 1, 0, 2]
    assert np.array_equal(one.vertices[0], np.array([0.55, 0.45, 0.5], dtype=np.float32))
    assert np.array_equal(one.vertices[2], np.array([1.75, 0.25, 0.375], dtype=np.float32))      # the outside vertex lies on the border
    none = sr.simplify(v, np.array([[0, 3, 2]], dtype=np.int32), (0, 0, 0), 1.0, (2, 2, 1))
    assert len(none.vertices) == 0 and len(none.triangles) == 0 and (none.vertex_map == -1).all()


# ---------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", sr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = []
    for name, (v, t, grid) in _cases().items():
        if not sr.same(sr.simplify(v, t, *grid), sr.simplify(v, t, *grid, mutant=mutant)):
            caught.append(name)
    print(mutant, "caught by", caught)
    assert caught, f"no case tells the rule from its mutant {mutant!r}"


# ---------------------------------------------------------------- the table of the issue, and the invariants
TABLE = {("sphere", 2): (538, 1072), ("sphere", 3): (247, 490), ("sphere", 4): (133, 262),
         ("torus", 2): (774, 1548), ("torus", 3): (374, 778), ("torus", 4): (222, 444),
         ("noise40", 2): (7991, 38184), ("noise40", 3): (2197, 16306), ("noise40", 4): (1000, 9288),
         ("noise12", 2): (212, 514), ("noise12", 3): (64, 188), ("noise12", 4): (27, 86)}
MANIFOLD = {("sphere", 2): 2, ("sphere", 3): 2, ("sphere", 4): 2, ("torus", 2): 0, ("torus", 4): 0}       # Euler characteristic where manifold
SPHERE_VOLUME_RATIO = {2: 0.9833820618040109, 3: 0.9580490767593629, 4: 0.9195175624440775}           # what this statement gives


def _invariants(v, t, grid, res):
    assert mesh_ref.is_closed(res.triangles)                            # with multiplicity: the input is closed
    assert np.array_equal(np.unique(res.triangles), np.arange(len(res.vertices)))     # no unreferenced output vertex
    assert int(res.members.sum()) == int((res.vertex_map >= 0).sum())
    assert (res.triangles[:, 0] < res.triangles[:, 1]).all() and (res.triangles[:, 0] < res.triangles[:, 2]).all()
    origin, cell, inv, dims = sr.grid(*grid)
    c, r, k = sr.cells(v, origin, cell, inv, dims)
    c_raw = sr.cells(v, origin, cell, inv, dims, mutant="noclamp")[0]
    inside = (c_raw == c).all(-1)                                        # vertices the clamp did not move
    cell_c = np.zeros((len(res.vertices), 3), dtype=np.int64)
    cell_c[res.vertex_map[res.vertex_map >= 0]] = c[res.vertex_map >= 0]
    clamped_cell = np.zeros(len(res.vertices), dtype=bool)
    clamped_cell[res.vertex_map[(res.vertex_map >= 0) & ~inside]] = True
    lo = origin.astype(np.float64) + cell_c * cell.astype(np.float64)
    hi = lo + cell.astype(np.float64)
    x = res.vertices.astype(np.float64)
    slack = np.abs(hi).max() * 2.0 ** -23                                # the one fp32 rounding of the stored coordinate
    ok = ((x >= lo - slack) & (x <= hi + slack)).all(-1)
    assert ok[~clamped_cell].all()


@pytest.mark.parametrize("name,k", sorted(TABLE))
def test_table_and_invariants(name, k):
    v, t, grid = _lattice(name, k)
    assert mesh_ref.is_closed(t)
    res = sr.simplify(v, t, *grid)
    assert (len(res.vertices), len(res.triangles)) == TABLE[name, k]
    _invariants(v, t, grid, res)
    if (name, k) in MANIFOLD:
        assert mesh_ref.is_manifold(res.triangles) and mesh_ref.euler_characteristic(len(res.vertices), res.triangles) == MANIFOLD[name, k]
    if name == "sphere":
        ratio = mesh_ref.signed_volume(res.vertices, res.triangles) / mesh_ref.signed_volume(v, t)
        assert abs(ratio - SPHERE_VOLUME_RATIO[k]) <= 2.0 ** -23


def test_table_details():
    v, t, grid = _lattice("sphere", 3)
    res = sr.simplify(v, t, *grid)
    occupied = len(np.unique(sr.cells(v, *sr.grid(*grid))[2]))
    assert occupied == 248 and int((res.vertex_map < 0).sum()) == 5      # a cell all of whose triangles collapsed: kept cells are defined by triangles
    v, t, grid = _lattice("torus", 3)
    res = sr.simplify(v, t, *grid)
    assert mesh_ref.is_closed(res.triangles) and not mesh_ref.is_manifold(res.triangles)
    v, t, grid = _lattice("noise40", 2)
    assert len(np.unique(sr.cells(v, *sr.grid(*grid))[2])) == 7993 and grid[2] == (20, 20, 20)
    v, t, grid = _lattice("noise40", 4)
    assert sr.simplify(v, t, *grid).members.max() == 116
    v, t, grid = _lattice("noise12", 3)
    u = sr.simplify(v, t, *grid, unique=True).triangles
    assert len(u) == 186 and np.array_equal(u, np.unique(sr.simplify(v, t, *grid).triangles, axis=0))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_world_units_give_the_same_counts(k):
    w, t, n = _world_sphere()
    grid = sr.lattice_grid((-1, -1, -1), (SPACING,) * 3, n, k)
    res = sr.simplify(w, t, *grid)
    assert (len(res.vertices), len(res.triangles)) == TABLE["sphere", k]
    _invariants(w, t, grid, res)


def test_clamped_and_odd_grids_keep_the_invariants():
    for name in ("three_cells", "small_grid"):
        v, t, grid = _cases()[name]
        _invariants(v, t, grid, sr.simplify(v, t, *grid))


def test_refusals_of_the_statement():
    v, t, grid = _lattice("noise12", 2)
    bad = v.copy()
    bad[7, 2] = np.nan
    for args in ((bad, t, *grid), (v, np.where(t == 5, len(v), t), *grid), (v, np.where(t == 5, -1, t), *grid),
                 (v, t, grid[0], (1.0, 0.0, 1.0), grid[2]), (v, t, grid[0], np.nan, grid[2]), (v, t, grid[0], grid[1], (1 << 11, 1 << 10, 1 << 10)),
                 (v, t, grid[0], grid[1], (4, 0, 4))):
        with pytest.raises(ValueError):
            sr.simplify(*args)


# ---------------------------------------------------------------- the public interface (fails before this feature exists)
def test_public_interface():
    import torch
    import focnerf_amd
    from focnerf_amd import _lib, mesh
    assert {"foc_simplify_workspace_bytes", "foc_simplify_count", "foc_simplify_emit"} <= set(_lib.SIGNATURES)
    assert issubclass(focnerf_amd.SimplifiedMesh, focnerf_amd.Mesh)
    v, t = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        focnerf_amd.simplify_mesh(v, t, cell=1.0)                        # a CPU tensor
    with pytest.raises(ValueError, match="float32"):
        focnerf_amd.simplify_mesh(v.double(), t, cell=1.0)               # a wrong dtype
    for cell in (0.0, -1.0, float("nan"), float("inf"), (1.0, 1.0), None):
        with pytest.raises(ValueError, match="cell"):
            focnerf_amd.simplify_mesh(v, t, cell=cell)
    for fn, args in ((mesh.extract_geometry, (None,)), (mesh.extract_scene_geometry, (None, None, None)), (mesh.extract_mesh, (None,)),
                     (mesh.extract_scene_mesh, (None, None, None)), (lambda *a, **kw: mesh.save_mesh(*a, "x.ply", **kw), (None,))):
        for bad in (1, 0, 2.5, "2", True):
            with pytest.raises(ValueError, match="simplify"):
                fn(*args, simplify=bad)
    from focnerf_amd.simplify import lattice_grid
    o, c, d = lattice_grid(*mesh.world_map([-1, -1, -1, 1, 1, 1], 32), 32, 3)
    ro, rc, rd = sr.lattice_grid((-1, -1, -1), (SPACING,) * 3, 32, 3)
    assert np.array_equal(o, ro) and np.array_equal(c.view(np.uint32), rc.view(np.uint32)) and tuple(d) == tuple(rd) == (11, 11, 11)
