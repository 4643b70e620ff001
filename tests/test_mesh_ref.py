"""CPU: the marching-cubes case table and its float64 reference (tests/mesh_ref.py) on volumes with known answers, the PLY writer, the
host-side refusals of the mesh entry points and the mcubes drop-in's interface. The device kernels are compared against the same
reference in tests/test_gpu_mesh.py."""
import ctypes
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402
import make_mc_table                                                     # noqa: E402  (tools/, put on the path by mesh_ref)

HEADER = os.path.join(REPO, "focnerf_amd", "csrc", "mc_table.h")


def _header_tables():
    text = open(HEADER).read()
    ntri = [int(v) for v in re.search(r"MC_NTRI\[256\] = \{(.*?)\};", text, re.S).group(1).replace("\n", " ").split(",") if v.strip()]
    body = re.search(r"MC_TRI\[256\]\[3 \* MC_MAX_TRIS\] = \{(.*)\};", text, re.S).group(1)
    rows = [[int(v) for v in r.split(",")] for r in re.findall(r"\{([^}]*)\}", body)]
    corner = [int(v) for v in re.search(r"MC_EDGE_CORNER\[12\] = \{(.*?)\};", text).group(1).split(",")]
    return np.array(ntri), np.array(rows), np.array(corner)


def test_case_table_regenerates_byte_identically_and_is_the_references():
    assert open(HEADER).read() == make_mc_table.header_text()
    ntri, rows, corner = _header_tables()
    assert ntri.shape == (256,) and rows.shape == (256, 15)
    assert np.array_equal(ntri, mesh_ref.NTRI) and np.array_equal(rows, mesh_ref.TRI) and np.array_equal(corner, mesh_ref.EDGE_CORNER)
    assert ntri[0] == 0 and ntri[255] == 0
    assert {k: int((ntri == k).sum()) for k in range(6)} == {0: 2, 1: 16, 2: 50, 3: 80, 4: 76, 5: 32}
    assert int(ntri.sum()) == 820
    for case in range(256):                                              # a row holds its count of triangles, then padding
        assert (rows[case, :3 * ntri[case]] >= 0).all() and (rows[case, 3 * ntri[case]:] == -1).all()


def test_edge_numbering_is_axis_major_by_lower_corner():
    assert make_mc_table.EDGES == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]


def _cases_present(vol, thr):
    inside = vol >= thr
    n = vol.shape[0] - 1
    case = np.zeros((n, n, n), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[ox:ox + n, oy:oy + n, oz:oz + n].astype(np.int64) << c
    return set(np.unique(case).tolist())


@pytest.mark.parametrize("n", [24, 16])
def test_noise_volume_meets_every_case_and_closes(n):
    vol = mesh_ref.noise_volume(n)
    assert _cases_present(vol, 0.5) == set(range(256))                  # what makes the test exhaustive
    v, f = mesh_ref.marching_cubes(vol, 0.5)
    assert len(f) > 0 and f.min() == 0 and f.max() == len(v) - 1
    assert mesh_ref.is_closed(f)                                         # every directed edge as often as its reverse
    assert (v >= 0).all() and (v <= n - 1).all()


@pytest.mark.parametrize("name, chi, lo", [("sphere", 2, 0.97), ("torus", 0, 0.95)])
def test_smooth_volumes_are_manifold_with_the_right_topology_and_volume(name, chi, lo):
    if name == "sphere":
        vol, exact = mesh_ref.sphere_volume(), 4.0 / 3.0 * math.pi * 6.3 ** 3
    else:
        vol, exact = mesh_ref.torus_volume(), 2.0 * math.pi ** 2 * 6.0 * 2.5 ** 2
    v, f = mesh_ref.marching_cubes(vol, 0.0)
    assert mesh_ref.is_manifold(f)
    assert mesh_ref.euler_characteristic(len(v), f) == chi
    ratio = mesh_ref.signed_volume(v, f) / exact                         # positive: the triangles face outward
    print(f"{name}: signed volume / analytic = {ratio:.4f}")
    assert lo < ratio < 1.0


def test_reference_normals_point_outward_on_the_sphere_and_refuses_nan():
    vol = mesh_ref.sphere_volume()
    v, f, nrm = mesh_ref.marching_cubes(vol, 0.0, normals=True)
    centre = (20 - 1) / 2 + np.array([0.13, 0.21, 0.37])
    radial = (v - centre) / np.linalg.norm(v - centre, axis=-1, keepdims=True)
    assert (np.einsum("ij,ij->i", nrm, radial) > 0.99).all()
    bad = vol.copy()
    i = np.argwhere((vol[:-1] >= 0) != (vol[1:] >= 0))[0]
    bad[tuple(i)] = np.nan
    with pytest.raises(ValueError):
        mesh_ref.marching_cubes(bad, 0.0)


def test_origin_and_spacing_of_the_reference():
    vol = mesh_ref.sphere_volume()
    v, f = mesh_ref.marching_cubes(vol, 0.0)
    w, g = mesh_ref.marching_cubes(vol, 0.0, origin=(-1, 2, 0.5), spacing=(0.1, 0.2, 0.3))
    assert np.array_equal(f, g) and np.allclose(w, np.array([-1, 2, 0.5]) + v * np.array([0.1, 0.2, 0.3]), rtol=0, atol=1e-12)


def test_lattice_cull_reference_on_a_hand_made_case():
    xs = np.linspace(-1, 1, 3, dtype=np.float32)
    H = 4
    bits = np.zeros(H ** 3 // 8, dtype=np.uint8)
    index, _, _ = mesh_ref.fixed_cull_ref.cell_index(np.array([[1.0, 1.0, 1.0]], dtype=np.float32), 1.0, 1, H)
    bits[index[0] >> 3] |= 1 << (index[0] & 7)
    mask, offsets, pts = mesh_ref.lattice_cull(xs, xs, xs, bound=1.0, bitfield=bits, cascade=1, H=H)
    # cell 3 of an axis covers [0.5, 1]: of the lattice {-1, 0, 1}^3 only (1, 1, 1), the last point, lies in the set cell
    assert mask.tolist() == [1 << 26] and offsets.tolist() == [0, 1] and pts.tolist() == [[1.0, 1.0, 1.0]]
    mask, offsets, pts = mesh_ref.lattice_cull(xs, xs, xs, first=13, count=14, w2o=[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], obj_aabb=[0, 0, 0, 1, 1, 1])
    assert offsets.tolist() == [0, 8] and len(pts) == 8 and mask[0] == sum(1 << (i - 13) for i in (13, 14, 16, 17, 22, 23, 25, 26))


def test_ply_round_trip(tmp_path):
    from focnerf_amd import mesh
    v, f, nrm = mesh_ref.marching_cubes(mesh_ref.sphere_volume(), 0.0, normals=True)
    for normals in (None, nrm):
        path = str(tmp_path / "m.ply")
        mesh.write_ply(path, v, f, normals)
        head = open(path, "rb").read(400).split(b"end_header\n")[0].decode("ascii").split("\n")
        assert head[:2] == ["ply", "format binary_little_endian 1.0"]
        assert f"element vertex {len(v)}" in head and f"element face {len(f)}" in head
        assert ("property float nx" in head) == (normals is not None)
        size = len("\n".join(head)) + len("end_header\n") + len(v) * (12 if normals is None else 24) + len(f) * 13
        assert os.path.getsize(path) == size
        rv, rf, rn = mesh.read_ply(path)
        assert rv.shape == (len(v), 3) and rf.shape == (len(f), 3)
        assert np.array_equal(rv[0], v[0].astype(np.float32)) and np.array_equal(rv[-1], v[-1].astype(np.float32))
        assert np.array_equal(rf[0], f[0]) and np.array_equal(rf[-1], f[-1]) and np.array_equal(rf, f)
        assert (rn is None) if normals is None else np.array_equal(rn, nrm.astype(np.float32))


def test_mesh_entry_points_refuse_on_the_host_without_a_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)                                             # never dereferenced: validation fails first
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    assert lib.foc_mc_workspace_bytes(2, 2, 2) > 0
    assert lib.foc_mc_workspace_bytes(1, 4, 4) == 0 and b">= 2" in lib.foc_last_error()
    assert lib.foc_mc_workspace_bytes(1024, 1024, 513) == 0 and b"2^29" in lib.foc_last_error()
    assert lib.foc_mc_workspace_bytes(1024, 1024, 512) > 0
    assert lib.foc_mc_workspace_bytes(65536, 65536, 2) == 0             # the product does not wrap
    for dims, msg in (((4, 1, 4), b">= 2"), ((1024, 1024, 513), b"2^29")):
        assert lib.foc_mc_count(one, *dims, 0.5, one, one, None) == 1 and msg in lib.foc_last_error()
        assert lib.foc_mc_emit(one, *dims, 0.5, one, None, None, one, None, one, None) == 1 and msg in lib.foc_last_error()
    assert lib.foc_mc_count(None, 4, 4, 4, 0.5, one, one, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_mc_count(one, 4, 4, 4, 0.5, None, one, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_mc_count(one, 4, 4, 4, 0.5, one, None, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_mc_count(one, 4, 4, 4, float("nan"), one, one, None) == 1 and b"finite" in lib.foc_last_error()
    assert lib.foc_mc_emit(one, 4, 4, 4, 0.5, one, None, None, None, None, one, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_mc_emit(one, 4, 4, 4, 0.5, one, None, None, one, None, None, None) == 1 and b"null pointer" in lib.foc_last_error()
    zero = (ctypes.c_float * 3)(1, 0, 1)
    assert lib.foc_mc_emit(one, 4, 4, 4, 0.5, one, f3, zero, one, None, one, None) == 1 and b"spacing" in lib.foc_last_error()
    # lattice cull
    assert lib.foc_lattice_cull_scratch_bytes(1) == 4 and lib.foc_lattice_cull_scratch_bytes(4097) == 8
    w2o = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    args = dict(xs=one, ys=one, zs=one, r=(4, 4, 4), first=0, count=64, w2o=None, box=None, bound=1.0, bits=None, cascade=1, grid=128,
                mask=one, offsets=one, n_out=one, scratch=one, nbytes=4)

    def cull(**kw):
        a = dict(args, **kw)
        return lib.foc_lattice_cull(a["xs"], a["ys"], a["zs"], *a["r"], a["first"], a["count"], a["w2o"], a["box"], a["bound"], a["bits"], a["cascade"],
                                    a["grid"], a["mask"], a["offsets"], a["n_out"], a["scratch"], a["nbytes"], None)
    assert cull(xs=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert cull(mask=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert cull(first=1) == 1 and b"leaves the lattice" in lib.foc_last_error()
    assert cull(count=0) == 1 and b"empty slab" in lib.foc_last_error()
    assert cull(r=(1024, 1024, 513)) == 1 and b"2^29" in lib.foc_last_error()
    assert cull(w2o=w2o) == 1 and b"come together" in lib.foc_last_error()
    w2o_bad = (ctypes.c_float * 12)(*([float("inf")] + [0] * 11))
    assert cull(w2o=w2o_bad, box=box) == 1 and b"non-finite" in lib.foc_last_error()
    assert cull(bits=one, grid=100) == 1 and b"power of two" in lib.foc_last_error()
    assert cull(bits=one, cascade=0) == 1 and b"cascade" in lib.foc_last_error()
    assert cull(nbytes=3) == 1 and b"scratch of" in lib.foc_last_error()
    assert lib.foc_lattice_cull_emit(one, one, one, 4, 4, 4, 0, 64, None, None, one, 5, one, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_lattice_cull_emit(one, one, one, 4, 4, 4, 1, 64, None, one, one, 5, one, None) == 1 and b"leaves the lattice" in lib.foc_last_error()
    assert lib.foc_volume_scatter_max(None, one, one, 1.0, one, 64, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_volume_scatter_max(one, one, one, 0.0, one, 64, None) == 1 and b"gain" in lib.foc_last_error()
    assert lib.foc_volume_scatter_max(one, one, one, 1.0, one, (1 << 29) + 1, None) == 1 and b"2^29" in lib.foc_last_error()


def test_python_interface_refuses_bad_arguments_without_a_gpu():
    import torch
    import focnerf_amd
    from focnerf_amd import mesh
    for name in ("density_volume", "scene_volume", "marching_cubes", "extract_geometry", "extract_scene_geometry", "write_ply", "save_mesh"):
        assert getattr(focnerf_amd, name) is getattr(mesh, name) and name in focnerf_amd.__all__
    with pytest.raises(ValueError):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)                   # a host tensor: these ops have no CPU implementation
    with pytest.raises(ValueError):
        mesh._res3(1)
    with pytest.raises(ValueError):
        mesh._res3((1024, 1024, 513))
    assert mesh._res3(5) == (5, 5, 5) and mesh._res3((5, 3, 67)) == (5, 3, 67)
    origin, spacing = mesh.world_map([-1, -2, -3, 1, 2, 3], (3, 5, 7))
    assert origin.tolist() == [-1, -2, -3] and spacing.tolist() == [1, 1, 1] and origin.dtype == np.float32
    sig = inspect.signature(mesh.extract_geometry)
    assert sig.parameters["resolution"].default == 256 and sig.parameters["threshold"].default == 10     # the reference's save_mesh defaults
    assert "PyMCubes" in mesh.__doc__ and "not pinned" in mesh.__doc__


def test_mcubes_dropin_imports_with_pymcubes_signature():
    import importlib
    dropin = os.path.join(REPO, "focnerf_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("mcubes", None)
        mcubes = importlib.import_module("mcubes")
        assert os.path.dirname(os.path.abspath(mcubes.__file__)) == os.path.join(dropin, "mcubes")
        assert list(inspect.signature(mcubes.marching_cubes).parameters) == ["u", "isovalue"]
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("mcubes", None)
