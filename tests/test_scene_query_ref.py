"""CPU: the scene point query's reference (tests/scene_query_ref.py) pinned against the lattice cull's, its select against deliberately
wrong variants, the host-side refusals of the new entry points, the PLY writer's new properties and the exports. The device kernels are
compared against the same reference in tests/test_gpu_scene_query.py."""
import ctypes
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402
import scene_query_ref as Q                                              # noqa: E402
from focnerf_amd import query                                            # noqa: E402  (what the reference states; the kernels need no GPU to refuse)

H = 128


@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("placed", [False, True])
def test_point_cull_on_lattice_points_is_the_lattice_cull(bound, placed):
    from focnerf_amd import Placement
    res, cascade = (5, 3, 67), bound
    xs, ys, zs = (np.linspace(-bound, bound, r, dtype=np.float32) for r in res)
    pts = mesh_ref.lattice_points(xs, ys, zs)
    w2o = Placement.rotated((0, 0, 1), 90, translation=(0.8 * bound, 0.7 * bound, 0.9 * bound), scale=0.5).world_to_object() if placed else None
    box = [-bound] * 3 + [bound] * 3 if placed else None
    bits = np.random.default_rng(5).integers(0, 256, cascade * H ** 3 // 8, dtype=np.uint8)
    for bitfield in (None, bits):
        for first, count in ((0, len(pts)), (100, 333)):
            kw = dict(bound=float(bound), bitfield=bitfield, cascade=cascade, H=H) if bitfield is not None else {}
            rmask, roffsets, rpos = mesh_ref.lattice_cull(xs, ys, zs, first, count, w2o, box, **kw)
            mask, offsets, pos, xn = Q.points_cull(pts[first:first + count], w2o, box, **(kw or dict(bound=float(bound))))
            assert np.array_equal(mask, rmask) and np.array_equal(offsets, roffsets)
            assert np.array_equal(pos.view(np.uint32), rpos.view(np.uint32))
            assert len(pos) <= count <= query.MAX_POINTS and (first or 0 < len(pos)) and Q.unpack(mask, count).sum() == len(pos) == offsets[-1]
            assert np.array_equal(xn, ((pos + np.float32(bound)) / np.float32(2 * bound)).astype(np.float32)) and xn.dtype == np.float32


def test_point_cull_never_keeps_a_nan_in_a_box_and_keeps_the_faces():
    w2o = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
    box = [-1, -1, -1, 1, 1, 1]
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0], [1, -1, 1], [1.0000001, 0, 0], [0, 0, -np.inf], [-1, 0.5, 1]], np.float32)
    mask, offsets, pos, xn = Q.points_cull(pts, w2o, box, bound=1.0)
    assert Q.unpack(mask, len(pts)).tolist() == [True, False, False, True, False, False, True]
    assert offsets.tolist() == [0, 3] and xn[1].tolist() == [1.0, 0.0, 1.0]
    assert len(pts) <= query.MAX_POINTS == 1 << 29
    ones = np.full(H ** 3 // 8, 255, np.uint8)
    assert np.array_equal(Q.points_cull(pts, w2o, box, 1.0, ones, 1, H)[0], mask)         # the cell of a rejected point is never computed


def test_select_rules_and_mutants():
    n, keeps, sig, gains = Q.select_case()[:4]
    assert callable(query.scene_select)                                  # the wrapper of the kernel these rules are stated for
    _run_select = Q.run_select
    bs, bi, br, bn = _run_select()
    assert bi[0] == 0 and bs[0] == sig[0][0]                             # the tie: the earlier object stays
    assert bi[1] == 0 and not np.isnan(bs).any()                         # a NaN never wins
    assert bi[2] == -1 and bs[2] == 0 and not np.signbit(bs[2]) and (br[2] == 0).all()
    assert bi[3] == 1 and np.isinf(bs[3])
    assert bi[4] == 1 and bs[4] == 1.5
    assert bi[5] == 0 and bs[5] == sig[0][5] and float(bs[5]) != float(np.float32(0.3)) * float(sig[2][5])     # the product was rounded to fp32
    none = ~(keeps[0] | keeps[1] | keeps[2])
    init = Q.select_case()[6]
    assert none.sum() > 1 and all(np.array_equal(got[none].view(np.uint32), was[none].view(np.uint32)) for got, was in zip((bs, bi, br, bn), init))
    assert (bs[none].view(np.uint32) == 0xDEADBEEF).all() and (bi[~none][bi[~none] < 0] == -1).all()
    for payload in ((True, False), (False, True), (False, False)):     # NULL payload pairs: the rest is unchanged
        ps, pi, pr, pn = Q.run_select(payload=payload)
        assert np.array_equal(ps.view(np.uint32), bs.view(np.uint32)) and np.array_equal(pi, bi)
        assert (pr is None) == (not payload[0]) and (pn is None) == (not payload[1])
    winners = np.stack([np.where(keeps[k], gains[k] * sig[k], -np.inf) for k in range(3)])
    plain = ~np.isnan(winners).any(0) & (winners.max(0) > 0) & ((winners == winners.max(0)).sum(0) == 1)
    assert plain.sum() > 80 and np.array_equal(bi[plain], winners.argmax(0)[plain]) and np.array_equal(bs[plain], winners.max(0)[plain].astype(np.float32))
    for mutant in Q.MUTANTS:
        ms, mi, mr, mn = _run_select(mutant)
        same = np.array_equal(ms, bs, equal_nan=True) and np.array_equal(mi, bi) and np.array_equal(mr, br) and np.array_equal(mn, bn)
        assert not same, mutant
    assert _run_select("ge")[1][0] == 1 and _run_select("ge")[1][2] != -1
    assert np.isnan(_run_select("nan_wins")[0][1])
    assert _run_select("gain_after")[1][4] == 2


def test_surface_frame_reference():
    g = np.array([[3, 0, 4], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-30, -2e-30, 2e-30], [1e38, 1e38, -1e38]], np.float32)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    q = Q.surface_frame(g, rot9=R)
    assert (query.MODE_NORMAL, query.MODE_EYE) == (0, 1)                 # foc_surface_frame's modes, as the reference's eye_obj=None / given
    assert np.allclose(q["normal"][0], [0, -0.6, -0.8]) and np.allclose(q["dirs"][0], [0.6, 0, 0.8])
    for row in (1, 2, 3):
        assert (q["normal"][row] == 0).all() and q["dirs"][row].tolist() == [0, 0, -1] and (q["normal_bound"][row] == 0).all()
    assert np.allclose(np.linalg.norm(q["normal"][4:], axis=-1), 1) and np.allclose(q["normal"][5], np.array([1, -1, 1]) / np.sqrt(3))
    assert (q["dirs_bound"][0] == 2 * 2.0 ** -24 * Q.N_NORMALISE).all() and q["normal_bound"][0].max() < 32 * 2.0 ** -24
    pos = np.array([[1, 2, 3], [0.5, 0.5, 0.5], [np.inf, 0, 0], [1, 1, 1]], np.float32)
    e = Q.surface_frame(np.zeros((4, 3), np.float32), pos, None, np.array([0.5, 0.5, 0.5], np.float32))
    assert np.allclose(e["dirs"][0], np.array([0.5, 1.5, 2.5]) / np.linalg.norm([0.5, 1.5, 2.5]))
    assert e["dirs"][1].tolist() == [0, 0, -1] and e["dirs"][2].tolist() == [0, 0, -1] and (e["normal"] == 0).all()
    assert 0 < e["dirs_bound"][0].max() < 64 * 2.0 ** -24 and (e["dirs_bound"][1] == 0).all()
    c = Q.surface_frame(g[:1], grad_bound=0.05)                          # a carried bound: 2 * 0.05 / 5
    assert np.allclose(c["normal_bound"][0], 0.02 + 2 * 2.0 ** -24 * Q.N_NORMALISE)


def test_new_entry_points_refuse_on_the_host_without_a_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib
    assert _lib.lib.foc_abi_version() == 2
    one = ctypes.c_void_p(8)                                             # never dereferenced: validation fails first
    w2o = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    w2o_bad = (ctypes.c_float * 12)(*([float("inf")] + [0] * 11))
    box = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    box_bad = (ctypes.c_float * 6)(-1, -1, float("nan"), 1, 1, 1)
    args = dict(points=one, M=64, w2o=None, box=None, bound=1.0, bits=None, cascade=1, grid=128, mask=one, offsets=one, n_out=one, scratch=one, nbytes=4)

    def cull(**kw):
        a = dict(args, **kw)
        return lib.foc_points_cull(a["points"], a["M"], a["w2o"], a["box"], a["bound"], a["bits"], a["cascade"], a["grid"], a["mask"], a["offsets"],
                                   a["n_out"], a["scratch"], a["nbytes"], None)

    def refused(rc, text):
        return rc == 1 and text in lib.foc_last_error()                  # FOC_E_INVALID, with a message
    assert cull(M=0) == 0 and cull(M=0, points=None) == 0                # nothing to do, nothing enqueued
    for name in ("points", "mask", "offsets", "n_out", "scratch"):
        assert refused(cull(**{name: None}), b"null pointer"), name
    assert refused(cull(M=(1 << 29) + 1, nbytes=1 << 20), b"2^29")
    assert refused(cull(w2o=w2o), b"come together") and refused(cull(box=box), b"come together")
    assert refused(cull(w2o=w2o_bad, box=box), b"non-finite") and refused(cull(w2o=w2o, box=box_bad), b"non-finite")
    assert refused(cull(bits=one, grid=100), b"power of two") and refused(cull(bits=one, cascade=17), b"cascade")
    assert refused(cull(bits=one, bound=float("nan")), b"bound")
    assert refused(cull(nbytes=3), b"scratch of") and refused(cull(M=4097, nbytes=4), b"scratch of")

    def emit(points=one, M=64, w=None, bound=1.0, mask=one, offsets=one, m_occ=5, pos=one, xn=one):
        return lib.foc_points_cull_emit(points, M, w, bound, mask, offsets, m_occ, pos, xn, None)
    assert emit(M=0) == 0 and emit(m_occ=0) == 0 and emit(pos=None, xn=None) == 0
    assert refused(emit(points=None), b"null pointer") and refused(emit(mask=None), b"null pointer") and refused(emit(offsets=None), b"null pointer")
    assert refused(emit(M=(1 << 29) + 1), b"2^29") and refused(emit(m_occ=65), b"m_occ")
    assert refused(emit(w=w2o_bad), b"non-finite") and refused(emit(bound=0.0), b"bound") and refused(emit(bound=float("inf")), b"bound")

    eye = (ctypes.c_float * 3)(0, 0, 3)
    eye_bad = (ctypes.c_float * 3)(0, float("nan"), 3)
    rot = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    rot_bad = (ctypes.c_float * 9)(*([float("inf")] + [0] * 8))

    def frame(g=one, pos=one, m=5, r=None, mode=0, e=None, dirs=one, normal=one):
        return lib.foc_surface_frame(g, pos, m, r, mode, e, dirs, normal, None)
    assert frame(m=0) == 0 and frame(dirs=None, normal=None) == 0
    assert refused(frame(mode=2), b"mode") and refused(frame(g=None), b"null pointer") and refused(frame(g=None, mode=1, e=eye), b"null pointer")
    assert refused(frame(mode=1, e=None), b"null pointer") and refused(frame(mode=1, e=eye, pos=None), b"null pointer")
    assert refused(frame(mode=1, e=eye_bad), b"non-finite") and refused(frame(r=rot_bad), b"non-finite")
    assert refused(frame(m=(1 << 29) + 1, r=rot), b"2^29")

    def select(sigma=one, rgb=one, nrm=one, mask=one, offsets=one, gain=1.0, k=0, bs=one, bi=one, br=one, bn=one, n=64):
        return lib.foc_scene_select(sigma, rgb, nrm, mask, offsets, gain, k, bs, bi, br, bn, n, None)
    assert select(n=0) == 0
    for name in ("sigma", "mask", "offsets", "bs", "bi"):
        assert refused(select(**{name: None}), b"null pointer"), name
    assert refused(select(rgb=None), b"pairs") and refused(select(bn=None), b"pairs")
    assert refused(select(gain=0.0), b"gain") and refused(select(gain=float("nan")), b"gain") and refused(select(n=(1 << 29) + 1), b"2^29")


def _expected_ply(v, f, n=None, c=None, ids=None):
    """The file's bytes, built from the format."""
    props = ["x", "y", "z"] + (["nx", "ny", "nz"] if n is not None else [])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {p}" for p in props]
    if c is not None:
        head += [f"property uchar {p}" for p in ("red", "green", "blue")]
    if ids is not None:
        head += ["property int object_id"]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    out = ("\n".join(head) + "\n").encode("ascii")
    for i in range(len(v)):
        out += struct.pack("<3f", *v[i])
        if n is not None:
            out += struct.pack("<3f", *n[i])
        if c is not None:
            out += struct.pack("<3B", *c[i])
        if ids is not None:
            out += struct.pack("<i", ids[i])
    for t in f:
        out += struct.pack("<B3i", 3, *t)
    return out


def test_write_ply_old_arguments_byte_identical_and_the_new_properties_round_trip(tmp_path):
    from focnerf_amd import mesh
    rng = np.random.default_rng(2)
    v, n = rng.standard_normal((7, 3)).astype(np.float32), rng.standard_normal((7, 3)).astype(np.float32)
    f = rng.integers(0, 7, (5, 3)).astype(np.int32)
    c = rng.integers(0, 256, (7, 3)).astype(np.uint8)
    ids = np.array([0, 1, -1, 2, 0, 1, 1], np.int32)
    path = str(tmp_path / "m.ply")
    for nrm in (None, n):
        mesh.write_ply(path, v, f, nrm)
        assert open(path, "rb").read() == _expected_ply(v, f, nrm)
        assert mesh.read_ply_attributes(path) == {}
    for nrm, col, oid in ((n, c, ids), (None, c, None), (None, None, ids), (n, None, ids)):
        mesh.write_ply(path, v, f, nrm, colors=col, object_id=oid)
        assert open(path, "rb").read() == _expected_ply(v, f, nrm, col, oid)
        rv, rf, rn = mesh.read_ply(path)
        assert np.array_equal(rv, v) and np.array_equal(rf, f) and ((rn is None) if nrm is None else np.array_equal(rn, nrm))
        attrs = mesh.read_ply_attributes(path)
        assert set(attrs) == {k for k, a in (("colors", col), ("object_id", oid)) if a is not None}
        assert col is None or (np.array_equal(attrs["colors"], col) and attrs["colors"].dtype == np.uint8)
        assert oid is None or (np.array_equal(attrs["object_id"], oid) and attrs["object_id"].dtype == np.int32)
    fc = np.array([[0.0, 1.0, 0.5], [-1.0, 2.0, np.nan], [0.49803922, 0.001, 0.999]] + [[0.25, 0.25, 0.25]] * 4, np.float32)
    mesh.write_ply(path, v, f, colors=fc)                                # floats: floor(clamp(c, 0, 1) * 255 + 0.5), a NaN -> 0
    got = mesh.read_ply_attributes(path)["colors"]
    assert got[:3].tolist() == [[0, 255, 128], [0, 255, 0], [127, 0, 255]] and got[3].tolist() == [64, 64, 64]
    with pytest.raises(ValueError):
        mesh.write_ply(path, v, f, colors=c[:3])
    with pytest.raises(ValueError):
        mesh.write_ply(path, v, f, object_id=ids[:3])


def test_mesh_colors_u8_and_exports():
    import torch
    import focnerf_amd
    from focnerf_amd import mesh, query
    for name, home in (("query_scene", query), ("SceneSample", query), ("Mesh", mesh), ("extract_mesh", mesh), ("extract_scene_mesh", mesh),
                       ("read_ply_attributes", mesh)):
        assert getattr(focnerf_amd, name) is getattr(home, name) and name in focnerf_amd.__all__
    for name in ("foc_points_cull", "foc_points_cull_emit", "foc_surface_frame", "foc_scene_select"):
        assert name in focnerf_amd._lib.SIGNATURES and hasattr(focnerf_amd._lib.lib, name)
    m = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), colors=torch.tensor([[0.0, 1.0, 0.5], [-1.0, 2.0, float("nan")], [0.49803922, 0.001, 0.999]]))
    assert m.colors_u8.dtype == torch.uint8 and m.colors_u8.tolist() == [[0, 255, 128], [0, 255, 0], [127, 0, 255]]
    assert mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)).colors_u8 is None
    with pytest.raises(ValueError):
        query.query_scene([], [], torch.zeros(4, 3))
    with pytest.raises(ValueError, match="not served for a scene"):
        mesh.extract_scene_geometry([], [], [-1] * 3 + [1] * 3, normals="field")
    assert "extract_scene_mesh" in mesh.extract_scene_geometry.__doc__ and "capturable" in query.query_scene.__doc__
