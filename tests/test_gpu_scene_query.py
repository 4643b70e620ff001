"""GPU: the scene point query (csrc/mesh.hip foc_points_cull / foc_surface_frame / foc_scene_select, focnerf_amd/query.py) against the
reference of tests/scene_query_ref.py, `query_scene` against the field kernels it sequences, and the attributed meshes end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402
import scene_query_ref as Q                                              # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 128
SCENE = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _np_bits(t, ref):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))


def _floats(values):
    from focnerf_amd.fixedcull import _host_floats
    return _host_floats(np.asarray(values, dtype=np.float32).reshape(-1), len(np.asarray(values).reshape(-1)), "test")


# ---------------------------------------------------------------- cull
def _placement(kind, bound):
    from focnerf_amd import Placement
    if kind == "turned":                                                 # the lattice cull test's: a quarter turn, half size, moved to a corner
        return Placement.rotated((0, 0, 1), 90, translation=(0.8 * bound, 0.7 * bound, 0.9 * bound), scale=0.5)
    return Placement() if kind == "identity" else None                   # identity: q = x, so a point can stand exactly on a face of the box


def _cull_points(M, bound, kind, seed):
    rng = np.random.default_rng(seed)
    pts = ((rng.random((M, 3)) * 2 - 1) * 1.3 * bound).astype(np.float32)
    b = float(bound)
    special = [[b, 0.1, -0.2], [-b, -b, b], [0.3, b, 0.0], [np.nextafter(np.float32(b), np.float32(9)), 0, 0], [0, -1.25 * b, 0], [3 * b, 3 * b, 3 * b]]
    if kind is not None:                                                 # a box rejects these before any cell is computed
        special += [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan, np.nan, np.nan]]
    special = np.array(special, np.float32)[:M]
    pts[M - len(special):] = special                                     # at the END: the last, ragged chunk holds them
    return pts


@pytest.mark.parametrize("M", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("kind", [None, "turned", "identity"])
def test_points_cull_against_the_reference(M, bound, kind):
    from focnerf_amd import query
    from focnerf_amd.fixedcull import Occupancy
    cascade = bound
    pts = _cull_points(M, bound, kind, 17 * M + bound)
    P = _placement(kind, bound)
    w2o = None if P is None else P.world_to_object()
    box = None if P is None else [-bound] * 3 + [bound] * 3
    cw2o, cbox = (None, None) if P is None else (_floats(w2o), _floats(box))
    x = torch.from_numpy(pts).to(DEV)
    _, _, inbox, _ = Q.points_cull(pts, w2o, box)
    cells = cascade * H ** 3
    fields = {"none": None, "zero": np.zeros(cells // 8, np.uint8), "ones": np.full(cells // 8, 255, np.uint8),
              "random": np.random.default_rng(7).integers(0, 256, cells // 8, dtype=np.uint8)}
    if len(inbox):
        c = int(mesh_ref.fixed_cull_ref.cell_index(inbox[:1], float(bound), cascade, H)[0][0])
        fields["one"] = fields["zero"].copy()
        fields["one"][c >> 3] = 1 << (c & 7)
    if kind == "identity":
        keep = Q.unpack(Q.points_cull(pts, w2o, box)[0], M)
        n_sp = min(M, 10)
        assert keep[M - n_sp:].tolist() == [True, True, True, False, False, False, False, False, False, False][:n_sp]    # faces in, an ulp past out, NaN / inf out
    for name, bits in fields.items():
        occ = None if bits is None else Occupancy(torch.from_numpy(bits).to(DEV), cascade, H, bound)
        mask, offsets, n_out = query.points_cull(x, 0, M, cw2o, cbox, occ)
        kw = {} if bits is None else dict(bitfield=bits, cascade=cascade, H=H)
        rmask, roffsets, rpos, rxn = Q.points_cull(pts, w2o, box, bound=float(bound), **kw)
        assert np.array_equal(mask.cpu().numpy().view(np.uint64), rmask), name
        assert np.array_equal(offsets.cpu().numpy().view(np.uint32), roffsets), name
        m_occ = int(n_out.item())
        assert m_occ == len(rpos) == int(roffsets[-1]), name
        assert name != "zero" or m_occ == 0
        assert name != "one" or m_occ >= 1
        assert not (name in ("none", "ones") and kind is None) or m_occ == M
        if m_occ:
            pos, xn = query.points_cull_emit(x, 0, M, mask, offsets, m_occ, bound, cw2o)
            assert _np_bits(pos, rpos) and _np_bits(xn, rxn), name
            only_xn = query.points_cull_emit(x, 0, M, mask, offsets, m_occ, bound, cw2o, want_pos=False)
            assert only_xn[0] is None and _same(only_xn[1], xn)


def test_points_cull_on_a_lattice_is_the_lattice_cull_and_slices_by_pointer():
    from focnerf_amd import mesh, query
    from focnerf_amd.fixedcull import Occupancy
    bound, res = 2, (5, 3, 67)
    axes = mesh.lattice_axes([-bound] * 3 + [bound] * 3, res, DEV)
    pts = mesh_ref.lattice_points(*(a.cpu().numpy() for a in axes))
    x = torch.from_numpy(pts).to(DEV)
    P = _placement("turned", bound)
    box = [-bound] * 3 + [bound] * 3
    occ = Occupancy(torch.from_numpy(np.random.default_rng(7).integers(0, 256, 2 * H ** 3 // 8, dtype=np.uint8)).to(DEV), 2, H, bound)
    for first, count in ((0, len(pts)), (100, 333)):
        for o in (None, occ):
            want = mesh.lattice_cull(axes, first, count, P, box, o)
            got = query.points_cull(x, first, count, _floats(P.world_to_object()), _floats(box), o)
            assert all(torch.equal(a, b) for a, b in zip(got, want))
            m_occ = int(want[2].item())
            if m_occ:
                pos = query.points_cull_emit(x, first, count, got[0], got[1], m_occ, bound, _floats(P.world_to_object()), want_xn=False)[0]
                assert _same(pos, mesh.lattice_cull_emit(axes, first, count, want[0], want[1], m_occ, P))


def test_a_nan_point_without_a_box_is_kept_as_it_is():
    from focnerf_amd import query
    pts = np.array([[np.nan, 0, 1], [0.5, np.inf, 0], [0.25, 0.5, -0.75]], np.float32)
    x = torch.from_numpy(pts).to(DEV)
    mask, offsets, n_out = query.points_cull(x, 0, 3)
    assert int(n_out.item()) == 3 and int(mask.item()) == 7 and offsets.tolist() == [0, 3]
    pos, xn = query.points_cull_emit(x, 0, 3, mask, offsets, 3, 1.0)
    assert _np_bits(pos, pts) and xn[2].tolist() == [0.625, 0.75, 0.125]


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("payload", [(True, True), (True, False), (False, True), (False, False)])
def test_scene_select_against_the_reference_over_three_calls(payload):
    from focnerf_amd import query
    n, keeps, sig, gains, rgbs, nrms, init = Q.select_case()
    bs, bi, br, bn = (torch.from_numpy(a.copy()).to(DEV) for a in init)
    br, bn = (br if payload[0] else None), (bn if payload[1] else None)
    for k in range(3):
        mask, offsets = Q.pack(keeps[k])
        m, o = torch.from_numpy(mask.view(np.int64)).to(DEV), torch.from_numpy(offsets.view(np.int32)).to(DEV)
        sc = torch.from_numpy(sig[k][keeps[k]]).to(DEV)
        rc = torch.from_numpy(rgbs[k]).to(DEV) if payload[0] else None
        nc = torch.from_numpy(nrms[k]).to(DEV) if payload[1] else None
        query.scene_select(sc, rc, nc, m, o, gains[k], k, bs, bi, br, bn, 0, n)
        want = Q.run_select(payload=payload, calls=k + 1)
        for got, ref in zip((bs, bi, br, bn), want):
            assert (got is None) == (ref is None)
            assert got is None or _np_bits(got, ref), f"call {k}"
    assert int(bi[0]) == 0 and int(bi[3]) == 1 and int(bi[4]) == 1 and int(bi[2]) == -1 and not torch.isnan(bs).any()


# ---------------------------------------------------------------- surface frame
def _frame_case(seed=4, m=301):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((m, 3)) * 10.0 ** rng.integers(-20, 20, (m, 1))).astype(np.float32)
    g[:8] = [[0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1, -np.inf, 2], [3, 0, 4], [0, 0, -1e-30], [1e38, 1e38, -1e38], [-0.0, 0.0, 0.0]]
    pos = (rng.standard_normal((m, 3))).astype(np.float32)
    eye = np.array([0.25, -1.5, 2.0], np.float32)
    pos[0] = eye                                                         # pos == eye
    pos[1] = [np.inf, 0, 0]
    pos[2] = [np.nan, 0, 0]
    pos[3] = eye + np.array([0, 0, 1e-3], np.float32)
    return g, pos, eye


@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("mode", ["normal", "eye"])
def test_surface_frame_inside_the_counted_bound(rotated, mode):
    from focnerf_amd import query, Placement
    g, pos, eye = _frame_case()
    R = Placement.rotated((1, 2, 0.5), 33).rotation.astype(np.float32) if rotated else None
    ref = Q.surface_frame(g, pos, R, eye if mode == "eye" else None)
    dirs, normal = query.surface_frame(torch.from_numpy(g).to(DEV), torch.from_numpy(pos).to(DEV), None if R is None else _floats(R),
                                       _floats(eye) if mode == "eye" else None)
    dirs, normal = dirs.cpu().numpy().astype(np.float64), normal.cpu().numpy().astype(np.float64)
    err_n, err_d = np.abs(normal - ref["normal"]), np.abs(dirs - ref["dirs"])
    print(f"surface_frame rotated={rotated} mode={mode}: max normal error / bound {np.max(err_n / np.maximum(ref['normal_bound'], 1e-300) * (err_n > 0)):.3f}, "
          f"dirs {np.max(err_d / np.maximum(ref['dirs_bound'], 1e-300) * (err_d > 0)):.3f}")
    assert np.isfinite(ref["normal_bound"]).all() and np.isfinite(ref["dirs_bound"]).all() and ref["normal_bound"].max() < 64 * 2.0 ** -24
    assert (err_n <= ref["normal_bound"]).all() and (err_d <= ref["dirs_bound"]).all()
    zero = [0, 1, 2, 3, 7]                                               # zero and non-finite gradients
    assert (normal[zero] == 0).all() and np.abs(np.linalg.norm(normal[8:], axis=-1) - 1).max() < 1e-6
    if mode == "normal":
        assert (dirs[zero] == [0, 0, -1]).all()
        if not rotated:
            assert np.array_equal(dirs[8:], -normal[8:])
    else:
        assert (dirs[[0, 1, 2]] == [0, 0, -1]).all() and np.allclose(dirs[3], [0, 0, 1], atol=1e-3)
    only_n = query.surface_frame(torch.from_numpy(g).to(DEV), None, None if R is None else _floats(R), None, want_dirs=False)
    assert only_n[0] is None and np.array_equal(only_n[1].cpu().numpy(), normal.astype(np.float32))
    if mode == "eye":                                                    # no gradient at all: the direction alone
        only_d = query.surface_frame(None, torch.from_numpy(pos).to(DEV), None, _floats(eye), want_normal=False)
        assert only_d[1] is None and np.array_equal(only_d[0].cpu().numpy(), dirs.astype(np.float32))


# ---------------------------------------------------------------- query_scene
@pytest.fixture(scope="module")
def model():
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(3)
    m = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


def _placements():
    from focnerf_amd import Placement
    return (Placement.rotated((0, 0, 1), 90, translation=(0.4, -0.2, 0.1), scale=0.5),
            Placement.rotated((1, 2, 0.5), 33, translation=(-0.5, 0.3, 0.0), scale=1.25))


def _scene_points(n=700, seed=5, half=1.5):
    return torch.from_numpy(((np.random.default_rng(seed).random((n, 3)) * 2 - 1) * half).astype(np.float32)).to(DEV)


def _occupancy(seed):
    from focnerf_amd.fixedcull import Occupancy
    return Occupancy(torch.from_numpy(np.random.default_rng(seed).integers(0, 256, H ** 3 // 8, dtype=np.uint8)).to(DEV), 1, H, 1)


def _sample_same(a, b):
    return all((u is None and v is None) or _same(u, v) for u, v in ((a.sigma, b.sigma), (a.object_id, b.object_id), (a.rgb, b.rgb), (a.normal, b.normal)))


def _by_hand(model, P, x, occ=None, eye=None, obj_feat=None):
    """One object's answer from the kernels query_scene sequences, called one at a time: -> (keep bool [n] on the device, sigma_c (not
    gained), rgb_c, normal_c, dirs_c)."""
    from focnerf_amd import query
    from focnerf_amd.field import field_infer
    from focnerf_amd.normals import _launch
    n = x.shape[0]
    w2o = _floats(P.world_to_object())
    mask, offsets, n_out = query.points_cull(x, 0, n, w2o, _floats(model.aabb_infer.cpu().numpy()), occ)
    m_occ = int(n_out.item())
    keep = torch.from_numpy(Q.unpack(mask.cpu().numpy(), n)).to(DEV)
    pos_c, xn_c = query.points_cull_emit(x, 0, n, mask, offsets, m_occ, float(model.bound), w2o)
    sigma_n, grad, _, _ = _launch(model, xn_c, None, want_sigma=True, want_grad=True)
    eye_obj = None if eye is None else query._eye_in_object(np.asarray(eye, np.float64), P)
    dirs_c, normal_c = query.surface_frame(grad, pos_c, _floats(P.rotation.astype(np.float32)), eye_obj)
    sigma_c, rgb_c = field_infer(model, xn_c, dirs_c, dir_div=1, obj_feat=obj_feat)
    assert _same(sigma_c, sigma_n)                                       # the header's contract: one sigma, whichever kernel
    return keep, sigma_c, rgb_c, normal_c, dirs_c


def test_query_one_object_identity_placement_has_the_field_kernels_bits(model):
    from focnerf_amd import query_scene, Placement, field_normals
    x = _scene_points(600, 6, 1.2)
    for view in ("normal", (0.3, -2.0, 1.7)):
        s = query_scene([model], [Placement()], x, view=view)
        keep, sigma_c, rgb_c, normal_c, _ = _by_hand(model, Placement(), x, eye=None if view == "normal" else view)
        assert 100 < int(keep.sum()) < 600
        assert _same(s.sigma[keep], sigma_c) and _same(s.rgb[keep], rgb_c) and _same(s.normal[keep], normal_c)
        assert (s.object_id[keep] == 0).all() and s.object_id.dtype == torch.int32
        out = ~keep
        assert (s.object_id[out] == -1).all() and not s.sigma[out].any() and not s.rgb[out].any() and not s.normal[out].any()
        assert _sample_same(s, query_scene([model], [None], x, view=view))                       # None: the object in its own frame
    xn = (x[keep] + 1.0) / 2.0
    _, nrgb = field_normals(model, xn)
    assert _same(0.5 * s.normal[keep] + 0.5, nrgb)                       # the normals kernel's own encoding of the same normal
    only = query_scene([model], [None], x, want=("normal",))
    assert only.rgb is None and _same(only.normal, s.normal) and _same(only.sigma, s.sigma)
    grid = query_scene([model], [None], x.view(20, 30, 3), want=())
    assert grid.sigma.shape == (20, 30) and grid.object_id.shape == (20, 30) and grid.rgb is None and grid.normal is None and _same(grid.sigma.view(-1), s.sigma)


@pytest.mark.parametrize("culled", [False, True], ids=["dense", "occupancy"])
def test_query_two_placed_objects_select_by_gained_sigma(model, culled):
    from focnerf_amd import query_scene
    P1, P2 = _placements()
    occs = [_occupancy(11), _occupancy(12)] if culled else [None, None]
    x = _scene_points(4000)
    s1, s2 = (query_scene([model], [P], x, occupancies=[o]) for P, o in zip((P1, P2), occs))
    both = query_scene([model, model], [P1, P2], x, occupancies=occs)
    for P, o, s in ((P1, occs[0], s1), (P2, occs[1], s2)):               # per object: the kernels' results, gained
        keep, sigma_c, rgb_c, normal_c, _ = _by_hand(model, P, x, o)
        assert _same(s.sigma[keep], sigma_c * float(P.sigma_gain)) and _same(s.rgb[keep], rgb_c) and _same(s.normal[keep], normal_c)
        assert (s.object_id[keep] == 0).all() and (s.object_id[~keep] == -1).all() and 20 < int(keep.sum()) < x.shape[0]
    second = s2.sigma > s1.sigma                                         # strict: a tie, and empty against empty, stays with the first
    assert second.any() and (~second & (s1.object_id == 0)).any() and ((s1.object_id == 0) & (s2.object_id == 0)).any()
    want_id = torch.where(second, torch.ones_like(s1.object_id), s1.object_id)
    assert torch.equal(both.object_id, want_id)
    assert _same(both.sigma, torch.where(second, s2.sigma, s1.sigma))
    assert _same(both.rgb, torch.where(second[:, None], s2.rgb, s1.rgb)) and _same(both.normal, torch.where(second[:, None], s2.normal, s1.normal))
    empty = both.object_id == -1
    assert empty.any() and not both.sigma[empty].any() and not both.rgb[empty].any() and not both.normal[empty].any()
    assert _sample_same(both, query_scene([model, model], [P1, P2], x, occupancies=occs))      # two runs: the same bits
    assert _sample_same(both, query_scene([model, model], [P1, P2], x, occupancies=occs, chunk=100))
    twice = query_scene([model, model], [P1, P1], x, occupancies=[occs[0], occs[0]])            # the same object twice: every tie stays with 0
    assert _sample_same(twice, s1)


def test_query_object_conditioned_network_takes_its_feature():
    from focnerf_amd import query_scene, Placement
    from focnerf_amd.field import field_plan
    from focnerf_amd.network_foc import NeRFNetwork
    torch.manual_seed(0)
    m = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    assert field_plan(m).uses_object_feature
    yolo = (None, None, torch.randn(144, generator=torch.Generator().manual_seed(100)).to(DEV))
    x = _scene_points(300, 8, 1.2)
    P = _placements()[1]
    s = query_scene([m], [P], x, yolo_details=[yolo])
    keep, sigma_c, rgb_c, normal_c, _ = _by_hand(m, P, x, obj_feat=m.encode_object_feature(yolo, torch.device(DEV)))
    assert int(keep.sum()) > 50 and _same(s.rgb[keep], rgb_c) and _same(s.sigma[keep], sigma_c * float(P.sigma_gain)) and _same(s.normal[keep], normal_c)
    other = (None, None, torch.randn(144, generator=torch.Generator().manual_seed(101)).to(DEV))
    assert not torch.equal(query_scene([m], [P], x, yolo_details=[other]).rgb, s.rgb)           # the feature reaches the colour network


def test_query_refuses_what_the_fused_kernels_do_not_serve(model, monkeypatch):
    from focnerf_amd import query_scene
    from focnerf_amd.network import NeRFNetwork
    x = _scene_points(65, 5, 0.9)                                        # every point inside the object's box
    base =query_scene([model], [None], x)
    monkeypatch.setenv("FOC_FUSED_INFER", "0")
    with pytest.raises(ValueError, match="infer"):
        query_scene([model], [None], x)
    assert query_scene([model], [None], x, want=("normal",)).rgb is None                        # normals do not need it
    monkeypatch.delenv("FOC_FUSED_INFER")
    monkeypatch.setenv("FOC_FUSED_NORMALS", "0")
    with pytest.raises(ValueError, match="normals"):
        query_scene([model], [None], x)
    with pytest.raises(ValueError, match="normals"):
        query_scene([model], [None], x, want=("normal",), view=(0, 0, 3))
    assert query_scene([model], [None], x, want=("rgb",), view=(0, 0, 3)).normal is None       # colours from an eye point do not need it
    alone = query_scene([model], [None], x, want=())                                           # the density alone: the inference kernel's sigma
    assert base.object_id.min() == 0 and _same(alone.sigma, base.sigma) and torch.equal(alone.object_id, base.object_id)
    monkeypatch.delenv("FOC_FUSED_NORMALS")
    torch.manual_seed(1)
    bg = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    bg.bg_radius = 2.0
    with pytest.raises(ValueError, match="bg_radius"):
        query_scene([model, bg], [None, None], x)
    with pytest.raises(ValueError):
        query_scene([model], [None], x, view="eye")
    with pytest.raises(ValueError):
        query_scene([model], [None], x.cpu())


# ---------------------------------------------------------------- meshes
R17 = 17


def test_extract_scene_mesh_is_the_scene_geometry_with_the_querys_attributes(model):
    from focnerf_amd import mesh, query_scene
    P1, P2 = _placements()
    vol = mesh.scene_volume([model, model], [P1, P2], R17, SCENE)
    thr = float(vol[vol > 0].median())
    m = mesh.extract_scene_mesh([model, model], [P1, P2], SCENE, R17, thr)
    v, f = mesh.extract_scene_geometry([model, model], [P1, P2], SCENE, R17, thr)
    assert len(f) > 0 and _same(m.vertices, v) and torch.equal(m.triangles, f)
    s = query_scene([model, model], [P1, P2], v)
    assert _same(m.normals, s.normal) and _same(m.colors, s.rgb) and torch.equal(m.object_id, s.object_id)
    assert (m.object_id == 0).any() and (m.object_id == 1).any() and m.object_id.min() >= -1
    assert 0 <= float(m.colors.min()) and float(m.colors.max()) <= 1


def test_extract_mesh_normals_colours_and_the_ply_round_trip(model, tmp_path):
    from focnerf_amd import mesh, density_gradient
    from scene_query_ref import CC, U
    thr = float(mesh.density_volume(model, R17).median())
    m = mesh.extract_mesh(model, R17, thr)
    v, f = mesh.extract_geometry(model, R17, thr)
    assert len(f) > 0 and _same(m.vertices, v) and torch.equal(m.triangles, f)
    inside = (m.object_id == 0).cpu().numpy()
    assert inside.mean() > 0.9 and ((m.object_id == 0) | (m.object_id == -1)).all()
    # the float64 unit normal of density_gradient's gradient: that gradient is the kernel's grad_raw times the slope and 1 / (2 bound), two
    # fp32 roundings per component, carried as C U 2 |g_d|
    _, grad = density_gradient(model, v)
    g = grad.cpu().numpy()
    ref = Q.surface_frame(g, grad_bound=CC * U * 2 * np.abs(g.astype(np.float64)))
    err = np.abs(m.normals.cpu().numpy().astype(np.float64) - ref["normal"])[inside]
    bound = ref["normal_bound"][inside]
    print(f"extract_mesh normals: max error {err.max():.3e}, max error / bound {np.max(err / bound):.3f}, bound max {bound.max():.3e}")
    assert np.isfinite(bound).all() and bound.max() < 64 * U and (err <= bound).all()
    # colours: the stated rounding, and the file
    c = m.colors.cpu().numpy()
    want_u8 = np.floor(np.clip(c, np.float32(0), np.float32(1)) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    assert m.colors_u8.dtype == torch.uint8 and np.array_equal(m.colors_u8.cpu().numpy(), want_u8) and len(np.unique(want_u8)) > 10
    path = str(tmp_path / "object.ply")
    assert mesh.save_mesh(model, path, R17, thr, colors=True) == (len(v), len(f))
    pv, pf, pn = mesh.read_ply(path)
    attrs = mesh.read_ply_attributes(path)
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy()) and np.array_equal(pn, m.normals.cpu().numpy())
    assert np.array_equal(attrs["colors"], want_u8) and np.array_equal(attrs["object_id"], m.object_id.cpu().numpy())
    eye = mesh.extract_mesh(model, R17, thr, view=(0.0, 0.0, 3.0))
    assert _same(eye.normals, m.normals) and not torch.equal(eye.colors, m.colors)
