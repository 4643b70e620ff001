"""GPU: the mesh extraction (csrc/mesh.hip, focnerf_amd/mesh.py) against the float64 reference of tests/mesh_ref.py — marching cubes,
normals, the lattice cull, the density volumes of an object and of a placed scene, and extract_geometry / save_mesh end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref                                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VTOL = 2.0 ** -21                                                        # thr - u[p], u[q] - u[p] and the division are correctly rounded, one more rounding in the add onto the index


def _mc(vol, thr, **kw):
    from focnerf_amd import mesh
    out = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV), thr, **kw)
    return tuple(o.cpu().numpy() for o in out)


def _check_against_ref(vol, thr):
    v, f = _mc(vol, thr)
    rv, rf = mesh_ref.marching_cubes(vol, thr)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(f, rf)
    assert (np.abs(v - rv) <= VTOL * np.maximum(1.0, np.abs(rv))).all()
    return v, f


def test_all_256_single_cube_cases():
    for case in range(256):
        vol = np.array([(case >> c) & 1 for c in range(8)], dtype=np.float32).reshape(2, 2, 2).transpose(2, 1, 0)    # corner c at (c&1, c>>1&1, c>>2&1)
        v, f = _check_against_ref(vol, 0.5)
        assert len(f) == mesh_ref.NTRI[case]


@pytest.mark.parametrize("shape", [(3, 2, 5), (5, 7, 67), (65, 3, 2)])
def test_odd_shapes(shape):
    vol = np.random.default_rng(sum(shape)).random(shape).astype(np.float32)
    v, f = _check_against_ref(vol, 0.5)
    assert len(f) > 0


def test_noise_volume_closes_on_the_device():
    v, f = _check_against_ref(mesh_ref.noise_volume(24), 0.5)
    assert mesh_ref.is_closed(f)


def test_sphere_and_second_call_and_deterministic_mode():
    import focnerf_amd
    vol = mesh_ref.sphere_volume()
    v, f = _check_against_ref(vol, 0.0)
    assert mesh_ref.is_manifold(f) and mesh_ref.euler_characteristic(len(v), f) == 2
    v2, f2 = _mc(vol, 0.0)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(f, f2)
    with focnerf_amd.deterministic():
        v3, f3 = _mc(vol, 0.0)
    assert np.array_equal(v.view(np.uint32), v3.view(np.uint32)) and np.array_equal(f, f3)


def test_empty_surfaces():
    for fill in (0.0, 1.0):
        v, f = _mc(np.full((5, 4, 70), fill, dtype=np.float32), 0.5)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f, n = _mc(np.zeros((2, 2, 2), dtype=np.float32), 0.5, normals=True)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


def test_values_equal_to_the_threshold_still_close():
    vol = np.round(mesh_ref.sphere_volume(n=14, r=4.0, offset=(0, 0, 0)) * 2) / 2        # multiples of 1/2: many values are exactly 0
    assert (vol == 0).sum() > 8
    v, f = _check_against_ref(vol, 0.0)
    assert mesh_ref.is_closed(f)


def test_non_finite_values():
    vol = mesh_ref.sphere_volume()
    i = tuple(np.argwhere((vol[:-1] >= 0) != (vol[1:] >= 0))[0])
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = vol.copy()
        bad[i] = bad_value
        with pytest.raises(ValueError):
            _mc(bad, 0.0)
    far = vol.copy()
    far[0, 0, 0] = np.nan                                                # outside, among outside values: no edge there is crossed
    v, f = _mc(far, 0.0)
    rv, rf = mesh_ref.marching_cubes(vol, 0.0)
    assert np.array_equal(f, rf)


def test_origin_and_spacing():
    vol = mesh_ref.noise_volume(16)
    origin, spacing = np.array([-1.5, 0.25, 3.0], dtype=np.float32), np.array([0.125, 0.3, 0.01], dtype=np.float32)
    v, f = _mc(vol, 0.5)
    w, g = _mc(vol, 0.5, origin=origin, spacing=spacing)
    assert np.array_equal(f, g)
    want = origin.astype(np.float64) + v.astype(np.float64) * spacing.astype(np.float64)       # one fmaf: a single rounding of this
    assert (np.abs(w - want) <= np.spacing(np.abs(w))).all()
    u, _ = _mc(vol, 0.5, origin=(0, 0, 0), spacing=(1, 1, 1))
    assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_normals_on_the_sphere():
    vol = mesh_ref.sphere_volume()
    v, f, n = _mc(vol, 0.0, normals=True)
    rv, rf, rn = mesh_ref.marching_cubes(vol, 0.0, normals=True)
    assert np.array_equal(f, rf) and n.shape == rn.shape
    assert np.abs(n - rn).max() < 1e-5
    _, _, ns = _mc(vol, 0.0, normals=True, origin=(0, 0, 0), spacing=(1, 2, 4))
    _, _, rs = mesh_ref.marching_cubes(vol, 0.0, normals=True, spacing=(1, 2, 4))
    assert np.abs(ns - rs).max() < 1e-5


def test_mcubes_dropin_on_the_device():
    dropin = os.path.join(mesh_ref.REPO, "focnerf_amd", "dropin")
    sys.path.insert(0, dropin)
    try:
        sys.modules.pop("mcubes", None)
        import mcubes
        vol = mesh_ref.sphere_volume()
        v, f = mcubes.marching_cubes(vol, 0.0)
        rv, rf = mesh_ref.marching_cubes(vol, 0.0)
        assert v.dtype == np.float64 and f.dtype == np.int64 and np.array_equal(f, rf) and np.abs(v - rv).max() <= VTOL * 19
    finally:
        sys.path.remove(dropin)
        sys.modules.pop("mcubes", None)


# ---------------------------------------------------------------- lattice cull
H = 128


def _placement(bound):
    from focnerf_amd import Placement
    return Placement.rotated((0, 0, 1), 90, translation=(0.8 * bound, 0.7 * bound, 0.9 * bound), scale=0.5)     # the lattice's corner (b, b, b) lands inside


def _bitfields(points, bound, cascade):
    """name -> uint8 bitfield; `points` fp32 [n,3]: positions (in the frame the cell test sees) of lattice points inside the box."""
    cells = cascade * H ** 3
    index, _, _ = mesh_ref.fixed_cull_ref.cell_index(points, float(bound), cascade, H)
    a, others = int(index[0]), index[index != index[0]]
    b = int(others[0]) if len(others) else None                         # a second cell some lattice point lies in (forced clear), if there is one

    def with_bits(bits, set_cells, clear_cells=()):
        bits = bits.copy()
        for c in set_cells:
            bits[c >> 3] |= np.uint8(1 << (c & 7))
        for c in clear_cells:
            bits[c >> 3] &= np.uint8(~(1 << (c & 7)) & 0xFF)
        return bits
    zero = np.zeros(cells // 8, dtype=np.uint8)
    rand = np.random.default_rng(7).integers(0, 256, cells // 8, dtype=np.uint8)
    return {"one": with_bits(zero, [a]), "random": with_bits(rand, [a], [] if b is None else [b]), "ones": np.full(cells // 8, 255, dtype=np.uint8), "zero": zero}, a, b


@pytest.mark.parametrize("res", [(2, 2, 2), (5, 3, 67)])
@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("placed", [False, True])
def test_lattice_cull_against_the_reference(res, bound, placed):
    from focnerf_amd import mesh
    from focnerf_amd.fixedcull import Occupancy
    cascade = bound                                                      # bound 1: one cascade; bound 2: two
    axes = mesh.lattice_axes([-bound] * 3 + [bound] * 3, res, DEV)
    xs, ys, zs = (a.cpu().numpy() for a in axes)
    n = res[0] * res[1] * res[2]
    P = _placement(bound) if placed else None
    w2o = P.world_to_object() if placed else None
    box = [-bound] * 3 + [bound] * 3 if placed else None
    pts = mesh_ref.lattice_points(xs, ys, zs)
    if placed:
        q = mesh_ref.to_object(w2o, pts)
        inside = ((q >= -bound) & (q <= bound)).all(-1)
        assert inside.any() and not inside.all()                         # some lattice points fall outside the object's box
        pts = q[inside]
    fields, a, b = _bitfields(pts, bound, cascade)
    slabs = [(0, n)] if n < 100 else [(0, n), (100, 333)]
    for name, bits in fields.items():
        occ = Occupancy(torch.from_numpy(bits).to(DEV), cascade, H, bound)
        for first, count in slabs:
            mask, offsets, n_out = mesh.lattice_cull(axes, first, count, P, box, occ)
            rmask, roffsets, rpts = mesh_ref.lattice_cull(xs, ys, zs, first, count, w2o, box, float(bound), bits, cascade, H)
            assert np.array_equal(mask.cpu().numpy().view(np.uint64), rmask), name
            assert np.array_equal(offsets.cpu().numpy().view(np.uint32), roffsets), name
            m_occ = int(n_out.item())
            assert m_occ == len(rpts) == int(roffsets[-1])
            if name == "one" and first == 0:
                assert m_occ >= 1
            if name == "zero":
                assert m_occ == 0
            if name == "ones" and not placed:
                assert m_occ == count
            if m_occ:
                pos = mesh.lattice_cull_emit(axes, first, count, mask, offsets, m_occ, P)
                assert np.array_equal(pos.cpu().numpy().view(np.uint32), rpts.view(np.uint32)), name
    # without a bitfield: the box test alone (every point, unplaced)
    mask, offsets, n_out = mesh.lattice_cull(axes, 0, n, P, box, None)
    rmask, roffsets, rpts = mesh_ref.lattice_cull(xs, ys, zs, 0, n, w2o, box)
    assert np.array_equal(mask.cpu().numpy().view(np.uint64), rmask) and np.array_equal(offsets.cpu().numpy().view(np.uint32), roffsets)
    assert int(n_out.item()) == len(rpts)


# ---------------------------------------------------------------- volumes
@pytest.fixture(scope="module")
def model():
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(3)
    m = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


def _torch_lattice_sigma(model, res):
    """model.density on the torch-built lattice: the reference's extract_fields in one piece."""
    from focnerf_amd import mesh
    xs, ys, zs = mesh.lattice_axes(model.aabb_infer, res, DEV)
    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        return model.density(pts)['sigma'].reshape(xs.numel(), ys.numel(), zs.numel()).float()


def _bits_of(mask, n):
    m = mask.cpu().numpy().view(np.uint64)
    return ((m[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:n]


@pytest.fixture(scope="module", params=[9, (5, 3, 67)], ids=["R9", "R5x3x67"])
def dense(request, model):
    res = (request.param,) * 3 if isinstance(request.param, int) else request.param
    return res, _torch_lattice_sigma(model, res)


def test_dense_volume_is_the_models_density_on_the_lattice(model, dense):
    from focnerf_amd import mesh
    res, want = dense
    assert want.min() >= 0 and want.max() > want.min()
    for chunk in (1 << 22, 100):
        got = mesh.density_volume(model, res, chunk=chunk)
        assert got.dtype == torch.float32 and tuple(got.shape) == res
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"chunk {chunk}"


def test_culled_volume_is_the_dense_one_under_the_kernels_mask(model, dense):
    from focnerf_amd import mesh
    from focnerf_amd.fixedcull import Occupancy
    res, want = dense
    n = res[0] * res[1] * res[2]
    bits = torch.from_numpy(np.random.default_rng(11).integers(0, 256, H ** 3 // 8, dtype=np.uint8)).to(DEV)
    occ = Occupancy(bits, 1, H, 1)
    axes = mesh.lattice_axes(model.aabb_infer, res, DEV)
    mask, _, n_out = mesh.lattice_cull(axes, 0, n, occupancy=occ)
    keep = torch.from_numpy(_bits_of(mask, n)).to(DEV).reshape(res)
    assert 0 < int(n_out.item()) < n
    expect = torch.where(keep, want, torch.zeros_like(want))
    for chunk in (1 << 22, 100):
        got = mesh.density_volume(model, res, chunk=chunk, occupancy=occ)
        assert torch.equal(got.view(torch.int32), expect.view(torch.int32)), f"chunk {chunk}"


def test_scene_volume(model, dense):
    from focnerf_amd import mesh, Placement
    res, want = dense
    same = mesh.scene_volume([model], [Placement()], res, model.aabb_infer)
    assert torch.equal(same.view(torch.int32), want.view(torch.int32))  # the identity placement in the object's own box
    box = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]
    P1 = Placement.rotated((0, 0, 1), 90, translation=(0.4, -0.2, 0.1), scale=0.5)
    P2 = Placement.rotated((1, 2, 0.5), 33, translation=(-0.5, 0.3, 0.0), scale=1.25)
    v1, v2 = (mesh.scene_volume([model], [P], res, box) for P in (P1, P2))
    both = mesh.scene_volume([model, model], [P1, P2], res, box, chunk=100)
    assert (v1 > 0).any() and (v1 == 0).any() and (v2 > 0).any()
    assert torch.equal(both, torch.maximum(v1, v2))
    # the placed value: sigma at q = A x + b times the placement's gain
    axes = mesh.lattice_axes(box, res, DEV)
    pts = mesh_ref.lattice_points(*(a.cpu().numpy() for a in axes))
    q = mesh_ref.to_object(P1.world_to_object(), pts)
    inside = ((q >= -1) & (q <= 1)).all(-1)
    assert np.array_equal((v1.reshape(-1) > 0).cpu().numpy(), inside)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        sig = model.density(torch.from_numpy(q[inside]).to(DEV))['sigma'].float()
    assert torch.equal(v1.reshape(-1)[torch.from_numpy(inside).to(DEV)], sig * float(P1.sigma_gain))


def test_extract_geometry_and_save_mesh(model, tmp_path):
    from focnerf_amd import mesh
    R = 17
    vol = mesh.density_volume(model, R)
    thr = float(vol.median())
    v, f = mesh.extract_geometry(model, R, thr)
    v0, f0 = mesh.marching_cubes(vol, thr)
    assert len(f) > 0 and torch.equal(f, f0)
    origin, spacing = mesh.world_map(model.aabb_infer, R)
    want = origin.astype(np.float64) + v0.cpu().numpy().astype(np.float64) * spacing.astype(np.float64)
    assert (np.abs(v.cpu().numpy() - want) <= np.spacing(np.abs(v.cpu().numpy()))).all()
    box = model.aabb_infer.cpu().numpy().astype(np.float64)
    ref = v0.cpu().numpy().astype(np.float64) / (R - 1.0) * (box[3:] - box[:3]) + box[:3]     # the reference's line
    assert np.abs(v.cpu().numpy() - ref).max() < 1e-6
    path = str(tmp_path / "object.ply")
    nv, nf = mesh.save_mesh(model, path, R, thr, normals=True)
    pv, pf, pn = mesh.read_ply(path)
    assert (nv, nf) == (len(v), len(f)) and pv.shape == (nv, 3) and pf.shape == (nf, 3) and pn.shape == (nv, 3)
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy())
    length = np.linalg.norm(pn, axis=-1)
    assert ((np.abs(length - 1) < 1e-5) | (length == 0)).all() and (length > 0).any()
