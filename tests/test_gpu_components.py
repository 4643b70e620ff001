"""GPU: connected components on the device (csrc/components.hip, focnerf_amd/components.py, the keywords of mesh.py and
Occupancy.pruned) against the numpy definition of tests/components_ref.py. Every comparison is exact: integers, or the bits of floats."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_ref as cr                                              # noqa: E402
import mesh_ref                                                          # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VTOL = 2.0 ** -21                                                        # test_gpu_mesh.py: the vertex arithmetic's three roundings


def _dev(vol):
    return torch.from_numpy(np.array(vol, dtype=np.float32)).to(DEV)    # a copy: a shared reference volume is read-only


def _raw(vol, thr):
    """foc_cc_label itself: -> (labels uint32 [n], sizes uint32 [n], counts list of 4)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    v = _dev(vol)
    nx, ny, nz = v.shape
    nbytes = lib.foc_cc_workspace_bytes(nx, ny, nz)
    assert nbytes == 8 * v.numel()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    labels = torch.empty(v.numel(), dtype=torch.int32, device=DEV)
    sizes = torch.empty(v.numel(), dtype=torch.int32, device=DEV)
    counts = torch.full((4,), -1, dtype=torch.int32, device=DEV)
    check(lib.foc_cc_label(ptr(v), nx, ny, nz, float(thr), ptr(labels), ptr(sizes), ptr(ws), nbytes, ptr(counts), stream_of(v)), "cc_label")
    return labels.cpu().numpy().view(np.uint32), sizes.cpu().numpy().view(np.uint32), [int(c) & 0xFFFFFFFF for c in counts.tolist()]


def _check(vol, thr, ref=None):
    """The kernel's three outputs and `label_components` against the reference. -> the reference's (labels, sizes, first, roots)."""
    from focnerf_amd import label_components
    ref = cr.label(vol, thr) if ref is None else ref
    rlabels, rsizes, rfirst, rroots = ref
    labels, sizes, counts = _raw(vol, thr)
    want = np.where(rroots.reshape(-1) >= 0, rroots.reshape(-1), cr.NONE).astype(np.uint32)
    wsz = np.zeros(want.size, dtype=np.uint32)
    wsz[rfirst] = rsizes
    print("counts", counts, "reference", [len(rfirst), int(rsizes.sum()), int(rsizes.max()) if len(rsizes) else 0, 0])
    assert counts == [len(rfirst), int(rsizes.sum()), int(rsizes.max()) if len(rsizes) else 0, 0]
    assert np.array_equal(labels, want)
    assert np.array_equal(sizes, wsz)
    c = label_components(_dev(vol), thr)
    assert c.count == len(rfirst) and c.labels.dtype == torch.int32 and c.sizes.dtype == torch.int64 and c.first.dtype == torch.int64
    assert tuple(c.labels.shape) == tuple(np.shape(vol))
    assert np.array_equal(c.labels.cpu().numpy(), rlabels) and np.array_equal(c.sizes.cpu().numpy(), rsizes)
    assert np.array_equal(c.first.cpu().numpy(), rfirst)
    return ref


@functools.lru_cache(maxsize=None)
def _random_case(shape, fraction):
    vol = cr.random_volume(shape, fraction, seed=sum(shape))
    vol.setflags(write=False)
    return vol, cr.label(vol, 1.0 - fraction)


def test_all_256_corner_patterns():
    for case in range(256):
        _, sizes, first, _ = _check(cr.corner_pattern(case), 0.5)
        assert len(sizes) == (1 if case else 0)


@pytest.mark.parametrize("shape", [(3, 2, 5), (5, 7, 67), (65, 3, 2), (35, 19, 131)])
@pytest.mark.parametrize("fraction", [0.05, 0.12, 0.5])
def test_random_volumes(shape, fraction):
    vol, ref = _random_case(shape, fraction)
    _check(vol, 1.0 - fraction, ref)


@pytest.mark.parametrize("t", [4, 8, 16, 32, 64])
def test_diagonal_only_contacts_across_tile_edges(t):
    for d in cr.FORWARD_26:
        vol, p, q = cr.diagonal_pair((70, 70, 70), t, d)
        _, sizes, first, _ = _check(vol, 0.5)
        assert sizes.tolist() == [2] and first.tolist() == [min(p, q)], (t, d)


def test_serpentine_is_one_component():
    vol, length = cr.serpentine()
    labels, sizes, counts = _raw(vol, 0.5)
    first = int(np.flatnonzero(vol.reshape(-1))[0])
    assert counts == [1, length, length, 0]
    assert np.array_equal(labels, np.where(vol.reshape(-1) > 0, first, cr.NONE).astype(np.uint32))
    assert int(sizes[first]) == length and int(sizes.astype(np.int64).sum()) == length


def test_special_values_all_inside_and_all_outside():
    _, sizes, first, _ = _check(cr.special_volume(), 0.5)
    assert sizes.tolist() == [2, 1]
    n = 9 * 17 * 70
    _, sizes, first, _ = _check(np.ones((9, 17, 70), dtype=np.float32), 0.5)
    assert sizes.tolist() == [n] and first.tolist() == [0]
    _, sizes, _, _ = _check(np.zeros((9, 17, 70), dtype=np.float32), 0.5)
    assert len(sizes) == 0


def _filter(vol, thr, **kw):
    from focnerf_amd import filter_components
    return filter_components(_dev(vol), thr, **kw).cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def test_keep_order_and_both_rules():
    vol = np.zeros((2, 2, 70), dtype=np.float32)
    vol[1, 1, 40:42], vol[0, 0, 3:5], vol[0, 1, 69], vol[1, 0, 10:17] = 2.0, 1.0, 3.0, 0.75       # sizes 2 (first 3), 2, 1, 7
    two = vol.copy()
    two[1, 0, 10:17] = 0.0
    assert _same_bits(_filter(two, 0.5, keep_largest=1), cr.filter(two, 0.5, keep_largest=1))      # a tie: the earlier first point stays
    assert _filter(two, 0.5, keep_largest=1)[0, 0, 3] == 1 and _filter(two, 0.5, keep_largest=1)[1, 1, 40] == 0
    for kw in (dict(keep_largest=1), dict(keep_largest=2), dict(min_voxels=2), dict(keep_largest=3, min_voxels=3), dict(keep_largest=2, min_voxels=2, fill=-1.5),
               dict(min_voxels=8)):
        assert _same_bits(_filter(vol, 0.5, **kw), cr.filter(vol, 0.5, **kw)), kw
    v = _dev(vol)
    from focnerf_amd import filter_components
    assert filter_components(v, 0.5, keep_largest=4) is v and filter_components(v, 0.5, min_voxels=1) is v      # nothing removed: the input itself
    vol, ref = _random_case((35, 19, 131), 0.12)
    assert _same_bits(_filter(vol, 0.88, keep_largest=3, min_voxels=5), cr.filter(vol, 0.88, keep_largest=3, min_voxels=5))


def test_second_call_and_deterministic_mode_give_the_same_bits():
    import focnerf_amd
    vol, _ = _random_case((35, 19, 131), 0.12)
    a = _raw(vol, 0.88)
    b = _raw(vol, 0.88)
    with focnerf_amd.deterministic():
        c = _raw(vol, 0.88)
        f = _filter(vol, 0.88, keep_largest=2)
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(a[1], other[1]) and a[2] == other[2]
    assert _same_bits(f, _filter(vol, 0.88, keep_largest=2))


def test_filter_in_place():
    from focnerf_amd import filter_components
    vol, _ = _random_case((5, 7, 67), 0.12)
    v = _dev(vol)
    out = filter_components(v, 0.88, keep_largest=1, fill=-2.0, out=v)
    assert out is v
    want = cr.filter(vol, 0.88, keep_largest=1, fill=-2.0)
    assert not _same_bits(want, vol) and _same_bits(v.cpu().numpy(), want)


# ---------------------------------------------------------------- meshes
def _mc(vol_dev, thr, **kw):
    from focnerf_amd import mesh
    return tuple(o.cpu().numpy() for o in mesh.marching_cubes(vol_dev, thr, **kw))


def _triangle_set(v, f):
    return {tuple(v[t].reshape(-1).view(np.uint32).tolist()) for t in f}


def test_mesh_of_a_filtered_volume_equals_the_reference():
    from focnerf_amd import filter_components
    vol = mesh_ref.noise_volume(14, seed=3)
    thr = float(np.quantile(vol, 0.8))
    v, f = _mc(filter_components(_dev(vol), thr, min_voxels=4), thr)
    rv, rf = mesh_ref.marching_cubes(cr.filter(vol, thr, min_voxels=4), thr)
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(f, rf)
    assert (np.abs(v - rv) <= VTOL * np.maximum(1.0, np.abs(rv))).all()
    v0, f0 = _mc(_dev(vol), thr)
    assert (len(f0), len(f)) == (4196, 4172) and _triangle_set(v, f) <= _triangle_set(v0, f0)


def test_two_balls_keep_the_larger_one():
    from focnerf_amd import filter_components
    vol = cr.two_balls()
    assert len(cr.label(vol, 0.0)[1]) == 2
    v0, f0 = _mc(_dev(vol), 0.0)
    v, f = _mc(filter_components(_dev(vol), 0.0, keep_largest=1, fill=-1.0), 0.0)
    assert 0 < len(f) < len(f0)
    assert mesh_ref.is_closed(f) and mesh_ref.is_manifold(f) and mesh_ref.euler_characteristic(len(v), f) == 2
    assert mesh_ref.euler_characteristic(len(v0), f0) == 4
    assert _triangle_set(v, f) <= _triangle_set(v0, f0)
    assert np.abs(v - np.array([9.13, 9.21, 9.37])).max() < 7.0         # the larger ball stayed


@pytest.fixture(scope="module")
def model():
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(3)
    m = NeRFNetwork(bound=1, cuda_ray=False).to(DEV).eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


def test_extract_geometry_and_save_mesh_with_keep_largest(model, tmp_path):
    from focnerf_amd import mesh, filter_components, label_components
    R = 9
    vol = mesh.density_volume(model, R)
    counts = {q: label_components(vol, float(vol.quantile(q))).count for q in (0.5, 0.6, 0.7, 0.8, 0.9)}
    print("components per quantile", counts)
    q = next((q for q, k in counts.items() if k >= 2), 0.5)             # a threshold with something to remove, where the field has one
    thr = float(vol.quantile(q))
    origin, spacing = mesh.world_map(model.aabb_infer, R)
    v, f = mesh.extract_geometry(model, R, thr, keep_largest=1)
    w, g = mesh.marching_cubes(filter_components(vol.clone(), thr, keep_largest=1), thr, origin, spacing)
    assert len(f) > 0 and torch.equal(f, g) and torch.equal(v.view(torch.int32), w.view(torch.int32))
    path = str(tmp_path / "object.ply")
    assert mesh.save_mesh(model, path, R, thr, keep_largest=1) == (len(v), len(f))
    pv, pf, pn = mesh.read_ply(path)
    assert pn is None and np.array_equal(pv.view(np.uint32), v.cpu().numpy().view(np.uint32)) and np.array_equal(pf, f.cpu().numpy())
    # without the keywords: today's output
    v0, f0 = mesh.extract_geometry(model, R, thr)
    w0, g0 = mesh.marching_cubes(vol, thr, origin, spacing)
    assert torch.equal(f0, g0) and torch.equal(v0.view(torch.int32), w0.view(torch.int32))
    if counts[q] >= 2:
        assert len(f) < len(f0)
    m = mesh.extract_mesh(model, R, thr, keep_largest=1)
    assert torch.equal(m.triangles, f) and torch.equal(m.vertices.view(torch.int32), v.view(torch.int32))


# ---------------------------------------------------------------- occupancy
def test_pruned_occupancy_against_the_reference_and_its_cull_is_a_subset():
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.fixedcull import Occupancy, fixed_cull
    C, H, bound = 2, 16, 2
    grid = np.random.default_rng(9).random((C, H, H, H)) < 0.05
    grid[:, 5:9, 5:9, 5:9] = True                                        # a body among the specks
    bits = cr.pack_bitfield(grid)
    occ = Occupancy(torch.from_numpy(bits).to(DEV), C, H, bound)
    before = occ.bitfield.clone()
    for kw in (dict(), dict(keep_largest=2, min_cells=3), dict(keep_largest=None, min_cells=2)):
        got = occ.pruned(**kw)
        assert got is not occ and got.cascade == C and got.grid_size == H and got.bound == occ.bound
        want = cr.pruned(bits, C, H, **{"keep_largest": 1, **kw})
        assert np.array_equal(got.bitfield.cpu().numpy(), want), kw
        assert torch.equal(occ.bitfield, before)                         # self is not modified
    with pytest.raises(ValueError):
        occ.pruned(keep_largest=None)
    small = occ.pruned()
    assert 0 < int(small.bitfield.count_nonzero()) and not torch.equal(small.bitfield, occ.bitfield)
    o, d = synthetic.make_view_rays(16, 16, bound, 1, seed=0, device=DEV, radius=2.0 * bound)
    o, d = o[0].contiguous(), d[0].contiguous()
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32, device=DEV)
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, 0.2)
    m_all, _, n_all = fixed_cull(o, d, nears, fars, aabb, 33, occ)
    m_small, _, n_small = fixed_cull(o, d, nears, fars, aabb, 33, small)
    assert bool(((m_small & ~m_all) == 0).all()) and 0 < int(n_small) < int(n_all)
