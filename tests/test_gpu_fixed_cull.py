"""GPU: occupancy-culled fixed-step fields (csrc/fixedcull.hip, focnerf_amd/fixedcull.py, `render_field4(..., occupancy=)`).

1. the cull pass (mask, offsets, compact positions / directions) against tests/fixed_cull_ref.py, exactly;
2. the culled field against the MASKED DENSE field built from existing entry points only — fixed_sample(rb=64) -> field_infer(dir_block=64)
   -> sigma zeroed where the kernel's own mask is clear -> foc_fixed_field_pack(ray_block=64) — bit for bit;
3. the same through ObjectCombiner.render_view; 4. Occupancy.estimate; 5. one full-size chunk."""
import functools

import numpy as np
import pytest
import torch

import fixed_cull_ref as ref

pytestmark = pytest.mark.gpu

H = 128


def _near_far(o, d, aabb, min_near=0.2):
    from focnerf_amd import raymarching
    return raymarching.near_far_from_aabb(o, d, aabb, min_near)


def _occ_bits(mask):
    """mask int64 [R] -> bool [R * 64]: the occupancy of every row of the block-interleaved per-sample arrays."""
    lanes = torch.arange(64, device=mask.device, dtype=torch.int64)
    return (((mask.unsqueeze(-1) >> lanes) & 1) != 0).reshape(-1)


# ---------------------------------------------------------------- 1. mask and list against the reference
def _cull_rays(N, bound, seed=0):
    """The LAST N of: view rays, one ray that misses the box, one whose far end lies outside it (its last samples clip onto a face).
    -> o, d, nears, fars, aabb (the far of the clipping ray is pushed out by half a box after near_far_from_aabb)."""
    from focnerf_amd import synthetic
    vo, vd = synthetic.make_view_rays(16, 16, bound, 1, seed=seed, device="cuda", radius=2.0 * bound)
    o = torch.cat([vo[0], torch.tensor([[3.0 * bound] * 3, [0.1, -0.2, -2.0 * bound]], device="cuda")])
    d = torch.cat([vd[0], torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], device="cuda")])
    o, d = o[-N:].contiguous(), d[-N:].contiguous()
    aabb = torch.tensor([-bound] * 3 + [bound] * 3, dtype=torch.float32, device="cuda")
    nears, fars = _near_far(o, d, aabb)
    if N >= 2:
        assert float(nears[-2]) > 1e30                               # the miss
    fars[-1] += 0.5 * bound
    return o, d, nears, fars, aabb


@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("T", [2, 3, 65])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_mask_offsets_and_compact_list_equal_the_reference(N, T, bound):
    from focnerf_amd.fixedcull import Occupancy, fixed_cull, fixed_cull_emit
    from focnerf_amd.fixedstep import fixed_sample
    C = 1 if bound == 1 else 2
    o, d, nears, fars, aabb = _cull_rays(N, bound)
    enc_blk, xyz_blk = fixed_sample(o, d, nears, fars, aabb, None, T, bound, want_xyzs=True, ray_block=64)
    nblk = -(-N // 64)
    xyz = xyz_blk.cpu().numpy().reshape(nblk, T, 64, 3)
    assert np.abs(xyz).max() <= bound
    assert abs(xyz[(N - 1) // 64, -1, (N - 1) % 64, 2]) == bound     # the clipping ray's last sample lies on a face
    idx, _, _ = ref.cell_index(xyz, bound, C, H)                     # [nblk, T, 64]
    own = (np.arange(nblk * 64) < N).reshape(nblk, 1, 64)
    # two real samples in different cells (the clipping ray alone has them: its first sample on one face, its last on the opposite one)
    own_idx = idx.transpose(0, 2, 1).reshape(nblk * 64, T)[:N].reshape(-1)
    cell_a = int(own_idx[0])
    cell_b = int(own_idx[own_idx != cell_a][0])
    single = np.zeros(C * H ** 3 // 8, np.uint8)
    single[cell_a >> 3] = 1 << (cell_a & 7)
    # random 50 %, seeded — with cell_a set and cell_b cleared, so that neither "nothing" nor "everything" can come out of it at N * T = 2
    rand = torch.randint(0, 256, (C * H ** 3 // 8,), generator=torch.Generator().manual_seed(7), dtype=torch.uint8).numpy()
    rand[cell_a >> 3] |= 1 << (cell_a & 7)
    rand[cell_b >> 3] &= 255 ^ (1 << (cell_b & 7))
    fields = {"zero": np.zeros(C * H ** 3 // 8, np.uint8), "one": np.full(C * H ** 3 // 8, 255, np.uint8), "random": rand, "single": single}
    for name, bits in fields.items():
        occ = Occupancy(torch.from_numpy(bits).cuda(), C, H, bound)
        want = ref.occupied(idx, bits) & own                         # [nblk, T, 64]
        w_mask, w_off, w_order = ref.cull(want.transpose(0, 2, 1).reshape(nblk * 64, T)[:N])
        runs = []
        for _ in range(2):
            mask, offsets, count = fixed_cull(o, d, nears, fars, aabb, T, occ)
            m_occ = int(count.item())
            enc_c, dirs_c = fixed_cull_emit(o, d, nears, fars, aabb, T, bound, mask, offsets, m_occ)
            runs.append((mask, offsets, count, enc_c, dirs_c))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), name   # the same list on every run
        assert np.array_equal(mask.cpu().numpy().view(np.uint64), w_mask), name
        assert np.array_equal(offsets.cpu().numpy().view(np.uint32), w_off), name
        assert m_occ == int(w_off[-1]) == int(want.sum()), name
        pick = torch.from_numpy(want.reshape(-1)).cuda()
        assert torch.equal(enc_c, enc_blk[pick]), name               # rows of foc_fixed_sample(ray_block=64), in row order
        assert torch.equal(dirs_c, d[torch.from_numpy(w_order[:, 0]).cuda()]), name
        assert torch.equal(pick, _occ_bits(mask)), name
        if name == "zero":
            assert m_occ == 0
        if name == "one":
            assert m_occ == N * T
        if name == "random":
            assert 0 < m_occ < N * T
        if name == "single":
            assert m_occ >= 1


# ---------------------------------------------------------------- 2. culled field against the masked dense field
KINDS = ["plain", "foc", "tcnn"]


@functools.lru_cache(maxsize=None)
def _model(kind, bound, seed=0):
    from focnerf_amd import network, network_foc, network_tcnn
    cls = {"plain": network.NeRFNetwork, "foc": network_foc.NeRFNetwork, "tcnn": network_tcnn.NeRFNetwork}[kind]
    torch.manual_seed(seed)
    m = cls(bound=bound, cuda_ray=False).cuda().eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


def _yolo(kind, seed=0):
    if kind == "plain":
        return None
    return (None, None, torch.randn(144, generator=torch.Generator().manual_seed(100 + seed)).cuda())


@functools.lru_cache(maxsize=None)
def _sphere(bound, center=(0.0, 0.0, 0.0), radius_frac=0.35):
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.fixedcull import Occupancy
    grid = synthetic.analytic_density_grid(bound, center=center, radius_frac=radius_frac, device="cuda")
    return Occupancy(raymarching.packbits(grid, 25.0), grid.shape[0], H, bound)      # half of sigma0: the cells inside the ball


def _view(n, bound, seed, side=24):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(side, side, bound, 1, seed=seed, device="cuda", radius=2.0 * bound)
    pick = torch.linspace(0, side * side - 1, n).long().cuda()        # spread over the whole view: rays through the ball and rays past it
    return o[0, pick].contiguous(), d[0, pick].contiguous()


def _masked_dense(model, o, d, T, occ, yolo=None, thresh=1e-10):
    """(field4 [N,T,4], occupied count) from existing entry points: dense field in the 64-ray block order, sigma zeroed where the cull
    kernel's own mask is clear, foc_fixed_field_pack."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from focnerf_amd.field import field_infer, field_plan
    from focnerf_amd.fixedcull import fixed_cull
    from focnerf_amd.fixedstep import fixed_sample
    N = o.shape[0]
    aabb = model.aabb_infer
    nears, fars = _near_far(o, d, aabb, model.min_near)
    enc_in, _ = fixed_sample(o, d, nears, fars, aabb, None, T, model.bound, ray_block=64)
    with torch.no_grad():
        obj = model.encode_object_feature(yolo, o.device) if field_plan(model).uses_object_feature else None
        sigma, rgb = field_infer(model, enc_in, d, dir_div=T, dir_block=64, obj_feat=obj)
    mask, _, count = fixed_cull(o, d, nears, fars, aabb, T, occ)
    sigma = torch.where(_occ_bits(mask), sigma, torch.zeros_like(sigma))
    out = torch.empty(N, T, 4, device=o.device)
    check(lib.foc_fixed_field_pack(ptr(sigma), ptr(rgb), ptr(nears), ptr(fars), None, None, 1.0, N, T, float(model.density_scale), float(thresh),
                                   None, None, None, ptr(out), 64, stream_of(sigma)), "fixed_field_pack")
    return out, int(count.item())


@pytest.mark.parametrize("bound", [1, 1.5])
@pytest.mark.parametrize("N,T", [(300, 96), (130, 65)])
@pytest.mark.parametrize("kind", KINDS)
def test_culled_field_equals_the_masked_dense_field(kind, N, T, bound):
    from focnerf_amd.fixedcull import Occupancy
    from focnerf_amd.fixedstep import render_field4
    m, yolo, occ = _model(kind, bound), _yolo(kind), _sphere(bound)
    o, d = _view(N, bound, seed=5)
    want, m_occ = _masked_dense(m, o, d, T, occ, yolo)
    assert 0 < m_occ < N * T and (want[..., 0] > 0).any() and (want[..., 1:] != 0).any()
    assert int((want[..., 0] > 0).sum()) <= m_occ
    got = render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=occ)
    assert got.shape == (N, T, 4) and torch.equal(got, want)
    buf = torch.full((N, T, 4), 7.0, device="cuda")
    assert render_field4(m, o, d, num_steps=T, yolo_details=yolo, out=buf, occupancy=occ) is buf and torch.equal(buf, want)
    # nothing occupied: all zeros, no field launch; everything occupied: today's dense result
    cells = occ.cascade * H ** 3 // 8
    none = Occupancy(torch.zeros(cells, dtype=torch.uint8, device="cuda"), occ.cascade, H, bound)
    assert not render_field4(m, o, d, num_steps=T, yolo_details=yolo, out=buf, occupancy=none).any()
    full = Occupancy(torch.full((cells,), 255, dtype=torch.uint8, device="cuda"), occ.cascade, H, bound)
    dense = render_field4(m, o, d, num_steps=T, yolo_details=yolo)
    assert torch.equal(render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=full), dense)
    assert not torch.equal(dense, want)                               # the cull removed something the dense field has


# ---------------------------------------------------------------- 3. through the combiner
def test_culled_objects_through_the_combiner():
    from focnerf_amd.combine import ObjectCombiner, combine_packed
    from focnerf_amd.fixedstep import render_field4
    K, T, N = 3, 64, 400
    models = [_model("plain", 1, seed=20 + k) for k in range(K)]
    occs = [_sphere(1, center=c, radius_frac=0.3) for c in ((0.0, 0.0, 0.0), (0.35, 0.1, -0.2), (-0.3, -0.25, 0.3))]
    o, d = _view(N, 1, seed=9)
    nears, fars = _near_far(o, d, models[0].aabb_infer, models[0].min_near)
    fns = [(lambda lo, hi, out, m=m, oc=oc: render_field4(m, o[lo:hi], d[lo:hi], num_steps=T, out=out, occupancy=oc)) for m, oc in zip(models, occs)]
    img, dep = ObjectCombiner(rank=0, world_size=1).render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=128)
    fields = [_masked_dense(m, o, d, T, oc)[0] for m, oc in zip(models, occs)]
    want_img, want_dep = combine_packed(fields, nears, fars, (1.0, 0.0))
    assert img.shape == (2, N, 4) and torch.equal(img, want_img) and torch.equal(dep, want_dep)
    assert not torch.equal(img[0], img[1])                           # the two backgrounds
    assert all((f[..., 0] > 0).any() for f in fields)


# ---------------------------------------------------------------- 4. Occupancy.estimate
def test_estimate_equals_the_three_ops_by_hand_and_repeats_with_a_seed():
    from focnerf_amd import densitygrid, raymarching
    from focnerf_amd.fixedcull import Occupancy
    m = _model("plain", 1)
    passes, decay, thresh = 2, 0.95, 1e9      # the threshold is then the grid's mean: some cells above it, some below
    occ = Occupancy.estimate(m, passes=passes, decay=decay, density_thresh=thresh, jitter=False)
    assert (occ.cascade, occ.grid_size, occ.bound) == (m.cascade, m.grid_size, float(m.bound)) and not hasattr(m, "density_bitfield")
    grid = torch.zeros(m.cascade, H ** 3, device="cuda")
    bits = torch.zeros(m.cascade * H ** 3 // 8, dtype=torch.uint8, device="cuda")
    mean = torch.zeros(1, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for _ in range(passes):
            at = densitygrid.grid_cells_xyz(m.cascade, H, m.bound, None, torch.device("cuda"))
            sig = m.density(at)['sigma'].reshape(-1)
            densitygrid.grid_update_apply(grid, m.cascade, H, sig, None, m.density_scale, decay, thresh, bits, mean)
    level = min(float(mean.item()), thresh)
    assert torch.equal(occ.bitfield, raymarching.packbits(grid, level))
    set_bits = int(np.unpackbits(occ.bitfield.cpu().numpy()).sum())
    assert 0 < set_bits < m.cascade * H ** 3                         # a threshold inside the field's range: the comparison is not vacuous
    a, b = (Occupancy.estimate(m, passes=2, density_thresh=thresh, generator=torch.Generator(device="cuda").manual_seed(3)).bitfield for _ in range(2))
    assert torch.equal(a, b) and bool(a.any())


# ---------------------------------------------------------------- 5. one full-size chunk
def test_full_size_chunk_equals_the_masked_dense_field():
    from focnerf_amd.fixedstep import render_field4
    N, T = 16384, 512
    m, occ = _model("plain", 1), _sphere(1)
    o, d = _view(N, 1, seed=2, side=128)
    want, m_occ = _masked_dense(m, o, d, T, occ)
    assert 0 < m_occ < N * T // 2
    assert torch.equal(render_field4(m, o, d, num_steps=T, occupancy=occ), want)
