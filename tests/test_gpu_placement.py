"""GPU: placed objects in the combined render (focnerf_amd/placement.py, csrc/fixedcull.hip foc_fixed_cull_placed /
foc_fixed_cull_emit_placed / foc_fixed_field_pack_culled_gain, `render_field4(..., occupancy=, placement=)`, combine.placed_field_fns).

1. cull and emit against tests/placement_ref.py, exactly;            2. the identity placement is the unplaced path, bit for bit;
3. the placed field against the masked dense field built from existing entry points;   4. a quarter turn is a turned camera;
5. doubling is exact;      6. through the combiner, with attribution;      7. one full-size chunk."""
import functools

import numpy as np
import pytest
import torch

import attribution_ref as aref
import fixed_cull_ref as ref
import placement_ref as pr

pytestmark = pytest.mark.gpu

H = 128


def _near_far(o, d, aabb, min_near=0.2):
    from focnerf_amd import raymarching
    return raymarching.near_far_from_aabb(o, d, aabb, min_near)


def _box(b):
    return torch.tensor([-float(b)] * 3 + [float(b)] * 3, dtype=torch.float32, device="cuda")


def _rays(N, SB, centre, seed=0):
    o, d = pr.rays(N, SB, centre, seed)
    return torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()


def _occ_bits(mask):
    """mask int64 [R] -> bool [R * 64]: the occupancy of every row of the block-interleaved per-sample arrays."""
    lanes = torch.arange(64, device=mask.device, dtype=torch.int64)
    return (((mask.unsqueeze(-1) >> lanes) & 1) != 0).reshape(-1)


@functools.lru_cache(maxsize=None)
def _random_bits(C, seed=7):
    return torch.randint(0, 256, (C * H ** 3 // 8,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).numpy()


# ---------------------------------------------------------------- 1. cull and emit against the reference
@pytest.mark.parametrize("SB,OB,C", pr.BOXES)
@pytest.mark.parametrize("T", pr.SHAPES_T)
@pytest.mark.parametrize("N", pr.SHAPES_N)
def test_placed_mask_offsets_and_compact_list_equal_the_reference(N, T, SB, OB, C):
    from focnerf_amd.fixedcull import Occupancy, fixed_cull, fixed_cull_emit
    from focnerf_amd.fixedstep import fixed_sample
    scene, obj_box = _box(SB), [-float(OB)] * 3 + [float(OB)] * 3
    nblk = -(-N // 64)
    own = (np.arange(nblk * 64) < N).reshape(nblk, 1, 64)
    n_bytes = C * H ** 3 // 8
    for name, P in pr.placements(SB).items():
        o, d = _rays(N, SB, P.translation)
        nears, fars = _near_far(o, d, scene)
        assert float(fars.max()) < 1e30                              # every ray crosses the scene's box
        _, xyz_blk = fixed_sample(o, d, nears, fars, scene, None, T, SB, want_xyzs=True, ray_block=64)
        xyz = xyz_blk.cpu().numpy().reshape(nblk, T, 64, 3)
        w2o = P.world_to_object()
        q = pr.to_object(w2o, xyz)
        ins = pr.inside(q, obj_box) & own                            # [nblk, T, 64]
        idx, _, _ = ref.cell_index(np.where(ins[..., None], q, np.float32(0)), OB, C, H)
        want_dirs = pr.to_object_dir(w2o, P.dir_scale, d.cpu().numpy())
        want_enc = torch.from_numpy(pr.norm(q, OB).reshape(-1, 3)).cuda()
        # "single": one cell an inside sample stands in; "random": 50 %, with that cell set and a second inside cell cleared where there
        # is one, so that neither "nothing" nor "everything" can come out of it
        cells = np.unique(idx[ins])
        single, rand = np.zeros(n_bytes, np.uint8), _random_bits(C).copy()
        if len(cells) >= 1:
            single[cells[0] >> 3] = 1 << (cells[0] & 7)
            rand[cells[0] >> 3] |= 1 << (cells[0] & 7)
        if len(cells) >= 2:
            rand[cells[1] >> 3] &= 255 ^ (1 << (cells[1] & 7))
        fields = {"zero": np.zeros(n_bytes, np.uint8), "one": np.full(n_bytes, 255, np.uint8), "random": rand, "single": single}
        for fname, bits in fields.items():
            tag = (name, fname)
            occ = Occupancy(torch.from_numpy(bits).cuda(), C, H, OB)
            want = ins & ref.occupied(idx, bits)
            w_mask, w_off, w_order = ref.cull(want.transpose(0, 2, 1).reshape(nblk * 64, T)[:N])
            runs = []
            for _ in range(2):
                mask, offsets, count = fixed_cull(o, d, nears, fars, scene, T, occ, placement=P, obj_aabb=obj_box)
                m_occ = int(count.item())
                enc_c, dirs_c = fixed_cull_emit(o, d, nears, fars, scene, T, OB, mask, offsets, m_occ, placement=P)
                runs.append((mask, offsets, count, enc_c, dirs_c))
            assert all(torch.equal(a, b) for a, b in zip(*runs)), tag               # the same list on every run
            assert np.array_equal(mask.cpu().numpy().view(np.uint64), w_mask), tag
            assert np.array_equal(offsets.cpu().numpy().view(np.uint32), w_off), tag
            assert m_occ == int(w_off[-1]) == int(want.sum()), tag
            pick = torch.from_numpy(want.reshape(-1)).cuda()
            assert torch.equal(pick, _occ_bits(mask)), tag
            assert torch.equal(enc_c, want_enc[pick]), tag
            assert torch.equal(dirs_c, torch.from_numpy(want_dirs[w_order[:, 0]]).cuda().reshape(-1, 3)), tag
            if fname == "zero":
                assert m_occ == 0, tag
            if fname == "one":
                assert m_occ == int(ins.sum()), tag
                if N >= 63 and T == 65:
                    assert 0 < m_occ < N * T, tag
            if fname == "random" and len(cells) >= 2:
                assert 0 < m_occ < int(ins.sum()), tag
            if fname == "single" and len(cells) >= 1:
                assert m_occ >= 1, tag


def test_placed_entry_points_refuse_and_handle_no_rays():
    import ctypes
    from focnerf_amd import Placement
    from focnerf_amd._lib import lib
    from focnerf_amd.fixedcull import Occupancy, fixed_cull, fixed_cull_emit
    occ = Occupancy(torch.full((H ** 3 // 8,), 255, dtype=torch.uint8, device="cuda"), 1, H, 1)
    e3 = torch.empty(0, 3, device="cuda")
    e1 = torch.empty(0, device="cuda")
    mask, offsets, count = fixed_cull(e3, e3, e1, e1, _box(2), 8, occ, placement=Placement(scale=0.5))
    assert mask.numel() == 0 and offsets.tolist() == [0] and count.tolist() == [0]
    enc_c, dirs_c = fixed_cull_emit(e3, e3, e1, e1, _box(2), 8, 1, mask, offsets, 0, placement=Placement())
    assert enc_c.shape == (0, 3) and dirs_c.shape == (0, 3)
    one = ctypes.c_void_p(offsets.data_ptr())
    bad = (ctypes.c_float * 12)(*([float("nan")] + [0.0] * 11))
    ok12, ok6 = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0), (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    assert lib.foc_fixed_cull_placed(one, one, one, one, one, 4, 8, None, ok6, 1.0, one, 1, H, one, one, one, one, 1 << 20, None) == 1
    assert b"null world_to_object" in lib.foc_last_error()
    assert lib.foc_fixed_cull_placed(one, one, one, one, one, 4, 8, bad, ok6, 1.0, one, 1, H, one, one, one, one, 1 << 20, None) == 1
    assert b"non-finite" in lib.foc_last_error()
    assert lib.foc_fixed_cull_placed(one, one, one, one, one, 4, 1, ok12, ok6, 1.0, one, 1, H, one, one, one, one, 1 << 20, None) == 1
    assert b"fixed_cull_placed: T must be >= 2" in lib.foc_last_error()
    assert lib.foc_fixed_cull_placed(one, one, one, one, one, 1 << 22, 512, ok12, ok6, 1.0, one, 1, H, one, one, one, one, 1 << 30, None) == 1
    assert b"2^31" in lib.foc_last_error()
    assert lib.foc_fixed_cull_emit_placed(one, one, one, one, one, 4, 8, bad, 1.0, 1.0, one, one, 1, one, one, None) == 1
    assert b"non-finite" in lib.foc_last_error()
    for gain in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.foc_fixed_field_pack_culled_gain(one, one, one, one, 1, one, one, 4, 8, 1.0, 1e-10, gain, one, None) == 1
        assert b"sigma_gain must be finite and > 0" in lib.foc_last_error()


# ---------------------------------------------------------------- models, grids, views
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
def _sphere(bound, radius_frac=0.35):
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.fixedcull import Occupancy
    grid = synthetic.analytic_density_grid(bound, radius_frac=radius_frac, device="cuda")
    return Occupancy(raymarching.packbits(grid, 25.0), grid.shape[0], H, bound)      # half of sigma0: the cells inside the ball


def _view(n, bound, seed, side=24):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(side, side, bound, 1, seed=seed, device="cuda", radius=2.0 * bound)
    pick = torch.linspace(0, side * side - 1, n).long().cuda()        # spread over the whole view
    return o[0, pick].contiguous(), d[0, pick].contiguous()


# ---------------------------------------------------------------- 2. the identity placement is the unplaced path
@pytest.mark.parametrize("kind", KINDS)
def test_identity_placement_equals_the_unplaced_culled_field(kind):
    from focnerf_amd import Placement
    from focnerf_amd.fixedstep import render_field4
    N, T = 130, 65
    m, yolo, occ = _model(kind, 1), _yolo(kind), _sphere(1)
    o, d = _view(N, 1, seed=5)
    want = render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=occ)
    assert (want[..., 0] > 0).any() and (want[..., 1:] != 0).any() and (want[..., 0] == 0).any()
    got = render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=occ, placement=Placement())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))                      # the bits
    buf = torch.full((N, T, 4), 7.0, device="cuda")
    got = render_field4(m, o, d, num_steps=T, yolo_details=yolo, out=buf, occupancy=occ, placement=Placement(), scene_aabb=m.aabb_infer.clone())
    assert got is buf and torch.equal(buf.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------- 3. placed field against the masked dense field
def _masked_dense_placed(model, o, d, T, occ, P, scene, yolo=None, thresh=1e-10):
    """(field4 [N,T,4], occupied count): the kernel's own mask / offsets / enc_in_c / dirs_c -> field_infer on the compact list -> sigma times
    the fp32 gain in torch -> scattered into dense block-interleaved arrays -> foc_fixed_field_pack(ray_block=64), an existing entry point."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from focnerf_amd.field import field_infer, field_plan
    from focnerf_amd.fixedcull import fixed_cull, fixed_cull_emit
    N = o.shape[0]
    nears, fars = _near_far(o, d, scene, model.min_near)
    mask, offsets, count = fixed_cull(o, d, nears, fars, scene, T, occ, placement=P, obj_aabb=model.aabb_infer)
    m_occ = int(count.item())
    enc_c, dirs_c = fixed_cull_emit(o, d, nears, fars, scene, T, model.bound, mask, offsets, m_occ, placement=P)
    with torch.no_grad():
        obj = model.encode_object_feature(yolo, o.device) if field_plan(model).uses_object_feature else None
        sigma_c, rgb_c = field_infer(model, enc_c, dirs_c, dir_div=1, dir_block=0, obj_feat=obj)
    sigma_c = sigma_c * torch.tensor(float(P.sigma_gain), dtype=torch.float32, device="cuda")
    bits = _occ_bits(mask)
    sigma = torch.zeros(bits.numel(), device="cuda")
    rgb = torch.zeros(bits.numel(), 3, device="cuda")
    sigma[bits] = sigma_c                                              # row order = the compact list's order
    rgb[bits] = rgb_c
    out = torch.empty(N, T, 4, device="cuda")
    check(lib.foc_fixed_field_pack(ptr(sigma), ptr(rgb), ptr(nears), ptr(fars), None, None, 1.0, N, T, float(model.density_scale), float(thresh),
                                   None, None, None, ptr(out), 64, stream_of(sigma)), "fixed_field_pack")
    return out, m_occ


@pytest.mark.parametrize("which", ["small", "large"])
@pytest.mark.parametrize("kind", KINDS)
def test_placed_field_equals_the_masked_dense_field(kind, which):
    from focnerf_amd.fixedstep import render_field4
    N, T, SB = 130, 65, 2
    P = pr.placements(SB)[which]
    m, yolo, occ, scene = _model(kind, 1), _yolo(kind), _sphere(1), _box(SB)
    o, d = _rays(N, SB, P.translation)
    want, m_occ = _masked_dense_placed(m, o, d, T, occ, P, scene, yolo)
    assert 0 < m_occ < N * T and (want[..., 0] > 0).any() and (want[..., 1:] != 0).any()
    got = render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=occ, placement=P, scene_aabb=scene)
    assert got.shape == (N, T, 4) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the gain is in the field: the same placement at scale 1 has other densities
    assert float(P.sigma_gain) != 1.0


# ---------------------------------------------------------------- 4. a quarter turn is a turned camera
@pytest.mark.parametrize("b,C", [(1, 1), (2, 2)])
@pytest.mark.parametrize("T", pr.SHAPES_T)
@pytest.mark.parametrize("N", pr.SHAPES_N)
def test_a_quarter_turn_is_a_turned_camera(N, T, b, C):
    """90 degrees about z on a box symmetric about the origin: A is a signed permutation, so A (o + d z) = (A o) + (A d) z product by
    product, the clamp commutes with it, and the placed cull on (o, d) is the unplaced cull on (R^T o, R^T d) along the same near / far."""
    from focnerf_amd import Placement
    from focnerf_amd.fixedcull import Occupancy, fixed_cull, fixed_cull_emit
    P = Placement.rotated((0, 0, 1), 90)
    w2o = P.world_to_object()
    box = _box(b)
    o, d = _rays(N, b, (0, 0, 0), seed=4)
    nears, fars = _near_far(o, d, box)
    o_t = torch.from_numpy(pr.to_object_dir(w2o, 1.0, o.cpu().numpy())).cuda()
    d_t = torch.from_numpy(pr.to_object_dir(w2o, 1.0, d.cpu().numpy())).cuda()
    assert torch.equal(o_t, torch.stack([o[:, 1], -o[:, 0], o[:, 2]], -1))
    for bits in (_random_bits(C), _sphere(b).bitfield.cpu().numpy()):
        occ = Occupancy(torch.from_numpy(bits).cuda(), C, H, b)
        mask, offsets, count = fixed_cull(o, d, nears, fars, box, T, occ, placement=P, obj_aabb=box)
        m_occ = int(count.item())
        enc_c, dirs_c = fixed_cull_emit(o, d, nears, fars, box, T, b, mask, offsets, m_occ, placement=P)
        mask_t, offsets_t, count_t = fixed_cull(o_t, d_t, nears, fars, box, T, occ)
        enc_t, dirs_t = fixed_cull_emit(o_t, d_t, nears, fars, box, T, b, mask_t, offsets_t, int(count_t.item()))
        assert torch.equal(mask, mask_t) and torch.equal(offsets, offsets_t) and torch.equal(count, count_t)
        assert torch.equal(enc_c, enc_t) and torch.equal(dirs_c, dirs_t)
        if N * T >= 63 * 65:
            assert 0 < m_occ < N * T


# ---------------------------------------------------------------- 5. doubling is exact
@pytest.mark.parametrize("kind", KINDS)
def test_doubling_is_exact(kind):
    """Scale 2 about the origin in the box +-2b against the unplaced object on (o / 2, d) with (near / 2, far / 2) in the box +-b: every
    position halves exactly, so the same samples are occupied with the same network inputs; sigma takes the exact factor 1/2 and the
    interval the exact factor 2, so alpha, the weights and the masked rgb are the same bits."""
    from focnerf_amd import Placement
    from focnerf_amd.field import field_plan
    from focnerf_amd.fixedcull import culled_field4
    from focnerf_amd.fixedstep import render_field4
    N, T, b = 130, 65, 1
    m, yolo, occ = _model(kind, b), _yolo(kind), _sphere(b)
    P, scene = Placement(scale=2), _box(2 * b)
    o, d = _rays(N, 2 * b, (0, 0, 0), seed=6)
    nears, fars = _near_far(o, d, scene, m.min_near)
    placed = render_field4(m, o, d, num_steps=T, yolo_details=yolo, occupancy=occ, placement=P, scene_aabb=scene)
    half = culled_field4(m, field_plan(m), (o * 0.5).contiguous(), d, nears * 0.5, fars * 0.5, m.aabb_infer, T, 1e-10, yolo,
                         torch.empty(N, T, 4, device="cuda"), occ)
    assert (half[..., 0] > 0).any() and (half[..., 1:] != 0).any() and (half[..., 0] == 0).any()
    assert torch.equal(placed[..., 1:], half[..., 1:])
    assert torch.equal(placed[..., 0], half[..., 0] * 0.5)
    # and along given near / far the placed sequence is render_field4's
    again = culled_field4(m, field_plan(m), o, d, nears, fars, scene, T, 1e-10, yolo, torch.empty(N, T, 4, device="cuda"), occ, P)
    assert torch.equal(again, placed)


# ---------------------------------------------------------------- 6. through the combiner
def _scene_of_three():
    """Model A twice (left, small and turned; right, as trained) and model B in the middle, in the box +-2. Rays come down the z axis in
    three bundles, each aimed at one object's centre and passing the other two at a distance: every object owns rays."""
    from focnerf_amd import Placement
    SB = 2
    placements = [Placement.rotated((1, 2, 3), 37, translation=(-1.2, 0.1, 0.0), scale=0.75), Placement(translation=(1.0, -0.1, 0.1)), Placement()]
    models = [_model("plain", 1, seed=20), _model("plain", 1, seed=20), _model("plain", 1, seed=21)]
    assert models[0] is models[1]
    return SB, models, [_sphere(1)] * 3, placements


def _bundle_rays(N, placements, seed=8):
    rng = np.random.default_rng(seed)
    target = np.stack([placements[k % 3].translation for k in range(N)])
    o = target + np.concatenate([rng.uniform(-0.3, 0.3, size=(N, 2)), np.full((N, 1), 3.0)], -1)
    d = target + rng.uniform(-0.1, 0.1, size=(N, 3)) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()


def test_placed_objects_through_the_combiner_with_attribution():
    from focnerf_amd.combine import ObjectCombiner, combine_packed, placed_field_fns
    from focnerf_amd.fixedstep import render_field4
    N, T = 130, 65
    SB, models, occs, placements = _scene_of_three()
    scene = _box(SB)
    o, d = _bundle_rays(N, placements)
    fns, nears, fars = placed_field_fns(models, occs, placements, o, d, T, scene)
    w_nears, w_fars = _near_far(o, d, scene, models[0].min_near)
    assert torch.equal(nears, w_nears) and torch.equal(fars, w_fars) and float(fars.max()) < 1e30
    img, dep = ObjectCombiner(rank=0, world_size=1).render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=64)
    fields = [render_field4(m, o, d, num_steps=T, occupancy=oc, placement=P, scene_aabb=scene) for m, oc, P in zip(models, occs, placements)]
    assert all((f[..., 0] > 0).any() for f in fields) and not torch.equal(fields[0], fields[1])
    want_img, want_dep, att = combine_packed(fields, nears, fars, (1.0, 0.0), attribution=True)
    assert img.shape == (2, N, 4) and torch.equal(img, want_img) and torch.equal(dep, want_dep)
    assert not torch.equal(img[0], img[1])                           # the two backgrounds
    img2, dep2 = combine_packed(fields, nears, fars, (1.0, 0.0))
    assert torch.equal(img2, want_img) and torch.equal(dep2, want_dep)
    # both copies of model A are seen: the float64 reference on the same fields says so, and the kernel's instance map agrees with it
    dens = np.stack([f[..., 0].cpu().numpy() for f in fields])
    r = aref.attribution(dens, nears.cpu().numpy(), fars.cpu().numpy(), 3)
    inst = att.instance.cpu().numpy()
    clear = aref.top_two_gap(r.obj_weights) > 1e-4
    for k in range(3):
        assert (r.instance[clear] == k).any(), k
        assert (inst[clear] == k).any(), k
    assert np.array_equal(inst[clear], r.instance[clear])
    # the attribution through render_view, cut in pieces of 64 rays
    img3, dep3, att3 = ObjectCombiner(rank=0, world_size=1).render_view(fns, N, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=64, attribution=(0, 3))
    assert torch.equal(img3, want_img) and torch.equal(dep3, want_dep) and torch.equal(att3.instance, att.instance)


# ---------------------------------------------------------------- 7. one full-size chunk
def _torch_placed_count(xyz, w2o, obj_box, occ):
    """The occupied count of block-interleaved world samples xyz [M,3] on the device: the contract's arithmetic in torch ops (eager: one
    rounding per op, nothing fused)."""
    w = [float(v) for v in w2o]
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    q = torch.stack([((w[3 * k] * x + w[3 * k + 1] * y) + w[3 * k + 2] * z) + w[9 + k] for k in range(3)], -1)
    lo, hi = obj_box[:3], obj_box[3:]
    ins = ((q >= lo) & (q <= hi)).all(-1)
    q = torch.where(ins[:, None], q, torch.zeros_like(q))
    level = torch.frexp(q.abs().max(-1).values)[1].clamp(0, occ.cascade - 1)
    pow2 = torch.tensor([float(2 ** c) for c in range(occ.cascade)], device=q.device)      # exact powers of two, by table
    mip = torch.minimum(pow2[level.long()], torch.tensor(float(occ.bound), device=q.device))
    t = q / mip[:, None] + 1.0
    n = (0.5 * t.double() * occ.grid_size).float().clamp(0, occ.grid_size - 1).long()

    def expand(v):
        v = (v * 0x00010001) & 0xFF0000FF
        v = (v * 0x00000101) & 0x0F00F00F
        v = (v * 0x00000011) & 0xC30C30C3
        v = (v * 0x00000005) & 0x49249249
        return v
    idx = level.long() * occ.grid_size ** 3 + (expand(n[:, 0]) | (expand(n[:, 1]) << 1) | (expand(n[:, 2]) << 2))
    bit = (occ.bitfield[idx >> 3].long() >> (idx & 7)) & 1
    return int((ins & (bit != 0)).sum())


def test_full_size_chunk_runs_and_counts_what_torch_counts():
    from focnerf_amd.fixedcull import fixed_cull
    from focnerf_amd.fixedstep import fixed_sample, render_field4
    N, T, SB = 16384, 512, 2
    P = pr.placements(SB)["large"]
    m, occ, scene = _model("plain", 1), _sphere(1), _box(SB)
    o, d = _view(N, SB, seed=2, side=128)
    nears, fars = _near_far(o, d, scene, m.min_near)
    mask, offsets, count = fixed_cull(o, d, nears, fars, scene, T, occ, placement=P, obj_aabb=m.aabb_infer)
    m_occ = int(count.item())
    _, xyz = fixed_sample(o, d, nears, fars, scene, None, T, SB, want_xyzs=True, ray_block=64)
    assert m_occ == _torch_placed_count(xyz, P.world_to_object(), m.aabb_infer, occ) == int(offsets[-1])
    assert 0 < m_occ < N * T // 2
    out = render_field4(m, o, d, num_steps=T, occupancy=occ, placement=P, scene_aabb=scene)
    assert int((out[..., 0] > 0).sum()) <= m_occ and (out[..., 0] > 0).any() and bool(torch.isfinite(out).all())
