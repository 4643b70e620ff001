"""GPU: the fused select + composite (+ attribution) fed from the compact culled lists (csrc/combine.hip k_combine_culled,
foc_combine_select_composite_culled; combine.culled_field_fns / combine_culled / render_scene_culled).

The yardstick is the two-step path — foc_fixed_field_pack_culled_gain per object, then foc_combine_select_composite{,_attr} — which
tests/test_gpu_fixed_cull.py, test_gpu_placement.py and test_gpu_attribution.py pin to float64 references. Every output is compared
bit for bit (torch.equal on the int32 view of the floats, so that a NaN equals itself), every ray, no tolerance.

1. synthetic lists over every shape;   2. the named cases, each asserted on the inputs;   3. refusals and N = 0;
4. three placed networks through render_scene_culled;   5. culled_field4 = culled_lists + pack, launch for launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
GAINS, SCALES, THRESH = (1.0, 2.0, 0.5), (1.0, 0.5), (1e-10, 1e-4, 1e-2)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    assert torch.equal(_bits(got), _bits(want)), tag


# ---------------------------------------------------------------- synthetic culled lists
class Obj:
    """One object's lists on the host (numpy), uploaded by `dev()`."""

    def __init__(self, N, occ, sigma_c, rgb_c, density_scale, thresh, gain):
        self.N, self.occ = N, occ                                               # bool [nblk, T, 64]: row (blk, i), lane n % 64
        self.sigma_c, self.rgb_c = sigma_c.astype(np.float32), rgb_c.astype(np.float32)
        self.density_scale, self.thresh, self.gain = density_scale, thresh, gain

    def slot(self, n, i):
        """index of sample (n, i) in the compact arrays (it must be occupied)"""
        assert self.occ[n // 64, i, n % 64]
        flat = self.occ.reshape(-1)
        return int(flat[: (n // 64 * self.occ.shape[1] + i) * 64 + n % 64].sum())

    def dev(self):
        from focnerf_amd.fixedcull import CulledField
        nblk, T, _ = self.occ.shape
        words = (self.occ.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).reshape(-1)
        counts = self.occ.sum(-1).reshape(-1)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        m_occ = int(offsets[-1])
        assert m_occ == len(self.sigma_c) == len(self.rgb_c)
        up = lambda a: torch.from_numpy(a).cuda()
        return CulledField(up(words.view(np.int64)), up(offsets.view(np.int32)), m_occ, up(self.sigma_c) if m_occ else None,
                           up(self.rgb_c.reshape(-1, 3)) if m_occ else None, self.density_scale, self.thresh, self.gain, self.N, T)


def _objects(N, T, K, density, seed):
    """K random objects: masks of the given density with the padding lanes cleared, offsets their exclusive popcount prefix sum, random
    sigma_c / rgb_c; gain, density_scale and thresh differ per object."""
    rng = np.random.default_rng(seed)
    nblk = -(-N // 64)
    own = (np.arange(nblk * 64) < N).reshape(nblk, 1, 64)
    objs = []
    for k in range(K):
        occ = (rng.random((nblk, T, 64)) < density) & own
        m = int(occ.sum())
        objs.append(Obj(N, occ, rng.gamma(0.7, 20.0, m), rng.random((m, 3)), SCALES[k % 2], THRESH[k % 3], GAINS[k % 3]))
    return objs


def _near_far(N, seed):
    rng = np.random.default_rng(seed + 1000)
    near = rng.uniform(0.2, 1.0, N).astype(np.float32)
    return near, (near + rng.uniform(1.0, 3.0, N)).astype(np.float32)


def _want(culled, nears, fars, ids, n_obj, bgs=(1.0, 0.0)):
    """The two-step path: the culled pack (with gain) per object into a dense field4, then the dense fused select + composite."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from focnerf_amd.combine import HipCombineOps
    N, T = culled[0].N, culled[0].T
    fields = []
    for c in culled:
        f = torch.full((N, T, 4), 7.0, device="cuda")
        check(lib.foc_fixed_field_pack_culled_gain(ptr(c.sigma_c), ptr(c.rgb_c), ptr(c.mask), ptr(c.offsets), c.m_occ, ptr(nears), ptr(fars), N, T,
                                                   c.density_scale, c.thresh, c.sigma_gain, ptr(f), stream_of(f)), "pack")
        fields.append(f)
    if n_obj:
        image4, depth, att, merged, winner = HipCombineOps.select_composite_attr(fields, nears, fars, bgs, n_obj, ids=ids, want_merged=True, want_winner=True)
        return dict(image4=image4, depth=depth, merged4=merged, obj_weights=att.weights, obj_depth=att.depth, instance=att.instance, winner=winner), fields
    image4, depth, merged = HipCombineOps.select_composite(fields, nears, fars, bgs, want_merged=True)
    return dict(image4=image4, depth=depth, merged4=merged), fields


def _got(culled, nears, fars, ids, n_obj, bgs=(1.0, 0.0)):
    from focnerf_amd.combine import HipCombineOps
    if n_obj:
        image4, depth, att, merged, winner = HipCombineOps.select_composite_culled(culled, nears, fars, bgs, n_obj, ids=ids, want_merged=True, want_winner=True)
        return dict(image4=image4, depth=depth, merged4=merged, obj_weights=att.weights, obj_depth=att.depth, instance=att.instance, winner=winner)
    image4, depth, att, merged = HipCombineOps.select_composite_culled(culled, nears, fars, bgs, 0, want_merged=True)
    assert att is None
    return dict(image4=image4, depth=depth, merged4=merged)


def _compare(culled, nears, fars, ids, n_obj, tag):
    """both forms of the entry point (with and without attribution) against the two-step path, every output; -> the attributed `want`"""
    out = None
    for n in (n_obj, 0):
        want, fields = _want(culled, nears, fars, ids, n)
        got = _got(culled, nears, fars, ids, n)
        assert set(got) == set(want)
        for name in want:
            _same(got[name], want[name], (tag, n, name))
        out = out or (want, fields)
    return out


def _ids(K, seed):
    """a permutation of K ids out of n_obj > K objects (K = 16 fills the scene: n_obj = 16)"""
    n_obj = min(16, K + 3)
    return [int(v) for v in np.random.default_rng(seed).permutation(n_obj)[:K]], n_obj


# ---------------------------------------------------------------- 1. every shape
@pytest.mark.parametrize("T", [2, 65, 130])
@pytest.mark.parametrize("N", [1, 63, 65, 130])
def test_culled_combine_equals_pack_then_combine(N, T):
    near, far = _near_far(N, N * 1000 + T)
    nears, fars = torch.from_numpy(near).cuda(), torch.from_numpy(far).cuda()
    for K in (1, 2, 5, 16):
        for density in (0.02, 0.5, 1.0):
            objs = _objects(N, T, K, density, seed=N * 100000 + T * 100 + K)
            ids, n_obj = _ids(K, K + T)
            assert len(set(ids)) == K and max(ids) < n_obj and (n_obj > K or K == 16)
            want, _ = _compare([o.dev() for o in objs], nears, fars, ids, n_obj, (N, T, K, density))
            if density == 1.0:                                       # something is rendered and attributed
                assert (want["image4"][1, :, :3] > 0).any() and (want["instance"] >= 0).all()
                assert set(want["winner"].unique().tolist()) <= set(ids)


# ---------------------------------------------------------------- 2. the named cases
def test_named_cases():
    N, T, K = 130, 130, 3
    objs = _objects(N, T, K, 0.3, seed=42)
    a, b, c = objs
    assert (a.gain, b.gain, c.gain) == GAINS and {o.density_scale for o in objs} == set(SCALES) and len({o.thresh for o in objs}) == 3
    near, far = _near_far(N, 42)

    def rebuild(o, occ, seed):
        """the object with another mask: its compact arrays drawn again for the new list"""
        rng = np.random.default_rng(seed)
        m = int(occ.sum())
        return Obj(N, occ, rng.gamma(0.7, 20.0, m), rng.uniform(0.1, 1.0, (m, 3)), o.density_scale, o.thresh, o.gain)

    occ = [o.occ.copy() for o in objs]
    r_empty, r_last, r_tie, r_miss, r_opaque, r_miss_bits = 3, 70, 10, 64, 129, 20
    for oc in occ:
        oc[r_empty // 64, :, r_empty % 64] = False                   # a ray with no bit in any object
        oc[r_last // 64, :, r_last % 64] = False                     # a ray whose only bits lie in the last tile (samples 128, 129 of object 1)
        oc[r_miss // 64, :, r_miss % 64] = False                     # a miss ray without bits ...
        oc[r_opaque // 64, :, r_opaque % 64] = False
    occ[1][r_last // 64, 128:, r_last % 64] = True
    occ[0][r_tie // 64, 7, r_tie % 64] = occ[1][r_tie // 64, 7, r_tie % 64] = True
    occ[2][r_tie // 64, 7, r_tie % 64] = False
    occ[0][r_opaque // 64, 2:40, r_opaque % 64] = True               # the opaque object, and a second one behind it
    occ[1][r_opaque // 64, 20:30, r_opaque % 64] = True
    a, b, c = (rebuild(o, oc, 50 + k) for k, (o, oc) in enumerate(zip(objs, occ)))
    assert (a.gain, b.gain) == (1.0, 2.0)                            # the tie: 33 * 1 and 16.5 * 2, both exact
    a.sigma_c[a.slot(r_tie, 7)], b.sigma_c[b.slot(r_tie, 7)] = np.float32(33.0), np.float32(16.5)
    for i in range(2, 40):
        a.sigma_c[a.slot(r_opaque, i)] = np.float32(1e4 if i == 2 else 5.0)
    for i in range(20, 30):
        b.sigma_c[b.slot(r_opaque, i)] = np.float32(10.0)        # 20 with its gain: above the 5 in front of it, and far from opaque
    nan_n, nan_i = 40, 11                                            # a NaN density
    occ_nan = c.occ.copy()
    occ_nan[nan_n // 64, nan_i, nan_n % 64] = True
    c = rebuild(c, occ_nan, 60)
    c.sigma_c[c.slot(nan_n, nan_i)] = np.float32("nan")
    near[[r_miss, r_miss_bits]] = far[[r_miss, r_miss_bits]] = FLT_MAX   # ... and one with bits
    empty = rebuild(objs[0], np.zeros_like(occ[0]), 61)                  # an object with m_occ == 0 and null arrays
    objs = [a, b, empty, c]
    culled = [o.dev() for o in objs]
    ids, n_obj = [5, 2, 0, 3], 7
    # ---- the preconditions, on the inputs
    any_bit = np.stack([o.occ for o in objs]).any(0)                 # [nblk, T, 64]
    ray_bits = lambda n: any_bit[n // 64, :, n % 64]
    assert culled[2].m_occ == 0 and culled[2].sigma_c is None and culled[2].rgb_c is None
    assert not ray_bits(r_empty).any() and not ray_bits(r_miss).any() and ray_bits(r_miss_bits).any()
    assert ray_bits(r_last)[128:].all() and not ray_bits(r_last)[:128].any()
    assert np.isnan(c.sigma_c).sum() == 1 and all(np.isfinite(o.sigma_c).all() for o in (a, b))
    assert a.sigma_c[a.slot(r_tie, 7)] * a.gain == b.sigma_c[b.slot(r_tie, 7)] * b.gain and not c.occ[r_tie // 64, 7, r_tie % 64]
    assert not (a.rgb_c[a.slot(r_tie, 7)] == b.rgb_c[b.slot(r_tie, 7)]).any()
    assert {o.gain for o in objs} == set(GAINS) and {o.density_scale for o in objs} == set(SCALES) and len({o.thresh for o in objs}) == 3
    assert near[r_miss] == far[r_miss] == FLT_MAX
    nears, fars = torch.from_numpy(near).cuda(), torch.from_numpy(far).cuda()
    want, fields = _compare(culled, nears, fars, ids, n_obj, "named")
    # ---- and on what the two-step path made of them: the cases are what they claim to be
    merged, winner = want["merged4"], want["winner"]
    assert (merged[r_empty] == 0).all() and (winner[r_empty] == ids[0]).all() and (merged[r_last, :128] == 0).all() and (merged[r_last, 128:, 0] > 0).all()
    assert torch.equal(want["image4"][0, r_empty], torch.ones(4, device="cuda")) and int(want["instance"][r_empty]) == -1
    assert bool(torch.isnan(want["depth"][r_miss])) and bool(torch.isnan(want["depth"][r_miss_bits]))        # 0 * NaN, as the dense composite has it
    assert int(winner[r_tie, 7]) == ids[0] and float(merged[r_tie, 7, 0]) == 33.0                            # the first keeps the tie ...
    assert torch.equal(merged[r_tie, 7, 1:], torch.from_numpy(a.rgb_c[a.slot(r_tie, 7)]).cuda())             # ... with its own rgb
    assert bool(torch.isnan(merged[nan_n, nan_i, 0]))
    # the opaque object: its own samples behind sample 2 fail w > thresh (rgb 0, density kept) ...
    assert float(fields[0][r_opaque, 2, 0]) == 1e4 and (fields[0][r_opaque, 3:40, 0] == 5.0).all() and (fields[0][r_opaque, 3:40, 1:] == 0).all()
    # ... while the second object behind it wins the select there and keeps its rgb: the mask is the object's own transmittance
    assert (winner[r_opaque, 20:30] == ids[1]).all() and (merged[r_opaque, 20:30, 1:] > 0).all() and (merged[r_opaque, 30:40, 1:] == 0).all()


# ---------------------------------------------------------------- 3. refusals and N = 0
def test_refusals_leave_the_outputs_untouched_and_no_rays_is_ok():
    from focnerf_amd._lib import lib, ptr, FocCulledField
    N, T, K = 65, 8, 2
    objs = [o.dev() for o in _objects(N, T, K, 0.5, seed=9)]
    near, far = _near_far(N, 9)
    nears, fars = torch.from_numpy(near).cuda(), torch.from_numpy(far).cuda()
    outs = dict(image4=torch.full((2, N, 4), 7.0, device="cuda"), depth=torch.full((N,), 7.0, device="cuda"), merged4=torch.full((N, T, 4), 7.0, device="cuda"),
                obj_weights=torch.full((N, 4), 7.0, device="cuda"), obj_depth=torch.full((N, 4), 7.0, device="cuda"),
                instance=torch.full((N,), 7, dtype=torch.int32, device="cuda"), winner=torch.full((N, T), 7, dtype=torch.uint8, device="cuda"))
    bgs = (ctypes.c_float * 2)(1.0, 0.0)

    def call(**kw):
        a = dict(K=K, struct_bytes=ctypes.sizeof(FocCulledField), ids=(ctypes.c_uint32 * 16)(1, 3), n_obj=4, nears=ptr(nears), fars=ptr(fars), N=N, T=T,
                 bgs=bgs, n_bg=2, edit=None, **{k: ptr(v) for k, v in outs.items()})
        a.update(kw)
        arr = (FocCulledField * 17)()
        for k in range(17):
            c = objs[k % K]
            arr[k].mask, arr[k].offsets, arr[k].sigma_c, arr[k].rgb_c = c.mask.data_ptr(), c.offsets.data_ptr(), c.sigma_c.data_ptr(), c.rgb_c.data_ptr()
            arr[k].m_occ, arr[k].density_scale, arr[k].thresh, arr[k].sigma_gain = c.m_occ, c.density_scale, c.thresh, c.sigma_gain
        if a["edit"]:
            a["edit"](arr[1])
        return lib.foc_combine_select_composite_culled(arr, a["K"], a["struct_bytes"], a["ids"], a["n_obj"], a["nears"], a["fars"], a["N"], a["T"], a["bgs"],
                                                       a["n_bg"], a["image4"], a["depth"], a["merged4"], a["obj_weights"], a["obj_depth"], a["instance"],
                                                       a["winner"], None)

    def field(name, value):
        return lambda o: setattr(o, name, value)
    refused = [dict(K=0), dict(K=17), dict(struct_bytes=40), dict(nears=None), dict(fars=None), dict(image4=None), dict(depth=None),
               dict(edit=field("mask", None)), dict(edit=field("offsets", None)), dict(edit=field("sigma_c", None)), dict(edit=field("rgb_c", None)),
               dict(n_bg=0), dict(n_bg=3), dict(T=1), dict(N=1 << 22, T=512), dict(ids=(ctypes.c_uint32 * 16)(1, 4)), dict(n_obj=17),
               dict(obj_weights=None), dict(obj_depth=None), dict(instance=None)]
    refused += [dict(edit=field("sigma_gain", g)) for g in (0.0, -1.0, float("nan"), float("inf"))]
    for kw in refused:
        assert call(**kw) == 1 and lib.foc_last_error().startswith(b"combine_select_composite_culled:"), kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert call(N=0) == 0 and call(N=0, n_obj=0, obj_weights=None, obj_depth=None, instance=None, winner=None) == 0
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert call() == 0                                               # the same arguments, unedited, are served
    torch.cuda.synchronize()
    assert not any(bool((v == 7).all()) for v in outs.values())
    from focnerf_amd.combine import combine_culled
    with pytest.raises(ValueError, match="1 to 16 objects"):
        combine_culled([objs[0]] * 17, nears, fars)


# ---------------------------------------------------------------- 4. three placed networks
H = 128


def _box(b):
    return torch.tensor([-float(b)] * 3 + [float(b)] * 3, dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _model(seed):
    from focnerf_amd import network
    torch.manual_seed(seed)
    m = network.NeRFNetwork(bound=1, cuda_ray=False).cuda().eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


@functools.lru_cache(maxsize=None)
def _sphere():
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.fixedcull import Occupancy
    grid = synthetic.analytic_density_grid(1, radius_frac=0.35, device="cuda")
    return Occupancy(raymarching.packbits(grid, 25.0), grid.shape[0], H, 1)


def _scene_of_three():
    """tests/test_gpu_placement.py's scene: model A twice (left, small and turned; right, as trained) and model B in the middle, in the box +-2."""
    from focnerf_amd import Placement
    placements = [Placement.rotated((1, 2, 3), 37, translation=(-1.2, 0.1, 0.0), scale=0.75), Placement(translation=(1.0, -0.1, 0.1)), Placement()]
    return 2, [_model(20), _model(20), _model(21)], [_sphere()] * 3, placements


def _bundle_rays(N, placements, seed=8):
    """three bundles down the z axis, each aimed at one object's centre: every object owns rays"""
    rng = np.random.default_rng(seed)
    target = np.stack([placements[k % 3].translation for k in range(N)])
    o = target + np.concatenate([rng.uniform(-0.3, 0.3, size=(N, 2)), np.full((N, 1), 3.0)], -1)
    d = target + rng.uniform(-0.1, 0.1, size=(N, 3)) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()


def test_render_scene_culled_equals_placed_fields_then_combine_packed():
    from focnerf_amd.combine import combine_packed, culled_field_fns, placed_field_fns, render_scene_culled
    N, T = 130, 65
    SB, models, occs, placements = _scene_of_three()
    scene = _box(SB)
    o, d = _bundle_rays(N, placements)
    fns, nears, fars = placed_field_fns(models, occs, placements, o, d, T, scene)
    fields = [fn(0, N) for fn in fns]
    want_img, want_dep, want_att = combine_packed(fields, nears, fars, (1.0, 0.0), attribution=True)
    cfns, c_nears, c_fars = culled_field_fns(models, occs, placements, o, d, T, scene)
    assert torch.equal(c_nears, nears) and torch.equal(c_fars, fars)
    assert all(fn(0, N).m_occ > 0 for fn in cfns) and all((f[..., 0] > 0).any() for f in fields)       # every object has occupied samples
    assert set(want_att.instance.unique().tolist()) >= {0, 1, 2}                                      # ... and owns rays
    img, dep, att = render_scene_culled(models, occs, placements, o, d, T, scene, max_ray_batch=64, attribution=True)
    for name, g, w in [("image4", img, want_img), ("depth", dep, want_dep), ("weights", att.weights, want_att.weights), ("depth_k", att.depth, want_att.depth),
                       ("instance", att.instance, want_att.instance)]:
        _same(g, w, name)
    assert not torch.equal(img[0], img[1])                           # the two backgrounds
    img2, dep2 = render_scene_culled(models, occs, placements, o, d, T, scene, max_ray_batch=64)
    _same(img2, want_img, "image4, no attribution")
    _same(dep2, want_dep, "depth, no attribution")


# ---------------------------------------------------------------- 5. culled_field4 is culled_lists + pack, launch for launch
@pytest.mark.parametrize("placed", [False, True])
def test_culled_field4_keeps_its_result_and_its_library_calls(placed, monkeypatch):
    from focnerf_amd import _lib, raymarching
    from focnerf_amd._lib import ptr, stream_of, check
    from focnerf_amd.field import field_infer, field_plan
    from focnerf_amd.fixedcull import culled_field4, fixed_cull, fixed_cull_emit
    N, T = 130, 65
    SB, models, occs, placements = _scene_of_three()
    m, occ, P = models[0], occs[0], placements[1] if placed else None
    scene = _box(SB) if placed else m.aabb_infer
    o, d = _bundle_rays(N, placements) if placed else _bundle_rays(N, [placements[2]] * 3)
    nears, fars = raymarching.near_far_from_aabb(o, d, scene, m.min_near)
    plan = field_plan(m)                                             # (asks the library for an option: outside the count)
    calls = []
    lib = _lib.lib
    for name in _lib.SIGNATURES:                                     # every module calls through this one object: count on it
        def counted(*a, _fn=getattr(lib, name), _name=name):
            calls.append(_name)
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)

    def old_sequence(out):
        """culled_field4 as it stood before culled_lists was cut out of it"""
        obj_aabb = None if P is None else m.aabb_infer
        mask, offsets, count = fixed_cull(o, d, nears, fars, scene, T, occ, P, obj_aabb)
        m_occ = int(count.item())
        enc_in_c, dirs_c = fixed_cull_emit(o, d, nears, fars, scene, T, m.bound, mask, offsets, m_occ, P)
        sigma, rgb = field_infer(m, enc_in_c, dirs_c, dir_div=1, dir_block=0, obj_feat=None)
        if P is not None:
            check(lib.foc_fixed_field_pack_culled_gain(ptr(sigma), ptr(rgb), ptr(mask), ptr(offsets), m_occ, ptr(nears), ptr(fars), N, T, float(m.density_scale),
                                                       1e-10, float(P.sigma_gain), ptr(out), stream_of(out)), "pack")
        else:
            check(lib.foc_fixed_field_pack_culled(ptr(sigma), ptr(rgb), ptr(mask), ptr(offsets), m_occ, ptr(nears), ptr(fars), N, T, float(m.density_scale),
                                                  1e-10, ptr(out), stream_of(out)), "pack")
        return out, m_occ

    want, m_occ = old_sequence(torch.full((N, T, 4), 7.0, device="cuda"))
    want_calls, calls[:] = [c for c in calls if c != "foc_last_error"], []
    got = culled_field4(m, plan, o, d, nears, fars, scene, T, 1e-10, None, torch.full((N, T, 4), 7.0, device="cuda"), occ, P)
    got_calls = [c for c in calls if c != "foc_last_error"]
    assert 0 < m_occ < N * T and (want[..., 0] > 0).any()
    _same(got, want, "field4")
    assert got_calls == want_calls and len(want_calls) >= 4 and want_calls[-1].startswith("foc_fixed_field_pack_culled")
