"""Multi-object combine — the one-object-per-GPU version of COMBINED.py / editable.py.

Reference semantics (COMBINED.py:592-618, 247-251, 141-200): every object network is evaluated on the
SAME rays and the SAME T fixed-step sample positions; per sample the colour of the object with the
highest density wins (strict '>', first checkpoint wins ties); the merged (sigma, rgb) field is
composited once per background. `editable.py` shifts the ray origins of ONE object before its evaluation
(modify_rays_for_object, :443-471) and is otherwise identical.

Sharding: objects are independent until the per-sample select, so rank r holds object r
(or a run of consecutive objects, pre-merged locally — the select is associative over the checkpoint
order) and evaluates it locally. The exchange is BY RAY (`ObjectCombiner.render_view`): every object's
per-sample field travels packed as one float4 per sample (sigma, rgb masked by the object's own weights,
`foc_fixed_field_pack`); per 4096-ray chunk ONE all-to-all hands rank q the q-th slice of the chunk's rays
from every rank — (p-1)/p x 16 B per sample leave each GPU, straight to their destination over the
point-to-point xGMI links, all seven at once — and rank q runs the select over the p objects and the
composite of ITS rays in one kernel (`foc_combine_select_composite`), so the merged field is never stored
or moved. The all-to-all of chunk c is asynchronous and overlaps the field evaluation of chunk c + 1; the
[N,4] images and depths are all-gathered once per view (12.8 MB per background). No keys, no all-reduce:
the strict-'>' rule is applied to the densities themselves, in rank order.

Kept from round 1, for callers that want the reference's merged tensors on every rank: `select` = ONE
all-reduce(MAX) over an order-preserving 64-bit key (float_bits(sigma) << 32 | 0xFFFFFFFF - rank) + ONE
all-reduce(SUM) of rgb masked to the winner (2.4x the bytes, ring-bound), and `render_chunk` on top of it.
`render_chunk_fast` is the cheaper model worded in north_star — each rank composites its own object and
the per-ray (rgb, depth, weight) are summed — which is NOT the reference's semantics (no inter-object
occlusion); it is offered and labelled as such.

The kernels live in libfocnerf_hip.so; `ops` can be replaced by a CPU implementation in the gloo tests,
which exercise only the host/collective logic.
"""
import os
from collections import namedtuple

import torch
import torch.distributed as dist

# Who the combined render came from (include/focnerf.h foc_combine_select_composite_attr): weights [N, n_obj] = each object's soft matte
# (the composite's weights of the samples it won), depth [N, n_obj] = the same sums of weight x normalised depth, instance [N] int32 = the
# object with the largest matte on the ray, -1 on an empty ray.
Attribution = namedtuple("Attribution", "weights depth instance")


class HipCombineOps:
    """Device kernels (include/focnerf.h: foc_combine_*, foc_composite_fixed_steps)."""

    @staticmethod
    def select(dens, rgb, max_dens, best_rgb):
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(dens, rgb, max_dens, best_rgb)
        check(lib.foc_combine_select(ptr(dens), ptr(rgb), ptr(max_dens), ptr(best_rgb), dens.numel(), stream_of(dens)), "combine_select")

    @staticmethod
    def pack_keys(dens, rank):
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(dens)
        keys = torch.empty(dens.shape, dtype=torch.int64, device=dens.device)
        check(lib.foc_combine_pack_keys(ptr(dens), rank, ptr(keys), dens.numel(), stream_of(dens)), "combine_pack_keys")
        return keys

    @staticmethod
    def unpack(keys, rank, rgb):
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(keys, rgb)
        max_dens = torch.empty(keys.shape, dtype=torch.float32, device=keys.device)
        masked = torch.empty(rgb.shape, dtype=torch.float32, device=keys.device)
        check(lib.foc_combine_unpack(ptr(keys), rank, ptr(rgb), ptr(max_dens), ptr(masked), keys.numel(), stream_of(keys)), "combine_unpack")
        return max_dens, masked

    @staticmethod
    def composite(sigmas, rgbs, nears, fars, bg):
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(sigmas, rgbs, nears, fars)
        N, T = sigmas.shape
        image4 = torch.empty(N, 4, dtype=torch.float32, device=sigmas.device)
        depth = torch.empty(N, dtype=torch.float32, device=sigmas.device)
        check(lib.foc_composite_fixed_steps(ptr(sigmas), ptr(rgbs), ptr(nears), ptr(fars), N, T, float(bg), ptr(image4), ptr(depth),
                                            stream_of(sigmas)), "composite_fixed_steps")
        return image4, depth


    @staticmethod
    def select_composite(fields4, nears, fars, bgs, want_merged=False):
        """fields4: K tensors [N,T,4] fp32 (sigma, r, g, b) in checkpoint order -> image4 [len(bgs),N,4], depth [N] (, merged4 [N,T,4])."""
        import ctypes
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(*fields4, nears, fars)
        N, T = fields4[0].shape[0], fields4[0].shape[1]
        for f in fields4:
            if f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (N, T, 4):
                raise RuntimeError("combine select_composite: fields must be contiguous float32 [N,T,4] tensors of one shape")
        dev = fields4[0].device
        K = len(fields4)
        image4 = torch.empty(len(bgs), N, 4, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        merged = torch.empty(N, T, 4, dtype=torch.float32, device=dev) if want_merged else None
        ptrs = (ctypes.c_void_p * K)(*[f.data_ptr() for f in fields4])
        cbgs = (ctypes.c_float * len(bgs))(*[float(b) for b in bgs])
        check(lib.foc_combine_select_composite(ptrs, K, ptr(nears), ptr(fars), N, T, cbgs, len(bgs), ptr(image4), ptr(depth), ptr(merged),
                                               stream_of(fields4[0])), "combine_select_composite")
        return (image4, depth, merged) if want_merged else (image4, depth)

    @staticmethod
    def select4(field4, acc4):
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(field4, acc4)
        if field4.shape != acc4.shape or field4.dtype != torch.float32 or acc4.dtype != torch.float32 or not (field4.is_contiguous() and acc4.is_contiguous()):
            raise RuntimeError("combine select4: two contiguous float32 [...,4] tensors of one shape expected")
        check(lib.foc_combine_select4(ptr(field4), ptr(acc4), field4.numel() // 4, stream_of(acc4)), "combine_select4")

    @staticmethod
    def select_composite_attr(fields4, nears, fars, bgs, n_obj, ids=None, want_merged=False, want_winner=False):
        """`select_composite` that keeps the select's decision. ids: per field its object id (an int) or, for a field pre-merged by
        `select4_ids`, its uint8 [N,T] id plane; default: field k is object k. -> (image4 [len(bgs),N,4], depth [N],
        Attribution(weights [N,n_obj], depth [N,n_obj], instance [N] int32), merged4 [N,T,4] or None, winner [N,T] uint8 or None)."""
        import ctypes
        from ._lib import lib, ptr, stream_of, check, require_cuda
        K = len(fields4)
        ids = list(range(K)) if ids is None else list(ids)
        if len(ids) != K:
            raise RuntimeError(f"combine select_composite_attr: {K} fields but {len(ids)} ids")
        planes = [i for i in ids if torch.is_tensor(i)]
        require_cuda(*fields4, nears, fars, *planes)
        N, T = fields4[0].shape[0], fields4[0].shape[1]
        for f in fields4:
            if f.dtype != torch.float32 or not f.is_contiguous() or tuple(f.shape) != (N, T, 4):
                raise RuntimeError("combine select_composite_attr: fields must be contiguous float32 [N,T,4] tensors of one shape")
        for pl in planes:
            if pl.dtype != torch.uint8 or not pl.is_contiguous() or tuple(pl.shape) != (N, T):
                raise RuntimeError("combine select_composite_attr: an id plane must be a contiguous uint8 [N,T] tensor")
        dev = fields4[0].device
        n_obj = int(n_obj)
        image4 = torch.empty(len(bgs), N, 4, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        merged = torch.empty(N, T, 4, dtype=torch.float32, device=dev) if want_merged else None
        winner = torch.empty(N, T, dtype=torch.uint8, device=dev) if want_winner else None
        att = Attribution(torch.empty(N, max(n_obj, 0), dtype=torch.float32, device=dev), torch.empty(N, max(n_obj, 0), dtype=torch.float32, device=dev),
                          torch.empty(N, dtype=torch.int32, device=dev))
        ptrs = (ctypes.c_void_p * K)(*[f.data_ptr() for f in fields4])
        cplanes = (ctypes.c_void_p * K)(*[i.data_ptr() if torch.is_tensor(i) else None for i in ids])
        cids = (ctypes.c_uint32 * K)(*[0 if torch.is_tensor(i) else int(i) for i in ids])
        cbgs = (ctypes.c_float * len(bgs))(*[float(b) for b in bgs])
        check(lib.foc_combine_select_composite_attr(ptrs, K, cplanes, cids, n_obj, ptr(nears), ptr(fars), N, T, cbgs, len(bgs), ptr(image4), ptr(depth),
                                                    ptr(merged), ptr(att.weights), ptr(att.depth), ptr(att.instance), ptr(winner),
                                                    stream_of(fields4[0])), "combine_select_composite_attr")
        return image4, depth, att, merged, winner

    @staticmethod
    def select_composite_culled(culled, nears, fars, bgs, n_obj=0, ids=None, want_merged=False, want_winner=False):
        """`select_composite` / `select_composite_attr` from K objects' `fixedcull.CulledField` lists (one chunk of N rays x T steps, nears /
        fars [N] fp32 contiguous). n_obj = 0: no attribution. -> (image4 [len(bgs),N,4], depth [N], Attribution or None, merged4 or None[,
        winner [N,T] uint8 when want_winner])."""
        import ctypes
        from ._lib import lib, ptr, stream_of, check, require_cuda, FocCulledField
        K, N, T, n_obj = len(culled), culled[0].N, culled[0].T, int(n_obj)
        require_cuda(nears, fars, *[t for c in culled for t in (c.mask, c.offsets, c.sigma_c, c.rgb_c)])
        dev = nears.device
        objs = (FocCulledField * K)()
        for o, c in zip(objs, culled):
            o.mask, o.offsets, o.sigma_c, o.rgb_c = (None if t is None else t.data_ptr() for t in (c.mask, c.offsets, c.sigma_c, c.rgb_c))
            o.m_occ, o.density_scale, o.thresh, o.sigma_gain = c.m_occ, c.density_scale, c.thresh, c.sigma_gain
        image4 = torch.empty(len(bgs), N, 4, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        merged = torch.empty(N, T, 4, dtype=torch.float32, device=dev) if want_merged else None
        winner = torch.empty(N, T, dtype=torch.uint8, device=dev) if want_winner and n_obj else None
        att = Attribution(torch.empty(N, n_obj, dtype=torch.float32, device=dev), torch.empty(N, n_obj, dtype=torch.float32, device=dev),
                          torch.empty(N, dtype=torch.int32, device=dev)) if n_obj else None
        cids = None if ids is None else (ctypes.c_uint32 * K)(*[int(i) for i in ids])
        cbgs = (ctypes.c_float * len(bgs))(*[float(b) for b in bgs])
        check(lib.foc_combine_select_composite_culled(objs, K, ctypes.sizeof(FocCulledField), cids, n_obj, ptr(nears), ptr(fars), N, T, cbgs, len(bgs),
                                                      ptr(image4), ptr(depth), ptr(merged), ptr(att.weights if att else None),
                                                      ptr(att.depth if att else None), ptr(att.instance if att else None), ptr(winner),
                                                      stream_of(nears)), "combine_select_composite_culled")
        return (image4, depth, att, merged, winner) if want_winner else (image4, depth, att, merged)

    @staticmethod
    def select4_ids(field4, obj_id, acc4, acc_ids):
        """`select4` that keeps the identity: acc_ids (uint8, one per sample of acc4) takes `obj_id` where acc4 takes field4's rgb."""
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(field4, acc4, acc_ids)
        if field4.shape != acc4.shape or field4.dtype != torch.float32 or acc4.dtype != torch.float32 or not (field4.is_contiguous() and acc4.is_contiguous()):
            raise RuntimeError("combine select4_ids: two contiguous float32 [...,4] tensors of one shape expected")
        if acc_ids.dtype != torch.uint8 or not acc_ids.is_contiguous() or acc_ids.shape != acc4.shape[:-1]:
            raise RuntimeError("combine select4_ids: acc_ids must be a contiguous uint8 tensor with one entry per sample of acc4")
        check(lib.foc_combine_select4_ids(ptr(field4), int(obj_id), ptr(acc4), ptr(acc_ids), field4.numel() // 4, stream_of(acc4)), "combine_select4_ids")

    @staticmethod
    def mo_select(sigma_new, feat_new, sigma_best, feat_best):
        """In place on (sigma_best [n], feat_best [n,w]): MONeRFNetwork's running max (multiobjectnetwork.py:66-82; the new object takes ties)."""
        from ._lib import lib, ptr, stream_of, check, require_cuda
        require_cuda(sigma_new, feat_new, sigma_best, feat_best)
        ts = (sigma_new, feat_new, sigma_best, feat_best)
        if (len({t.dtype for t in ts}) != 1 or sigma_new.dtype not in (torch.float16, torch.float32) or not all(t.is_contiguous() for t in ts)
                or sigma_new.shape != sigma_best.shape or feat_new.shape != feat_best.shape or feat_new.dim() != sigma_new.dim() + 1
                or feat_new.shape[:-1] != sigma_new.shape):
            raise RuntimeError("mo_select: contiguous sigma [...], feat [..., w] pairs of one dtype (float16 or float32) expected")
        check(lib.foc_mo_select(ptr(sigma_new), ptr(feat_new), ptr(sigma_best), ptr(feat_best), sigma_new.numel(), feat_new.shape[-1],
                                sigma_new.element_size(), stream_of(sigma_best)), "mo_select")


def composite_fixed_steps(sigmas, rgbs, nears, fars, bg, ops=HipCombineOps):
    """image_depth_generation of COMBINED.py:141-200: [N,T] sigmas, [N,T,3] rgbs -> image [N,4] (rgb + sum w*sigma, clamped), depth [N]."""
    return ops.composite(sigmas.contiguous().float(), rgbs.contiguous().float(), nears.contiguous().float(), fars.contiguous().float(), bg)


def combine_serial(fields, ops=HipCombineOps):
    """Single-process combine of K objects' (densities [N,T], rgbs [N,T,3]) in checkpoint order (COMBINED.py:609-618)."""
    max_d, best = None, None
    for dens, rgb in fields:
        dens = dens.contiguous().float()
        rgb = rgb.contiguous().float()
        if max_d is None:
            max_d, best = dens.clone(), rgb.clone()
        else:
            ops.select(dens, rgb, max_d, best)
    return max_d, best


def modify_rays_for_object(rays_o, offset, rays_d=None):
    """editable.py:451-462, the edited object's branch: origins + (offset_x, offset_y, offset_z) in fp32 (in-place adds of Python floats
    on fp32 columns), directions re-normalised with F.normalize (eps 1e-12). Returns the new origins, or (origins, directions) when
    `rays_d` is given."""
    new_o = rays_o + torch.as_tensor(offset, dtype=rays_o.dtype, device=rays_o.device)
    if rays_d is None:
        return new_o
    return new_o, torch.nn.functional.normalize(rays_d, dim=-1)


_EDITABLE_OBJECT_TYPES = ('book', 'chair', 'bottle', 'cup')


def object_type_from_ckpt(ckpt):
    """editable.py:500-508: the first of ['book', 'chair', 'bottle', 'cup'] that occurs as a SUBSTRING of the checkpoint path, else None
    ('ws/cupboard/ngp.pth' is a 'cup', 'ws/notebook/...' a 'book')."""
    for t in _EDITABLE_OBJECT_TYPES:
        if t in ckpt:
            return t
    return None


class RayEditor:
    """editable.py's `modify_rays_for_object` (:443-471) with its state. The object named `edit_object` is evaluated on shifted rays
    (see above). Every OTHER object is evaluated on the rays of the FIRST view that reached this method — the reference stores them in
    `self.first_rays_o / first_rays_d` on the first call of its else-branch and returns those ever after (:465-471), for every later
    view as well. That is what the reference computes, so it is what `freeze_first_view=True` (the default) reproduces;
    `freeze_first_view=False` gives the evidently intended behaviour (unedited objects see the current view's rays)."""

    def __init__(self, edit_object, offset=(0.01, 0.01, 0.60), freeze_first_view=True):      # defaults: editable.py:76-79
        self.edit_object, self.offset, self.freeze_first_view = edit_object, tuple(float(v) for v in offset), freeze_first_view
        self.first_rays_o = self.first_rays_d = None

    def __call__(self, rays_o, rays_d, object_type):
        if object_type == self.edit_object:
            return modify_rays_for_object(rays_o, self.offset, rays_d)
        if not self.freeze_first_view:
            return rays_o, rays_d
        if self.first_rays_o is None or self.first_rays_d is None:
            self.first_rays_o, self.first_rays_d = rays_o.clone(), rays_d.clone()
        return self.first_rays_o, self.first_rays_d


def pack_field4(densities, rgbs):
    """(densities [N,T] or [N,T,1], rgbs [N,T,3]) as `run(..., return_fields=True)` returns them -> packed [N,T,4] fp32 (torch ops; the
    fused producer is fixedstep.render_field4)."""
    d = densities.reshape(rgbs.shape[0], rgbs.shape[1], 1).float()
    return torch.cat([d, rgbs.float()], dim=-1).contiguous()


def combine_packed(fields4, nears, fars, bgs=(1.0, 0.0), want_merged=False, ops=HipCombineOps, attribution=False):
    """K resident objects on ONE device: the object loop of COMBINED.py:598-618 and image_depth_generation for every background in one
    pass over the packed fields of a ray chunk. fields4: list of [N,T,4] in checkpoint order (more than 16: pre-merged in runs).
    `attribution=True` (at most 16 fields; field k is object k) appends an `Attribution` to the returned tuple: every object's matte and
    depth per ray and the instance map, from the same pass."""
    fields4 = list(fields4)
    if attribution:
        if len(fields4) > 16:
            raise ValueError(f"combine_packed: attribution covers at most 16 objects, got {len(fields4)} fields")
        image4, depth, att, merged, _ = ops.select_composite_attr(fields4, nears.contiguous().float(), fars.contiguous().float(), tuple(bgs), len(fields4),
                                                                  want_merged=want_merged)
        return (image4, depth, merged, att) if want_merged else (image4, depth, att)
    while len(fields4) > 16:                                   # kernel argument block holds 16 pointers
        acc = fields4[0].clone()
        for f in fields4[1:16]:
            ops.select4(f, acc)
        fields4 = [acc] + fields4[16:]
    return ops.select_composite(fields4, nears.contiguous().float(), fars.contiguous().float(), tuple(bgs), want_merged)


def _placed_scene(who, models, occupancies, placements, rays_o, rays_d, T, scene_aabb, yolo_details, channels="rgb"):
    """The arguments of `placed_field_fns` / `culled_field_fns`, checked: -> (per-object (model, plan, occupancy, placement, yolo) tuples,
    rays_o, rays_d, T, box, nears, fars)."""
    from . import raymarching
    from .field import field_plan
    from .fixedcull import _check_culled, _scene_box
    from .normals import check_channels
    from .placement import Placement
    models, occupancies = list(models), list(occupancies)
    placements = [Placement() if p is None else p for p in placements]
    yolos = [None] * len(models) if yolo_details is None else list(yolo_details)
    if not (len(models) == len(occupancies) == len(placements) == len(yolos)) or not models:
        raise ValueError(f"{who}: {len(models)} models, {len(occupancies)} occupancies, {len(placements)} placements, {len(yolos)} "
                         "yolo_details: one of each per object, at least one object")
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    T = int(T)
    plans = [field_plan(m) for m in models]
    for m, plan, occ, p in zip(models, plans, occupancies, placements):
        if not isinstance(p, Placement):
            raise ValueError(f"{who}: placements must be focnerf_amd.Placement objects (or None for the identity)")
        _check_culled(m, plan, occ)
        check_channels(who, channels, plan)
        if float(m.min_near) != float(models[0].min_near):
            raise ValueError(f"{who}: the objects must share min_near (one near / far per ray): {float(m.min_near)} and "
                             f"{float(models[0].min_near)}")
    box = _scene_box(scene_aabb, models[0], rays_o.device)
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, box, models[0].min_near)
    return list(zip(models, plans, occupancies, placements, yolos)), rays_o, rays_d, T, box, nears, fars


def placed_field_fns(models, occupancies, placements, rays_o, rays_d, T, scene_aabb, yolo_details=None, weight_thresh=1e-10, channels="rgb"):
    """Objects placed in one scene, ready for the combiner: -> (field_fns, nears, fars) for `ObjectCombiner.render_view(field_fns, N, nears,
    fars, T, ...)` and `combine_packed`. Entry k is `models[k]` with its `occupancies[k]` (a `fixedcull.Occupancy`) under `placements[k]`
    (a `Placement`; None = the identity) — the same model may appear more than once with different placements, and hiding an object
    means leaving it out. rays_o / rays_d [N,3]: the view's rays; scene_aabb: float32 [6] tensor on their device. nears / fars [N] are
    those of the view's rays against the scene's box (the first model's `min_near`, which all must share): every field is built along
    them, and the composite must run along the same. yolo_details: None, or one entry per object. channels="normal": every field carries
    its encoded surface normals (rotated into the scene) where the colour stands (`render_field4`); every network must be one the
    normals kernel serves (ValueError otherwise)."""
    from .fixedcull import culled_field4
    objects, rays_o, rays_d, T, box, nears, fars = _placed_scene("placed_field_fns", models, occupancies, placements, rays_o, rays_d, T, scene_aabb,
                                                                 yolo_details, channels)

    def make(m, plan, occ, p, yolo):
        def fn(lo, hi, out=None):
            if out is None:
                out = torch.empty(hi - lo, T, 4, dtype=torch.float32, device=rays_o.device)
            return culled_field4(m, plan, rays_o[lo:hi], rays_d[lo:hi], nears[lo:hi], fars[lo:hi], box, T, weight_thresh, yolo, out, occ, p, channels)
        return fn
    return [make(*args) for args in objects], nears, fars


def culled_field_fns(models, occupancies, placements, rays_o, rays_d, T, scene_aabb, yolo_details=None, weight_thresh=1e-10, channels="rgb"):
    """`placed_field_fns` for `combine_culled`: the same arguments and checks -> (fns, nears, fars), but `fns[k](lo, hi)` (hi > lo) stops in
    front of the pack and returns the object's `fixedcull.CulledField` on rays lo:hi — no [hi-lo, T, 4] field is written."""
    from .fixedcull import culled_lists
    objects, rays_o, rays_d, T, box, nears, fars = _placed_scene("culled_field_fns", models, occupancies, placements, rays_o, rays_d, T, scene_aabb,
                                                                 yolo_details, channels)

    def make(m, plan, occ, p, yolo):
        def fn(lo, hi):
            if not 0 <= lo < hi <= rays_o.shape[0]:
                raise ValueError(f"culled_field_fns: rays {lo}:{hi} of {rays_o.shape[0]}: a non-empty range of the view's rays expected")
            return culled_lists(m, plan, rays_o[lo:hi], rays_d[lo:hi], nears[lo:hi], fars[lo:hi], box, T, weight_thresh, yolo, occ, p, channels)
        return fn
    return [make(*args) for args in objects], nears, fars


def combine_culled(culled, nears, fars, bgs=(1.0, 0.0), want_merged=False, attribution=False, ops=HipCombineOps):
    """`combine_packed` fed from the compact culled lists (include/focnerf.h foc_combine_select_composite_culled): culled = one
    `fixedcull.CulledField` per object in checkpoint order, all on the same N rays and T steps as nears / fars [N]. Returns what
    `combine_packed` returns for the objects' packed fields, bit for bit: (image4 [len(bgs),N,4], depth [N][, merged4 [N,T,4]][, Attribution]).
    At most 16 objects: more need the dense pre-merge (`combine_packed`)."""
    from .fixedcull import CulledField
    culled = list(culled)
    if not culled or len(culled) > 16:
        raise ValueError(f"combine_culled: 1 to 16 objects per call, got {len(culled)} (more than 16: the dense path pre-merges, combine_packed)")
    for c in culled:
        if not isinstance(c, CulledField):
            raise ValueError("combine_culled: the objects must be focnerf_amd.fixedcull.CulledField (what culled_field_fns' functions return)")
        if (c.N, c.T) != (culled[0].N, culled[0].T):
            raise ValueError(f"combine_culled: objects on {c.N} rays x {c.T} steps and on {culled[0].N} x {culled[0].T}: one chunk, one T expected")
    if nears.numel() != culled[0].N or fars.numel() != culled[0].N:
        raise ValueError(f"combine_culled: nears / fars of {nears.numel()} / {fars.numel()} rays, the objects' lists cover {culled[0].N}")
    image4, depth, att, merged = ops.select_composite_culled(culled, nears.contiguous().float(), fars.contiguous().float(), tuple(bgs),
                                                             len(culled) if attribution else 0, want_merged=want_merged)
    out = (image4, depth, merged) if want_merged else (image4, depth)
    return out + (att,) if attribution else out


def render_scene_culled(models, occupancies, placements, rays_o, rays_d, T, scene_aabb, bgs=(1.0, 0.0), max_ray_batch=16384, attribution=False,
                        yolo_details=None, channels="rgb"):
    """One view of placed objects on ONE device through `culled_field_fns` + `combine_culled`, in chunks of `max_ray_batch` rays:
    -> (image4 [len(bgs),N,4], depth [N][, Attribution]). The bits of `placed_field_fns` + `combine_packed` without the objects' dense
    fields; every object still costs one host read of its occupied count per chunk. channels="normal": a normal view of the scene
    (`normals.decode_normal_map` of image4 for bgs (1, 0)); depth and attribution are those of the colour view."""
    fns, nears, fars = culled_field_fns(models, occupancies, placements, rays_o, rays_d, T, scene_aabb, yolo_details, channels=channels)
    N, dev, chunk, n_obj = nears.shape[0], nears.device, int(max_ray_batch), len(fns)
    if chunk < 1:
        raise ValueError(f"render_scene_culled: max_ray_batch must be >= 1, got {chunk}")
    image4 = torch.empty(len(bgs), N, 4, dtype=torch.float32, device=dev)
    depth = torch.empty(N, dtype=torch.float32, device=dev)
    att = Attribution(torch.empty(N, n_obj, dtype=torch.float32, device=dev), torch.empty(N, n_obj, dtype=torch.float32, device=dev),
                      torch.empty(N, dtype=torch.int32, device=dev)) if attribution else None
    for lo in range(0, N, chunk):
        hi = min(lo + chunk, N)
        out = combine_culled([fn(lo, hi) for fn in fns], nears[lo:hi], fars[lo:hi], bgs, attribution=attribution)
        image4[:, lo:hi], depth[lo:hi] = out[0], out[1]
        if attribution:
            att.weights[lo:hi], att.depth[lo:hi], att.instance[lo:hi] = out[2]
    return (image4, depth, att) if attribution else (image4, depth)


class ObjectCombiner:
    """One object per rank. All tensors live on the rank's device; collectives go over `group`
    (backend nccl == RCCL on ROCm, gloo in the CPU tests)."""

    def __init__(self, rank=None, world_size=None, group=None, ops=HipCombineOps, collectives_at_world_1=False):
        self.group = group
        self.rank = dist.get_rank(group) if rank is None else rank
        self.world = dist.get_world_size(group) if world_size is None else world_size
        self.ops = ops
        # A single rank needs no exchange and issues none. `collectives_at_world_1` issues every collective anyway (needs an initialised
        # process group of one rank): the rehearsal of the RCCL path — buffers, split sizes, the order of the collective's stream against
        # this library's launches — on a box with one GPU (tests/test_gpu_rccl.py). Same results either way.
        self.xch = self.world > 1 or bool(collectives_at_world_1)
        self._side = {}                # device index -> the stream render_view evaluates on while collectives are in flight
        self.bytes_sent = 0            # bytes this rank put on the wire in the last render_view

    # ---- faithful per-sample select across ranks
    def select(self, dens, rgb):
        """dens [N,T] fp32 (>= 0), rgb [N,T,3] fp32 of THIS rank's object -> merged (max_dens, best_rgb), identical on all ranks."""
        dens = dens.contiguous().float()
        rgb = rgb.contiguous().float()
        keys = self.ops.pack_keys(dens, self.rank)
        if self.xch:
            dist.all_reduce(keys, op=dist.ReduceOp.MAX, group=self.group)
        max_dens, masked = self.ops.unpack(keys, self.rank, rgb)
        if self.xch:
            dist.all_reduce(masked, op=dist.ReduceOp.SUM, group=self.group)
        return max_dens, masked

    def ray_slice(self, N):
        per = (N + self.world - 1) // self.world
        lo = min(self.rank * per, N)
        return lo, min(lo + per, N), per

    def render_chunk(self, dens, rgb, nears, fars, bg=1.0):
        """Faithful combine of one ray chunk: select across ranks, composite this rank's slice of rays,
        all-gather the [N,4] image and [N] depth. Returns (image4, depth) for the whole chunk on every rank."""
        N = dens.shape[0]
        max_dens, best = self.select(dens, rgb)
        lo, hi, per = self.ray_slice(N)
        img = torch.zeros(per, 4, dtype=torch.float32, device=dens.device)
        dep = torch.zeros(per, dtype=torch.float32, device=dens.device)
        if hi > lo:
            i4, d = self.ops.composite(max_dens[lo:hi].contiguous(), best[lo:hi].contiguous(), nears[lo:hi].contiguous().float(),
                                       fars[lo:hi].contiguous().float(), bg)
            img[: hi - lo] = i4
            dep[: hi - lo] = d
        if self.xch:
            imgs = [torch.empty_like(img) for _ in range(self.world)]
            deps = [torch.empty_like(dep) for _ in range(self.world)]
            dist.all_gather(imgs, img, group=self.group)
            dist.all_gather(deps, dep, group=self.group)
            img, dep = torch.cat(imgs)[:N], torch.cat(deps)[:N]
        else:
            img, dep = img[:N], dep[:N]
        return img, dep

    # ---- exchange by ray: all-to-all of packed fields, fused select + composite on the owner of each ray slice
    def _slice_len(self, n_rays):
        return (n_rays + self.world - 1) // self.world

    def exchange_start(self, field4, bufs=None, ids=None, id_bufs=None):
        """field4 [n,T,4] fp32: this rank's (pre-merged) objects on the n rays of one chunk. Starts the all-to-all that gives rank q rays
        [q*per, (q+1)*per) of every rank's field, per = ceil(n / world) (zero rows pad a ragged chunk). Returns a handle for
        `exchange_finish`; the caller may enqueue other work (the next chunk's field evaluation) in between.
        `bufs` = (send, recv) of [world*per, T, 4] to reuse (double-buffered by render_view), else allocated here.
        `ids` (attribution only): the uint8 [n,T] id plane of field4; it travels in a second all-to-all of uint8 [world*per, T]
        (`id_bufs` = its (send, recv) to reuse) and the handle carries it to `exchange_finish`."""
        n, T = field4.shape[0], field4.shape[1]
        per = self._slice_len(n)
        if not self.xch:
            return (None, field4.contiguous(), n, per) if ids is None else (None, field4.contiguous(), n, per, None, ids.contiguous())
        if bufs is None:
            bufs = (torch.empty(self.world * per, T, 4, dtype=torch.float32, device=field4.device),
                    torch.empty(self.world * per, T, 4, dtype=torch.float32, device=field4.device))
        send, recv = bufs[0][: self.world * per], bufs[1][: self.world * per]
        if send.data_ptr() != field4.data_ptr():
            send[:n].copy_(field4)
        if self.world * per > n:
            send[n:].zero_()
        work = dist.all_to_all_single(recv, send, group=self.group, async_op=True)
        self.bytes_sent += (self.world - 1) * per * T * 16
        if ids is not None:
            if id_bufs is None:
                id_bufs = (torch.empty(self.world * per, T, dtype=torch.uint8, device=field4.device),
                           torch.empty(self.world * per, T, dtype=torch.uint8, device=field4.device))
            id_send, id_recv = id_bufs[0][: self.world * per], id_bufs[1][: self.world * per]
            if id_send.data_ptr() != ids.data_ptr():
                id_send[:n].copy_(ids)
            if self.world * per > n:
                id_send[n:].zero_()
            id_work = dist.all_to_all_single(id_recv, id_send, group=self.group, async_op=True)
            self.bytes_sent += (self.world - 1) * per * T
            return (work, recv, n, per, id_work, id_recv)
        return (work, recv, n, per)

    def my_slice(self, values, n, per, fill):
        """This rank's rows [rank*per, (rank+1)*per) of a per-ray vector of a chunk of n rays, padded with `fill` past the chunk's end."""
        lo = min(self.rank * per, n)
        hi = min(lo + per, n)
        out = torch.full((per,), float(fill), dtype=torch.float32, device=values.device)
        out[: hi - lo] = values[lo:hi]
        return out

    def exchange_finish(self, handle, nears_mine, fars_mine, bgs=(1.0, 0.0), n_objects=None):
        """-> (image4 [len(bgs), per, 4], depth [per]) of THIS rank's ray slice of the chunk (rows past the chunk's end are padding).
        nears_mine / fars_mine [per]: `my_slice` of the chunk's nears / fars — of the view's own (unedited) rays, because
        image_depth_generation composites along data['rays_o'] (COMBINED.py:143-149).
        A handle started with `ids` gives (image4, depth, Attribution) of the slice over the scene's `n_objects`: one id plane per
        received field."""
        work, recv, n, per = handle[:4]
        if work is not None:
            work.wait()
        fields = [recv[k * per:(k + 1) * per] for k in range(self.world)] if self.world > 1 else [recv]
        if len(handle) > 4:
            id_work, id_recv = handle[4], handle[5]
            if id_work is not None:
                id_work.wait()
            planes = [id_recv[k * per:(k + 1) * per] for k in range(self.world)] if self.world > 1 else [id_recv]
            return self.ops.select_composite_attr(fields, nears_mine, fars_mine, tuple(bgs), n_objects, ids=planes)[:3]
        return self.ops.select_composite(fields, nears_mine, fars_mine, tuple(bgs))

    def render_view(self, field_fns, n_rays, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=16384, overlap=True, attribution=None):
        """`_render_view` (below), on a stream of this combiner's own while collectives are in flight. Measured with one rank on RCCL
        (tools/time_rccl_one_rank.py, NOTEBOOK.md rounds 1-4 section 7): when RCCL's stream is the first stream a process uses after the default one —
        bench.py at N > 1, or a fresh COMBINED.py-style process — it shares a hardware queue with the DEFAULT stream, and an all-to-all
        "under" a field evaluation enqueued on the default stream runs strictly in turn with it (44.5 ms per view overlapped = not
        overlapped); with the evaluation on any other stream the two run side by side (43.1), whichever of the two was created first.
        To the caller nothing changes: the work is ordered behind what the caller's current stream holds, and the returned tensors
        may be used on that stream. FOC_COMBINE_SIDE_STREAM=0 evaluates on the caller's stream as before.
        `attribution=(first_object, n_objects)` — this rank's first object's index in checkpoint order and the scene's number of objects
        (at most 16) — returns (image4, depth, Attribution) for the whole view on every rank; see `_render_view`."""
        dev = nears.device
        if self.xch and overlap and dev.type == "cuda" and os.environ.get("FOC_COMBINE_SIDE_STREAM", "1") != "0":
            cur = torch.cuda.current_stream(dev)
            side = self._side.get(dev.index)
            if side is None:
                side = self._side[dev.index] = torch.cuda.Stream(dev)
            if cur != side:
                side.wait_stream(cur)
                try:
                    with torch.cuda.stream(side):
                        out = self._render_view(field_fns, n_rays, nears, fars, T, bgs, max_ray_batch, overlap, attribution)
                finally:
                    cur.wait_stream(side)              # also when a field function raised: kernels on `side` may still read the caller's buffers
                for t in out[:2] + (tuple(out[2]) if attribution is not None else ()):
                    t.record_stream(cur)               # allocated under `side`, consumed by the caller on `cur`
                return out
        return self._render_view(field_fns, n_rays, nears, fars, T, bgs, max_ray_batch, overlap, attribution)

    def _render_view(self, field_fns, n_rays, nears, fars, T, bgs=(1.0, 0.0), max_ray_batch=16384, overlap=True, attribution=None):
        """One view, the loop of COMBINED.py:592-618 + compute_metrics_both_backgrounds' composites, sharded by object and exchanged by ray.
        field_fns: THIS rank's objects in checkpoint order, each `fn(lo, hi, out)` -> packed field4 [hi-lo, T, 4] fp32 of the object on
        rays lo:hi of the view (it may write into `out`, a [hi-lo, T, 4] buffer, and return it). Ranks hold consecutive runs of the
        checkpoint list (rank order = checkpoint order). nears / fars [n_rays]: of the view's own rays. `max_ray_batch` = rays per piece (field
        evaluation and exchange granularity; 16384: 134 MB per object and piece at 512 samples — 10 % faster per view than 4096-ray pieces).
        Returns (image4 [len(bgs), n_rays, 4], depth [n_rays]) on every rank.
        attribution = (first_object, n_objects): additionally an Attribution (weights / depth [n_rays, n_objects], instance [n_rays]). The
        protocol is the same on every rank, whatever it holds: a uint8 [n,T] id plane per piece — filled with the first local object's id,
        the later ones pre-merged with `select4_ids` — travels in a second all-to-all beside the field's, the owner of a ray slice runs
        `select_composite_attr` with one plane per received field, and the view's gather carries the three extra tensors in its one
        flat buffer (instance bit-viewed as float32)."""
        dev = nears.device
        p, chunk = self.world, int(max_ray_batch)
        n_chunks = (n_rays + chunk - 1) // chunk
        first_obj, n_obj = (int(attribution[0]), int(attribution[1])) if attribution is not None else (0, 0)
        if attribution is not None and not (1 <= n_obj <= 16 and 0 <= first_obj and first_obj + len(field_fns) <= n_obj):
            raise ValueError(f"render_view: attribution=(first_object={first_obj}, n_objects={n_obj}) with {len(field_fns)} local objects: "
                             "1 <= n_objects <= 16 and first_object + local objects <= n_objects expected")
        if n_chunks == 0:
            if attribution is not None:
                return (torch.zeros(len(bgs), 0, 4, device=dev), torch.zeros(0, device=dev),
                        Attribution(torch.zeros(0, n_obj, device=dev), torch.zeros(0, n_obj, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)))
            return torch.zeros(len(bgs), 0, 4, device=dev), torch.zeros(0, device=dev)
        per = self._slice_len(min(chunk, n_rays))                          # slice length of a full chunk
        n_last = n_rays - (n_chunks - 1) * chunk
        per_last = self._slice_len(n_last)                                 # ... and of the (possibly shorter) last one
        # this rank's nears / fars for every chunk, once per view: row j of chunk c is ray c*chunk + rank*per_c + j
        j = torch.arange(per, device=dev)
        pc = torch.full((n_chunks, 1), per, device=dev, dtype=torch.long)
        pc[-1, 0] = per_last
        nc = torch.full((n_chunks, 1), chunk, device=dev, dtype=torch.long)
        nc[-1, 0] = n_last
        within = self.rank * pc + j[None, :]
        ok = (j[None, :] < pc) & (within < nc)
        ray = (torch.arange(n_chunks, device=dev)[:, None] * chunk + within).clamp(max=n_rays - 1)
        near_tab = torch.where(ok, nears.float()[ray], torch.ones((), device=dev)).contiguous()
        far_tab = torch.where(ok, fars.float()[ray], torch.full((), 2.0, device=dev)).contiguous()
        mine4 = torch.zeros(n_chunks, len(bgs), per, 4, dtype=torch.float32, device=dev)
        mined = torch.zeros(n_chunks, per, dtype=torch.float32, device=dev)
        bufs = [tuple(torch.empty(p * per, T, 4, dtype=torch.float32, device=dev) for _ in range(2)) for _ in range(2)] if self.xch else None
        if attribution is not None:
            minew = torch.zeros(n_chunks, per, n_obj, dtype=torch.float32, device=dev)
            minez = torch.zeros(n_chunks, per, n_obj, dtype=torch.float32, device=dev)
            minei = torch.full((n_chunks, per), -1, dtype=torch.int32, device=dev)
            # the id planes are double-buffered like the fields: [send, recv] x 2 with an exchange, else one plane per piece in turn
            id_bufs = [tuple(torch.empty(p * per, T, dtype=torch.uint8, device=dev) for _ in range(2)) for _ in range(2)]
        self.bytes_sent = 0

        def finish(pending):
            handle, c = pending
            k = handle[3]
            if attribution is not None:
                i4, d, att = self.exchange_finish(handle, near_tab[c, :k], far_tab[c, :k], bgs, n_objects=n_obj)
                minew[c, :k], minez[c, :k], minei[c, :k] = att.weights, att.depth, att.instance
            else:
                i4, d = self.exchange_finish(handle, near_tab[c, :k], far_tab[c, :k], bgs)
            mine4[c, :, :k] = i4
            mined[c, :k] = d

        pending = None
        for c in range(n_chunks):
            lo, hi = c * chunk, min((c + 1) * chunk, n_rays)
            k = self._slice_len(hi - lo)
            out = bufs[c % 2][0][: hi - lo] if bufs is not None else None
            acc = None
            plane = id_bufs[c % 2][0][: hi - lo].fill_(first_obj) if attribution is not None else None
            for j, fn in enumerate(field_fns):
                f4 = fn(lo, hi, out if acc is None else None)
                if acc is None:
                    acc = f4
                elif plane is not None:
                    self.ops.select4_ids(f4.contiguous(), first_obj + j, acc, plane)    # ... and the plane takes the id where acc takes the rgb
                else:
                    self.ops.select4(f4.contiguous(), acc)                 # this rank's later objects, same strict-'>' rule
            if plane is not None:
                handle = self.exchange_start(acc, (bufs[c % 2][0][: p * k], bufs[c % 2][1][: p * k]) if bufs is not None else None, ids=plane,
                                             id_bufs=(id_bufs[c % 2][0][: p * k], id_bufs[c % 2][1][: p * k]))
            else:
                handle = self.exchange_start(acc, (bufs[c % 2][0][: p * k], bufs[c % 2][1][: p * k]) if bufs is not None else None)
            if pending is not None:
                finish(pending)                                            # chunk c-1: its all-to-all ran under chunk c's evaluation
            pending = (handle, c)
            if not overlap:
                finish(pending)
                pending = None
        if pending is not None:
            finish(pending)
        if not self.xch:
            image4, depth = mine4.permute(1, 0, 2, 3).reshape(len(bgs), -1, 4)[:, :n_rays].contiguous(), mined.reshape(-1)[:n_rays].contiguous()
            if attribution is not None:
                return image4, depth, Attribution(minew.reshape(-1, n_obj)[:n_rays].contiguous(), minez.reshape(-1, n_obj)[:n_rays].contiguous(),
                                                  minei.reshape(-1)[:n_rays].contiguous())
            return image4, depth
        # ONE gather per view: image rows and depths of this rank's slices in one flat buffer
        if attribution is not None:   # ... and the mattes, their depths and the instance map (int32 bits carried as float32; nothing computes on them)
            flat = torch.cat([mine4.reshape(-1), mined.reshape(-1), minew.reshape(-1), minez.reshape(-1), minei.reshape(-1).view(torch.float32)])
        else:
            flat = torch.cat([mine4.reshape(-1), mined.reshape(-1)])
        gathered = torch.empty(p * flat.numel(), dtype=torch.float32, device=dev)
        dist.all_gather_into_tensor(gathered, flat, group=self.group)
        self.bytes_sent += (p - 1) * flat.numel() * 4
        gathered = gathered.view(p, flat.numel())
        g4 = gathered[:, : mine4.numel()].reshape(p, *mine4.shape)
        gd = gathered[:, mine4.numel(): mine4.numel() + mined.numel()].reshape(p, *mined.shape)
        image4 = torch.empty(len(bgs), n_rays, 4, dtype=torch.float32, device=dev)
        depth = torch.empty(n_rays, dtype=torch.float32, device=dev)
        full = n_chunks - 1 if (n_last != chunk or per_last != per) else n_chunks
        if full > 0:   # [rank, chunk, bg, per, 4] -> [bg, chunk, rank*per, 4]; a chunk's rays are the first `chunk` of its p*per rows
            image4[:, : full * chunk] = g4[:, :full].permute(2, 1, 0, 3, 4).reshape(len(bgs), full, p * per, 4)[:, :, :chunk].reshape(len(bgs), -1, 4)
            depth[: full * chunk] = gd[:, :full].permute(1, 0, 2).reshape(full, p * per)[:, :chunk].reshape(-1)
        if full < n_chunks:   # the shorter last chunk was cut into slices of per_last rays
            image4[:, full * chunk:] = g4[:, full, :, :per_last].permute(1, 0, 2, 3).reshape(len(bgs), p * per_last, 4)[:, :n_last]
            depth[full * chunk:] = gd[:, full, :per_last].reshape(p * per_last)[:n_last]
        if attribution is not None:
            def rows(g):                          # [rank, chunk, per, C] of every rank's slices -> [n_rays, C], the same walk as depth's
                o = torch.empty(n_rays, g.shape[-1], dtype=g.dtype, device=dev)
                if full > 0:
                    o[: full * chunk] = g[:, :full].permute(1, 0, 2, 3).reshape(full, p * per, -1)[:, :chunk].reshape(full * chunk, -1)
                if full < n_chunks:
                    o[full * chunk:] = g[:, full, :per_last].reshape(p * per_last, -1)[:n_last]
                return o
            at = mine4.numel() + mined.numel()
            gw = gathered[:, at: at + minew.numel()].reshape(p, *minew.shape)
            gz = gathered[:, at + minew.numel(): at + 2 * minew.numel()].reshape(p, *minew.shape)
            gi = gathered[:, at + 2 * minew.numel():].view(torch.int32).reshape(p, *minei.shape, 1)
            return image4, depth, Attribution(rows(gw), rows(gz), rows(gi).reshape(n_rays))
        return image4, depth

    # ---- north_star's cheaper model: per-ray sums of independently composited objects
    def render_chunk_fast(self, image, depth, weights_sum):
        """image [N,3] (premultiplied, no background), depth [N], weights_sum [N] of this rank's object.
        One all-reduce(SUM) of the packed [N,5]; the caller adds the background with the summed weight."""
        packed = torch.cat([image.float(), depth.float().unsqueeze(-1), weights_sum.float().unsqueeze(-1)], dim=-1).contiguous()
        if self.xch:
            dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=self.group)
        return packed[:, :3], packed[:, 3], packed[:, 4]
