"""A placed scene at arbitrary points: which object wins there, with what density, colour and normal (csrc/mesh.hip: foc_points_cull,
foc_surface_frame, foc_scene_select around the field kernels the renders use).

    s = query_scene(models, placements, x)                   # x [...,3] world units -> SceneSample(sigma, object_id, rgb, normal)
    s = query_scene([model], [None], x, view=(0, 0, 3))      # one object in its own frame, colours as seen from an eye point

Per object and chunk of points: cull (the object's box, then its occupancy grid) -> ONE host read of the count -> emit the compact
encoder coordinates and object-frame positions -> `foc_field_normals` (sigma and the density logit's gradient) -> `foc_surface_frame` (the
world-frame normal, the direction the colour network is asked about) -> encoder + `field_infer` (colour) -> `foc_scene_select`, which keeps
the object whose gained sigma is strictly the largest so far: the select rule of the combined render and of `scene_volume`, once, for
arbitrary points. `mesh.extract_mesh` / `extract_scene_mesh` evaluate it at a mesh's vertices.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ._lib import lib, ptr, stream_of, check
from .backend import _scratch
from .fixedcull import Occupancy, _host_floats
from .placement import Placement

MAX_POINTS = 1 << 29
MODE_NORMAL, MODE_EYE = 0, 1             # foc_surface_frame's `mode`
_WANT = ("rgb", "normal")


@dataclass
class SceneSample:
    """What `query_scene` found at every point: the winning object's density in world units of length (sigma * placement.sigma_gain; 0 in
    empty space), its index into `models` (-1 in empty space), its colour and its unit normal in the world's frame (0 in empty space and
    where the density gradient is zero or not finite). `rgb` / `normal` are None when not asked for."""
    sigma: torch.Tensor
    object_id: torch.Tensor
    rgb: Optional[torch.Tensor]
    normal: Optional[torch.Tensor]


def _at(t, first, width=1):
    """Pointer to row `first` of a contiguous fp32 / int32 tensor with `width` values per row (None -> NULL)."""
    import ctypes
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * width * first)


def points_cull(points, first, count, w2o=None, obj_aabb=None, occupancy=None):
    """foc_points_cull on rows [first, first + count) of `points` [M,3] fp32 (contiguous, on the device): -> (mask int64 [R], offsets int32
    [R + 1], count int32 [1]) with R = ceil(count / 64). w2o / obj_aabb: ctypes arrays of 12 / 6 floats (`_host_floats`), both or neither.
    No host synchronisation."""
    dev = points.device
    R = -(-count // 64)
    mask = torch.empty(R, dtype=torch.int64, device=dev)
    offsets = torch.empty(R + 1, dtype=torch.int32, device=dev)
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.foc_lattice_cull_scratch_bytes(count)
    scratch = _scratch.get("points_cull", nbytes, dev)
    bits, bound, cascade, grid = (None, 0.0, 0, 0) if occupancy is None else (occupancy.bitfield, occupancy.bound, occupancy.cascade, occupancy.grid_size)
    if bits is not None and bits.device != dev:
        raise ValueError(f"points_cull: the occupancy bitfield is on {bits.device}, the points on {dev}")
    check(lib.foc_points_cull(_at(points, first, 3), count, w2o, obj_aabb, bound, ptr(bits), cascade, grid, ptr(mask), ptr(offsets), ptr(n_out), ptr(scratch),
                              nbytes, stream_of(points)), "points_cull")
    return mask, offsets, n_out


def points_cull_emit(points, first, count, mask, offsets, m_occ, bound, w2o=None, want_pos=True, want_xn=True):
    """-> (pos_c, xn_c) fp32 [m_occ,3] of the set points in list order (None where not asked for): the point in the object's frame and
    (pos + bound) / (2 bound)."""
    dev = points.device
    pos = torch.empty(m_occ, 3, dtype=torch.float32, device=dev) if want_pos else None
    xn = torch.empty(m_occ, 3, dtype=torch.float32, device=dev) if want_xn else None
    check(lib.foc_points_cull_emit(_at(points, first, 3), count, w2o, float(bound), ptr(mask), ptr(offsets), m_occ, ptr(pos), ptr(xn), stream_of(points)),
          "points_cull_emit")
    return pos, xn


def surface_frame(grad_raw_c, pos_c, rot9=None, eye_obj=None, want_dirs=True, want_normal=True):
    """foc_surface_frame: -> (dirs_c, normal_c) fp32 [m,3], None where not asked for. rot9 / eye_obj: ctypes arrays of 9 / 3 floats or None
    (eye_obj None: the direction is against the normal)."""
    src = grad_raw_c if grad_raw_c is not None else pos_c
    m, dev = src.shape[0], src.device
    dirs = torch.empty(m, 3, dtype=torch.float32, device=dev) if want_dirs else None
    normal = torch.empty(m, 3, dtype=torch.float32, device=dev) if want_normal else None
    check(lib.foc_surface_frame(ptr(grad_raw_c), ptr(pos_c), m, rot9, MODE_NORMAL if eye_obj is None else MODE_EYE, eye_obj, ptr(dirs), ptr(normal),
                                stream_of(src)), "surface_frame")
    return dirs, normal


def scene_select(sigma_c, rgb_c, normal_c, mask, offsets, gain, object_index, best_sigma, best_id, best_rgb, best_normal, first, count):
    """foc_scene_select on points [first, first + count) of the flat best_* arrays (rgb / normal pairs may be None)."""
    check(lib.foc_scene_select(ptr(sigma_c), ptr(rgb_c), ptr(normal_c), ptr(mask), ptr(offsets), float(gain), int(object_index), _at(best_sigma, first),
                               _at(best_id, first), _at(best_rgb, first, 3), _at(best_normal, first, 3), count, stream_of(best_sigma)), "scene_select")


def _eye_in_object(eye, placement):
    """The eye (world, float64) in the object's frame, rounded once to fp32: 3 floats for the kernel's argument block."""
    A, b = placement.world_to_object64()
    return _host_floats((A @ eye + b).astype(np.float32), 3, "query_scene: view")


@torch.no_grad()
def query_scene(models, placements, x, occupancies=None, yolo_details=None, view="normal", want=("rgb", "normal"), chunk=1 << 22):
    """The placed scene at x [...,3] (world units, on the models' device) -> `SceneSample`: sigma [...] fp32, object_id [...] int32, rgb
    [...,3] and normal [...,3] fp32 (None unless named in `want`).

    placements[k]: a `Placement`, or None for an object in its own frame (the identity placement: the only box test is the object's
    `aabb_infer`). occupancies[k]: an `Occupancy` or None. yolo_details[k]: the object description of an object-conditioned network.
    view: "normal" (the colour network is asked about the direction against the surface normal, (0, 0, -1) where there is none) or an eye
    point, 3 numbers in world units (the direction from the eye to the point).
    A point no object covers reads sigma 0, object_id -1, rgb 0, normal 0 — empty space, as in `scene_volume`. Among the objects that
    cover a point the one with the strictly largest sigma * placement.sigma_gain wins; on a tie the earlier one in `models` stays; a NaN
    never wins. sigma is the fused kernels' (`field_normals` and `field_infer` agree bit for bit); when the normals launch runs, its sigma
    is the one selected by.

    Served: `field_plan(model).infer` for rgb, `.normals` for normals and for view="normal", no background model (bg_radius <= 0);
    ValueError otherwise — there is no fallback. Not capturable in a graph: one host read of the cull's count per object and chunk."""
    from .field import field_plan, field_infer
    from .normals import _launch as normals_launch
    models, placements = list(models), list(placements)
    K = len(models)
    occupancies = [None] * K if occupancies is None else list(occupancies)
    yolo_details = [None] * K if yolo_details is None else list(yolo_details)
    if K == 0 or len(placements) != K or len(occupancies) != K or len(yolo_details) != K:
        raise ValueError("query_scene: one placement (and one occupancy / yolo_details entry or None) per model, at least one model")
    want = (want,) if isinstance(want, str) else tuple(want)
    if any(w not in _WANT for w in want):
        raise ValueError(f"query_scene: want names 'rgb' and / or 'normal', got {want!r}")
    want_rgb, want_normal = "rgb" in want, "normal" in want
    eye = None
    if not (isinstance(view, str) and view == "normal"):
        if isinstance(view, str):
            raise ValueError(f"query_scene: view must be 'normal' or an eye point of 3 numbers, got {view!r}")
        eye = np.asarray(view.detach().cpu().numpy() if torch.is_tensor(view) else view, dtype=np.float64).reshape(-1)
        if eye.shape != (3,) or not np.isfinite(eye).all():
            raise ValueError(f"query_scene: view must be 'normal' or an eye point of 3 finite numbers, got {view!r}")
    need_grad = want_normal or (want_rgb and eye is None)
    if not torch.is_tensor(x) or x.shape[-1:] != (3,) or not x.is_cuda:
        raise ValueError("query_scene: x must be a CUDA tensor [...,3]")
    dev = x.device
    plans = []
    for k, (model, placement, occ) in enumerate(zip(models, placements, occupancies)):
        plan = field_plan(model)
        if next(model.parameters()).device != dev:
            raise ValueError(f"query_scene: model {k} is not on the points' device {dev}")
        if placement is not None and not isinstance(placement, Placement):
            raise ValueError(f"query_scene: placements[{k}] must be a focnerf_amd.Placement or None")
        if getattr(model, "bg_radius", 0) > 0:
            raise ValueError(f"query_scene: model {k} has a background model (bg_radius > 0); a point query has no ray to ask it about")
        if want_rgb and not plan.infer:
            raise ValueError(f"query_scene: rgb needs a network the fused inference serves (field_plan(model).infer), model {k} is not one")
        if need_grad and not plan.normals:
            raise ValueError(f"query_scene: normals and view='normal' need a network the fused normals kernel serves (field_plan(model).normals), "
                             f"model {k} is not one")
        if not (plan.normals or plan.infer):
            raise ValueError(f"query_scene: model {k} is served by neither fused kernel (field_plan(model).normals or .infer)")
        if occ is not None:
            if not isinstance(occ, Occupancy):
                raise ValueError("query_scene: occupancies hold focnerf_amd.fixedcull.Occupancy objects or None")
            if occ.bound != float(model.bound):
                raise ValueError(f"query_scene: the occupancy grid of model {k} covers bound {occ.bound}, the model bound {float(model.bound)}")
        plans.append(plan)

    prefix = list(x.shape[:-1])
    flat = x.detach().reshape(-1, 3).float().contiguous()
    n, chunk = flat.shape[0], min(max(int(chunk), 1), MAX_POINTS)
    sigma = torch.zeros(n, dtype=torch.float32, device=dev)
    ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rgb = torch.zeros(n, 3, dtype=torch.float32, device=dev) if want_rgb else None
    normal = torch.zeros(n, 3, dtype=torch.float32, device=dev) if want_normal else None
    for k, (model, placement, occ, plan) in enumerate(zip(models, placements, occupancies, plans)):
        P = Placement() if placement is None else placement
        w2o = _host_floats(P.world_to_object(), 12, "query_scene: placement.world_to_object()")
        box = _host_floats(model.aabb_infer, 6, "query_scene: model.aabb_infer")
        rot9 = None if placement is None else _host_floats(np.asarray(P.rotation, dtype=np.float64).astype(np.float32).reshape(-1), 9, "query_scene: rotation")
        eye_obj = None if eye is None else _eye_in_object(eye, P)
        obj_feat = model.encode_object_feature(yolo_details[k], dev) if (want_rgb and plan.uses_object_feature) else None
        bound = float(model.bound)
        for first in range(0, n, chunk):
            count = min(chunk, n - first)
            mask, offsets, n_out = points_cull(flat, first, count, w2o, box, occ)
            m_occ = int(n_out.item())                                    # the host read: sizes the compact arrays
            if m_occ == 0:
                continue
            pos_c, xn_c = points_cull_emit(flat, first, count, mask, offsets, m_occ, bound, w2o, want_pos=want_rgb and eye is not None)
            sigma_c = grad_c = rgb_c = normal_c = dirs_c = None
            if need_grad:
                sigma_c, grad_c, _, _ = normals_launch(model, xn_c, None, want_sigma=True, want_grad=True)
            if need_grad or want_rgb:
                dirs_c, normal_c = surface_frame(grad_c, pos_c, rot9, eye_obj, want_dirs=want_rgb, want_normal=want_normal)
            if want_rgb:
                s2, rgb_c = field_infer(model, xn_c, dirs_c, dir_div=1, obj_feat=obj_feat)
                sigma_c = s2 if sigma_c is None else sigma_c             # the same bits (include/focnerf.h, foc_field_normals)
            if sigma_c is None:                                          # neither colour nor normal: the density alone
                sigma_c = normals_launch(model, xn_c, None, want_sigma=True)[0] if plan.normals else _sigma_only(model, xn_c, plan)
            scene_select(sigma_c, rgb_c, normal_c, mask, offsets, P.sigma_gain, k, sigma, ids, rgb, normal, first, count)
    return SceneSample(sigma.view(prefix), ids.view(prefix), None if rgb is None else rgb.view(prefix + [3]),
                       None if normal is None else normal.view(prefix + [3]))


def _sigma_only(model, xn_c, plan):
    """sigma of a network the normals kernel does not serve, for want=(): the whole-field inference with a constant direction."""
    from .field import field_infer
    dirs = torch.zeros_like(xn_c)
    dirs[:, 2] = -1.0
    obj = torch.zeros(16, device=xn_c.device) if plan.uses_object_feature else None
    return field_infer(model, xn_c, dirs, dir_div=1, obj_feat=obj)[0]
