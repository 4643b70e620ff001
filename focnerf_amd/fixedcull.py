"""Occupancy-culled fixed-step fields for the multi-object combiner (csrc/fixedcull.hip).

The combiner's per-sample select (COMBINED.py `best_densities_and_colors_v3`) needs every object at the same T positions of the same
rays, so an object cannot march ragged samples of its own. With an `Occupancy`, `fixedstep.render_field4` keeps the fixed positions,
tests each against the object's occupancy bitfield and evaluates encoder + networks on the occupied ones only; every other sample
has sigma = 0. That is the approximation `run_cuda` makes: densities below the grid's threshold are dropped, the transmittance behind
such samples is slightly higher, and a sample whose own weight stood at the 1e-10 mask threshold can change sides.

    occ = Occupancy.of(model)            # a cuda_ray network: its trained density_bitfield, no copy
    occ = Occupancy.estimate(model)      # any network with density(x): the full-grid passes of update_extra_state on own buffers
    render_field4(model, rays_o, rays_d, num_steps=T, out=buf, occupancy=occ)
    render_field4(model, rays_o, rays_d, num_steps=T, out=buf, occupancy=occ, placement=P, scene_aabb=box)     # placement.py

`culled_lists` is the same sequence without its last step, the pack into a dense field4: it returns the compact lists as a `CulledField`,
which `combine.combine_culled` selects and composites from directly.
"""
import torch

from ._lib import lib, ptr, stream_of, check
from .backend import _scratch


class Occupancy:
    """An object's occupancy bitfield with the grid it describes: uint8 [cascade * grid_size^3 / 8] in Morton order (what
    `raymarching.packbits` writes), cascades of a box of half-width `bound`."""

    def __init__(self, bitfield, cascade, grid_size, bound):
        cascade, grid_size = int(cascade), int(grid_size)
        if not torch.is_tensor(bitfield) or bitfield.dtype != torch.uint8:
            raise ValueError("Occupancy: the bitfield must be a uint8 tensor")
        if cascade < 1 or grid_size < 2 or grid_size & (grid_size - 1):
            raise ValueError(f"Occupancy: cascade {cascade} / grid_size {grid_size}: need cascade >= 1 and a power-of-two grid_size")
        if bitfield.numel() != cascade * grid_size ** 3 // 8:
            raise ValueError(f"Occupancy: a bitfield of {bitfield.numel()} bytes does not describe {cascade} cascades of {grid_size}^3 cells")
        self.bitfield, self.cascade, self.grid_size, self.bound = bitfield.contiguous().view(-1), cascade, grid_size, float(bound)

    @classmethod
    def of(cls, model):
        """The trained grid of a `cuda_ray=True` network: its `density_bitfield`, `cascade`, `grid_size` and `bound`, without a copy (a
        later `update_extra_state` shows through). An all-zero bitfield — a grid that was never trained or installed — is refused: it
        would render nothing, silently."""
        bits = getattr(model, "density_bitfield", None)
        if not getattr(model, "cuda_ray", False) or bits is None:
            raise ValueError("Occupancy.of: the model has no occupancy grid (cuda_ray=False); use Occupancy.estimate(model)")
        if not bool(bits.any()):
            raise ValueError("Occupancy.of: the model's density_bitfield is all zero (an untrained grid would render nothing)")
        return cls(bits, model.cascade, model.grid_size, model.bound)

    @classmethod
    @torch.no_grad()
    def estimate(cls, model, passes=16, decay=0.95, density_thresh=None, jitter=True, generator=None):
        """A grid for any network with `density(x)` — FOC's default training is fixed-step, so most per-object checkpoints carry none.
        Runs `passes` full-grid passes of `update_extra_state` (densitygrid.grid_cells_xyz -> model.density -> grid_update_apply: the
        grid keeps max(old * decay, new), cells above min(mean, density_thresh or model.density_thresh) are occupied) on buffers of
        its own, under fp16 autocast like the trainer's call; it neither needs nor touches the model's cuda_ray state. jitter=False
        samples the cell centres (deterministic); `generator` (on the model's device) seeds the jitter."""
        from . import densitygrid
        dev = next(model.parameters()).device
        C, H = int(model.cascade), int(model.grid_size)
        thresh = float(model.density_thresh if density_thresh is None else density_thresh)
        grid = torch.zeros(C, H ** 3, dtype=torch.float32, device=dev)
        bits = torch.zeros(C * H ** 3 // 8, dtype=torch.uint8, device=dev)
        for _ in range(int(passes)):
            noise = torch.rand(C * H ** 3, 3, device=dev, generator=generator) if jitter else None
            at = densitygrid.grid_cells_xyz(C, H, model.bound, noise, dev)
            with torch.autocast("cuda", dtype=torch.float16, enabled=dev.type == "cuda"):      # as the trainer calls update_extra_state (--fp16)
                sigmas = model.density(at)['sigma'].reshape(-1).detach()
            densitygrid.grid_update_apply(grid, C, H, sigmas, None, model.density_scale, decay, thresh, bits)
        return cls(bits, C, H, model.bound)

    @torch.no_grad()
    def pruned(self, keep_largest=1, min_cells=None):
        """A new `Occupancy` without the grid's floaters: per cascade the bits are unpacked, brought out of Morton order to a 0/1 volume
        [H,H,H] (`raymarching.morton3D_invert`), filtered by `components.filter_components` at threshold 0.5 — the `keep_largest`
        largest 26-connected components and / or those of at least `min_cells` cells stay — and packed into a bitfield of its own.
        Cascades are independent (each holds the whole object at its own resolution; components are never joined across them). Culled
        renders of the result keep a subset of this grid's samples. `self` is not modified."""
        from . import raymarching
        from .components import filter_components
        C, H, dev = self.cascade, self.grid_size, self.bitfield.device
        shifts = torch.arange(8, dtype=torch.int32, device=dev)
        cells = ((self.bitfield.int().view(-1, 1) >> shifts) & 1).view(C, H ** 3)               # Morton order, cell index & 7 = the bit
        xyz = raymarching.morton3D_invert(torch.arange(H ** 3, dtype=torch.int32, device=dev)).long()
        lin = (xyz[:, 0] * H + xyz[:, 1]) * H + xyz[:, 2]
        out = torch.empty_like(cells)
        for c in range(C):
            vol = torch.empty(H ** 3, dtype=torch.float32, device=dev)
            vol[lin] = cells[c].float()
            out[c] = (filter_components(vol.view(H, H, H), 0.5, keep_largest, min_cells).view(-1)[lin] >= 0.5).int()
        bits = (out.view(-1, 8) << shifts).sum(-1, dtype=torch.int32).to(torch.uint8)
        return Occupancy(bits, C, H, self.bound)


def _host_floats(values, n, what):
    """`n` floats for a kernel argument block (ctypes array). A tensor is read on the host ONCE and remembered on the tensor object (a
    model's box never changes; an in-place write shows in `_version` and reads it again) — no synchronisation per call."""
    import ctypes
    if torch.is_tensor(values):
        kept = getattr(values, "_foc_host_floats", None)
        if kept is None or kept[0] != values._version:
            kept = (values._version, [float(v) for v in values.detach().reshape(-1).tolist()])
            values._foc_host_floats = kept
        values = kept[1]
    values = [float(v) for v in values]
    if len(values) != n:
        raise ValueError(f"{what}: {n} values expected, got {len(values)}")
    return (ctypes.c_float * n)(*values)


def fixed_cull(rays_o, rays_d, nears, fars, aabb, T, occ, placement=None, obj_aabb=None):
    """The cull pass for N rays x T fixed steps: -> (mask uint64-as-int64 [R], offsets uint32-as-int32 [R + 1], count int32 [1]) with
    R = ceil(N/64) * T rows of the block-interleaved order (include/focnerf.h). No host synchronisation.
    placement (a `Placement`, default None = the unplaced entry point): `aabb` is then the SCENE's box (the samples are the view's
    against it), each sample is mapped into the object's frame and tested against `obj_aabb` (6 floats or a tensor: the object's own
    box, lo then hi; default the cube of the grid's bound) before its cell is looked up (foc_fixed_cull_placed)."""
    N, dev = rays_o.shape[0], rays_o.device
    R = -(-N // 64) * T
    mask = torch.empty(R, dtype=torch.int64, device=dev)
    offsets = torch.empty(R + 1, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = lib.foc_fixed_cull_scratch_bytes(N, T)
    scratch = _scratch.get("fixed_cull", nbytes, dev)
    if placement is not None:
        w2o = _host_floats(placement.world_to_object(), 12, "fixed_cull: placement.world_to_object()")
        box = _host_floats([-occ.bound] * 3 + [occ.bound] * 3 if obj_aabb is None else obj_aabb, 6, "fixed_cull: obj_aabb")
        check(lib.foc_fixed_cull_placed(ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(aabb), N, T, w2o, box, occ.bound, ptr(occ.bitfield),
                                        occ.cascade, occ.grid_size, ptr(mask), ptr(offsets), ptr(count), ptr(scratch), nbytes, stream_of(rays_o)),
              "fixed_cull_placed")
        return mask, offsets, count
    if obj_aabb is not None:
        raise ValueError("fixed_cull: obj_aabb belongs to a placement; without one the samples are tested in the box they were clamped to")
    check(lib.foc_fixed_cull(ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(aabb), N, T, occ.bound, ptr(occ.bitfield), occ.cascade, occ.grid_size,
                             ptr(mask), ptr(offsets), ptr(count), ptr(scratch), nbytes, stream_of(rays_o)), "fixed_cull")
    return mask, offsets, count


def fixed_cull_emit(rays_o, rays_d, nears, fars, aabb, T, bound, mask, offsets, m_occ, placement=None):
    """-> enc_in_c [m_occ,3] (normalised positions of the occupied samples), dirs_c [m_occ,3] (their rays' directions). With a
    placement: the positions in the object's frame and the turned directions (foc_fixed_cull_emit_placed)."""
    N, dev = rays_o.shape[0], rays_o.device
    enc_in_c = torch.empty(m_occ, 3, dtype=torch.float32, device=dev)
    dirs_c = torch.empty(m_occ, 3, dtype=torch.float32, device=dev)
    if placement is not None:
        w2o = _host_floats(placement.world_to_object(), 12, "fixed_cull_emit: placement.world_to_object()")
        check(lib.foc_fixed_cull_emit_placed(ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(aabb), N, T, w2o, float(placement.dir_scale), float(bound),
                                             ptr(mask), ptr(offsets), m_occ, ptr(enc_in_c), ptr(dirs_c), stream_of(rays_o)), "fixed_cull_emit_placed")
        return enc_in_c, dirs_c
    check(lib.foc_fixed_cull_emit(ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(aabb), N, T, float(bound), ptr(mask), ptr(offsets), m_occ,
                                  ptr(enc_in_c), ptr(dirs_c), stream_of(rays_o)), "fixed_cull_emit")
    return enc_in_c, dirs_c


def _check_culled(model, plan, occ):
    if not isinstance(occ, Occupancy):
        raise ValueError("render_field4: occupancy must be a focnerf_amd.fixedcull.Occupancy")
    if not (plan.infer and model.bg_radius <= 0):
        raise ValueError("render_field4: occupancy needs a network the fused inference serves (field_plan(model).infer) without a background "
                         "model; this one would have to render dense")
    if occ.bound != float(model.bound):
        raise ValueError(f"render_field4: the occupancy grid covers bound {occ.bound}, the model bound {float(model.bound)}")


class CulledField:
    """One object on a ray chunk as the cull and the field kernels left it (include/focnerf.h `FocCulledField`): the row masks and offsets of
    `fixed_cull`, the occupied samples' sigma_c [m_occ] / rgb_c [m_occ,3] (None when m_occ == 0) and the pack's arguments. What
    `combine.combine_culled` reads in place of a dense field4; the object keeps its tensors alive."""
    __slots__ = ("mask", "offsets", "m_occ", "sigma_c", "rgb_c", "density_scale", "thresh", "sigma_gain", "N", "T")

    def __init__(self, mask, offsets, m_occ, sigma_c, rgb_c, density_scale, thresh, sigma_gain, N, T):
        self.mask, self.offsets, self.m_occ, self.sigma_c, self.rgb_c = mask, offsets, int(m_occ), sigma_c, rgb_c
        self.density_scale, self.thresh, self.sigma_gain = float(density_scale), float(thresh), float(sigma_gain)
        self.N, self.T = int(N), int(T)


def culled_lists(model, plan, rays_o, rays_d, nears, fars, aabb, T, weight_thresh, yolo_details, occ, placement=None, channels="rgb"):
    """`culled_field4` in front of its pack, for N > 0 rays: cull -> ONE host read of the count -> emit -> encoder + whole-field kernel on
    the occupied samples. -> a `CulledField` (sigma_gain 1 without a placement). channels="normal": rgb_c holds the encoded normals
    0.5 + 0.5 n of `normals.field_normals`, rotated object -> scene by the placement's rotation."""
    from .field import field_infer
    from .normals import check_channels, field_normals
    want_normal = check_channels("render_field4", channels, plan)
    N, dev = rays_o.shape[0], rays_o.device
    if occ.bitfield.device != dev:
        raise ValueError(f"render_field4: the occupancy bitfield is on {occ.bitfield.device}, the rays on {dev}")
    obj_aabb = None if placement is None else (model.aabb_train if model.training else model.aabb_infer)
    mask, offsets, count = fixed_cull(rays_o, rays_d, nears, fars, aabb, T, occ, placement, obj_aabb)
    m_occ = int(count.item())                                   # the host read: sizes the compact arrays and the field launch
    sigma = rgb = None
    if m_occ:
        enc_in_c, dirs_c = fixed_cull_emit(rays_o, rays_d, nears, fars, aabb, T, model.bound, mask, offsets, m_occ, placement)
        obj_feat = model.encode_object_feature(yolo_details, dev) if plan.uses_object_feature else None
        if want_normal:
            sigma, rgb = field_normals(model, enc_in_c, None if placement is None else placement.rotation)
        else:
            sigma, rgb = field_infer(model, enc_in_c, dirs_c, dir_div=1, dir_block=0, obj_feat=obj_feat)
    return CulledField(mask, offsets, m_occ, sigma, rgb, model.density_scale, weight_thresh, 1.0 if placement is None else placement.sigma_gain, N, T)


def culled_field4(model, plan, rays_o, rays_d, nears, fars, aabb, T, weight_thresh, yolo_details, out, occ, placement=None, channels="rgb"):
    """The culled field along GIVEN nears / fars [N] (of the rays against `aabb`): `culled_lists` -> culled pack. With a placement, `aabb`
    is the scene's box, the object's own box is the model's, and the pack applies the placement's sigma gain."""
    N = rays_o.shape[0]
    if N == 0:
        return out
    c = culled_lists(model, plan, rays_o, rays_d, nears, fars, aabb, T, weight_thresh, yolo_details, occ, placement, channels)
    if placement is not None:
        check(lib.foc_fixed_field_pack_culled_gain(ptr(c.sigma_c), ptr(c.rgb_c), ptr(c.mask), ptr(c.offsets), c.m_occ, ptr(nears), ptr(fars), N, T,
                                                   c.density_scale, c.thresh, c.sigma_gain, ptr(out), stream_of(out)), "fixed_field_pack_culled_gain")
        return out
    check(lib.foc_fixed_field_pack_culled(ptr(c.sigma_c), ptr(c.rgb_c), ptr(c.mask), ptr(c.offsets), c.m_occ, ptr(nears), ptr(fars), N, T, c.density_scale,
                                          c.thresh, ptr(out), stream_of(out)), "fixed_field_pack_culled")
    return out


def render_field4_culled(model, plan, rays_o, rays_d, T, weight_thresh, yolo_details, out, occ, channels="rgb"):
    """`render_field4` with an Occupancy (rays_o / rays_d [N,3] fp32 contiguous, out [N,T,4]): near_far -> cull -> ONE host read of the
    count -> encoder + whole-field kernel on the occupied samples -> culled pack."""
    from . import raymarching
    _check_culled(model, plan, occ)
    if rays_o.shape[0] == 0:
        return out
    aabb = model.aabb_train if model.training else model.aabb_infer
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, model.min_near)
    return culled_field4(model, plan, rays_o, rays_d, nears, fars, aabb, T, weight_thresh, yolo_details, out, occ, None, channels)


def _scene_box(scene_aabb, model, dev):
    if scene_aabb is None:
        return model.aabb_train if model.training else model.aabb_infer
    if not torch.is_tensor(scene_aabb) or scene_aabb.dtype != torch.float32 or scene_aabb.numel() != 6:
        raise ValueError("render_field4: scene_aabb must be a float32 tensor of 6 values (lo, then hi)")
    if scene_aabb.device != dev:
        raise ValueError(f"render_field4: scene_aabb is on {scene_aabb.device}, the rays on {dev}")
    return scene_aabb.contiguous().view(-1)


def render_field4_placed(model, plan, rays_o, rays_d, T, weight_thresh, yolo_details, out, occ, placement, scene_aabb=None, channels="rgb"):
    """`render_field4` with an Occupancy and a Placement: near / far of the view's rays against the SCENE's box (default: the model's),
    then the sequence of `render_field4_culled` through the placed entry points."""
    from . import raymarching
    from .placement import Placement
    if not isinstance(placement, Placement):
        raise ValueError("render_field4: placement must be a focnerf_amd.Placement")
    _check_culled(model, plan, occ)
    if rays_o.shape[0] == 0:
        return out
    aabb = _scene_box(scene_aabb, model, rays_o.device)
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, model.min_near)
    return culled_field4(model, plan, rays_o, rays_d, nears, fars, aabb, T, weight_thresh, yolo_details, out, occ, placement, channels)
