"""Hash-grid encoder -> fused MLP as ONE autograd node, with the encoding kept in the encoder's native layout.

The reference's encoder kernels work on [L, B, C] (gridencoder.cu:218, :283) and its Python wrapper permutes + copies to
[B, L*C] for the MLP and back for the gradient (grid.py:57, :75). `grid_encode` here avoids the copies by letting the
encoder kernels address [B, L*C] directly, but a level-major launch that keeps one level's table in one XCD's L2 wants to
write [L, B, C] planes (0.59 vs 0.74 ms per 2 M points on MI355X). This node keeps the planes and lets the MLP kernels read /
write them (`foc_ffmlp_forward_planar`, `foc_ffmlp_backward_planar`), so neither side pays for the other's layout:

    h = hashgrid_mlp(encoder, mlp, x)        # == mlp.forward_padded(encoder(x, bound))   (same values, same gradients)

Used by NeRFNetwork (fused head) and render_fixed_steps; FOC_FUSED_FIELD=0 restores the two separate nodes.

`field_plan(model)` decides, per call, which fused kernels serve a network — this node, the fixed-step tail, the whole-field inference
kernel, the occupancy-grid training node, the native occupancy render loop, the head kernels — and carries the shapes they take.
"""
import os
from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd import Function
from torch.amp import custom_bwd, custom_fwd

from .backend import _gridencoder, _ffmlp
from .ffmlp import FFMLP, PackedMLP, single_pass_backward
from .gridencoder import GridEncoder, GridSpec


def fused_mlp(model, name):
    """What the fused kernels read as `model.<name>` ('sigma_net', 'color_net', 'bg_net'): the FFMLP itself, or — for a network whose
    layers are bias-free nn.Linear modules (network_linear.py, `model.fused_mlp`) — its ffmlp.PackedMLP, whose `weights` is the packed
    blob. None when the model has no such network."""
    get = getattr(model, "fused_mlp", None)
    return get(name) if get is not None else getattr(model, name, None)


@dataclass(frozen=True)
class MlpShape:
    """What the MLP kernels take besides the tensors: an FFMLP's shape (its blob layout, ffmlp.py)."""
    input_dim: int
    hidden_dim: int
    num_layers: int
    activation: int
    output_activation: int
    padded_output_dim: int

    @staticmethod
    def of(mlp):
        if not isinstance(mlp, (FFMLP, PackedMLP)):
            return None
        return MlpShape(mlp.input_dim, mlp.hidden_dim, mlp.num_layers, mlp.activation, mlp.output_activation, mlp.padded_output_dim)

    def blob_numel(self):
        return self.hidden_dim * (self.input_dim + self.hidden_dim * (self.num_layers - 1) + self.padded_output_dim)


@dataclass(frozen=True)
class FieldPlan:
    """Which fused kernels serve a network, and the shapes they take. Built per call by `field_plan` (the switches are live); the
    per-call conditions (GPU tensors, autocast, autograd, training) stay with the callers."""
    grid: Optional[GridSpec]            # the hash grid's GridSpec (None: the encoder is no GridEncoder)
    levels: int
    sigma: Optional[MlpShape]           # None: not an FFMLP
    colour: Optional[MlpShape]
    uses_object_feature: bool           # FOC's network: a 16-wide encoded object feature in the colour input (48 wide)
    field: bool                         # hash grid -> sigma network as one node (_hashgrid_mlp)
    train_forward: bool                 # the fixed-step training forward of both networks in one kernel (foc_field_forward_train)
    tail: bool                          # density head -> colour network -> composite as one node (fixedstep._render_tail)
    infer: bool                         # the whole field without autograd in one kernel after the encoder (field_infer)
    occ: bool                           # the occupancy-grid training forward as one node (occtrain._occ_train)
    native_loop: bool                   # the occupancy-grid inference loop as one call per iteration (NeRFRenderer._native_inference_loop)
    head: bool                          # the glue between the two networks as kernels (head.sample_head / rgb_head)
    colour_input_pad: float = 0.0       # the colour input's last column: 47 of the 48-wide object-conditioned row (1.0: tinycudann layout,
                                        # network_tcnn.py), 31 of the 32-wide row (1.0: legacy tinycudann layout, network_tcnn_legacy.py)
    background: bool = False            # the background model (encoder_bg -> bg_net) as one kernel each way (background.py, csrc/background.hip)
    occ_object: bool = False            # `occ` for an object-conditioned network: the node with the encoded object feature (occtrain._occ_train with the feature)
    native_loop_object: bool = False    # `native_loop` for an object-conditioned network: the step takes the feature (and the column-47 pad twin)
    normals: bool = False               # sigma, the density logit's position gradient and the encoded normal in one kernel (normals.field_normals)


def pad_twin(name, pad, obj):
    """(entry point, extra arguments) for the library call `name` with the colour input's pad: `name` itself for pad 0 (the old call,
    unchanged), else its twin that takes the pad before the stream — `name`_pad for the 48-wide object-conditioned row (column 47),
    `name`_pad31 for the 32-wide row (column 31)."""
    from ._lib import lib
    if pad == 0:
        return getattr(lib, name), ()
    return getattr(lib, name + ("_pad" if obj else "_pad31")), (float(pad),)


def object_feature_half(obj_feat, who):
    """The ENCODED object feature as the kernels read it: a detached, contiguous fp16 [16] (None for None: a network without one)."""
    if obj_feat is None:
        return None
    obj16 = obj_feat.detach().reshape(-1).half().contiguous()
    if obj16.numel() != 16:
        raise RuntimeError(f"{who}: the encoded object feature has {obj16.numel()} elements, the colour head takes 16")
    return obj16


def _on(switch):
    return os.environ.get(switch, "1") != "0"


def field_plan(model):
    """The FieldPlan of `model` (a network of network.py / network_foc.py, or anything with some of their attributes) under the current
    switches. Every shape rule of the fused kernels is stated once here; each verdict is a conjunction of these facts and its switch."""
    from ._lib import get_option
    from .shencoder import SHEncoder
    enc, enc_dir = getattr(model, "encoder", None), getattr(model, "encoder_dir", None)
    sigma, colour = MlpShape.of(fused_mlp(model, "sigma_net")), MlpShape.of(fused_mlp(model, "color_net"))
    obj = bool(getattr(model, "uses_object_feature", False))
    pad = float(getattr(model, "colour_input_pad", 0.0))     # the *_pad / *_pad31 kernels take it; sample_head writes a zero there
    grid = enc.spec() if isinstance(enc, GridEncoder) else None

    # the hash grid the [L,B,C] kernels read: D 3, C 2, feeding the sigma network directly; the native loop's encoder is the plain one
    hash_grid = grid is not None and enc.input_dim == 3 and enc.level_dim == 2 and sigma is not None and sigma.input_dim == enc.output_dim
    plain_grid = grid is not None and grid.gridtype == 0 and not grid.align_corners and grid.interpolation == 0
    # sigma network: the single-pass backward serves it (FOC_MLP_BWD_FUSED), a 16-wide output (sigma + 15 geometry features)
    sigma_one_pass = sigma is not None and single_pass_backward(sigma.input_dim, sigma.hidden_dim, sigma.num_layers, sigma.activation)
    sigma_16 = sigma is not None and sigma.padded_output_dim == 16
    sigma_32_64 = sigma is not None and sigma.input_dim == 32 and sigma.hidden_dim == 64
    # colour network: fed [SH16 | geo 15 | (object feature 16) | 0], 64 wide, a 16-wide output
    colour_in = 48 if obj else 32
    colour_64 = colour is not None and colour.input_dim == colour_in and colour.hidden_dim == 64 and colour.padded_output_dim == 16
    colour_rows = (isinstance(enc_dir, SHEncoder) and enc_dir.degree == 4 and getattr(model, "geo_feat_dim", 0) == 15
                   and (not obj or getattr(model, "yolo_encoding_dim", 0) == 16))
    colour_relu_or_none = colour is not None and colour.activation in (0, 6)
    both = sigma is not None and colour is not None
    same_activation = both and sigma.activation == colour.activation
    layer_pair = both and (sigma.num_layers, colour.num_layers) in ((1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
    whole_field = sigma_32_64 and colour_64 and colour_rows and layer_pair and same_activation   # both networks in one kernel

    field = hash_grid and sigma_one_pass and sigma_16 and _on("FOC_FUSED_FIELD")
    tail = colour_64 and colour.num_layers in (2, 3) and colour_relu_or_none and colour_rows and _on("FOC_FUSED_TAIL")
    infer = field and whole_field and (not obj or sigma.activation == 0) and _on("FOC_FUSED_INFER")
    # the background model csrc/background.hip computes: a plain 4-level hash grid over D 2 with C 2, then [SH16(d) | grid 8 | 0] -> 64 ->
    # ReLU -> 3 without biases (legacy/nerf/network.py:71-92, 145-160)
    enc_bg, bg_mlp = getattr(model, "encoder_bg", None), fused_mlp(model, "bg_net")
    bg_grid = enc_bg.spec() if isinstance(enc_bg, GridEncoder) else None
    background = (bg_grid is not None and enc_bg.input_dim == 2 and enc_bg.level_dim == 2 and enc_bg.offsets.numel() == 5
                  and bg_grid.gridtype == 0 and not bg_grid.align_corners and bg_grid.interpolation == 0
                  and isinstance(bg_mlp, PackedMLP) and bg_mlp.in_features == 24 and MlpShape.of(bg_mlp) == MlpShape(32, 64, 1, 0, 6, 16)
                  and bg_mlp.output_dim == 3 and isinstance(enc_dir, SHEncoder) and enc_dir.degree == 4 and _on("FOC_FUSED_BG"))
    bg_radius = getattr(model, "bg_radius", 0)
    occ_common = field and tail and same_activation and _on("FOC_FUSED_OCC")
    native_common = infer and getattr(model, "density_scale", 1) == 1 and plain_grid and _on("FOC_RENDER_NATIVE")
    # csrc/normals.hip: the plain hash grid with 16 levels, the 32 -> 64 x (1..3) -> 16 ReLU sigma network whose column 0 is the density logit
    normals = (hash_grid and plain_grid and enc.offsets.numel() == 17 and sigma_32_64 and sigma_16 and sigma.activation == 0
               and 1 <= sigma.num_layers <= 3 and _on("FOC_FUSED_NORMALS"))
    return FieldPlan(
        grid=grid, levels=enc.offsets.numel() - 1 if grid is not None else 0, sigma=sigma, colour=colour, uses_object_feature=obj,
        field=field, tail=tail, infer=infer,
        train_forward=(field and tail and whole_field and sigma.output_activation == 6 and get_option("FOC_FIELD_FWD_FUSED") != 0),
        occ=occ_common and not obj and (bg_radius <= 0 or background),
        native_loop=native_common and not obj,
        head=both and colour.input_dim == colour_in and colour_rows and pad == 0 and _on("FOC_FUSED_HEAD"), colour_input_pad=pad,
        background=background,
        # an object-conditioned network: the object node sequences the whole-field kernels (their layer pairs), and no background model
        occ_object=occ_common and obj and whole_field and bg_radius <= 0,
        native_loop_object=native_common and obj and bg_radius <= 0,
        normals=normals)


def _raw_stream_of(device):
    """Handle of torch's current stream on `device` (an int: cheap to take and to compare)."""
    from ._lib import raw_stream
    return raw_stream(device.index if device.index is not None else torch.cuda.current_device())


_half_scope = None          # dict id(param) -> (param, fp16 copy) while a `half_cache_scope()` is open, else None


class half_cache_scope:
    """Within the scope the fp16 copies of parameters are made once and reused: a staged render evaluates the same 50 MB table and the
    same weight blobs for each of its 157 ray chunks, under `no_grad`, with nothing writing the parameters in between. The scope is the
    ONLY cache: outside it every forward converts again, as the reference does on every call (grid.py:41-44; ffmlp.py:23) — validity
    cannot be inferred from the parameter itself, because writes through `.data` (torch_ema's copy_to / restore around every
    evaluation, nerf/utils.py:1164-1174; `reset_parameters`) leave its version counter untouched. Re-entrant; the outermost exit drops
    the copies, and so does `drop_half_cache()` (ParameterEMA.copy_to / restore call it) while the scope stays open."""

    def __enter__(self):
        global _half_scope
        self._outer = _half_scope
        if _half_scope is None:
            _half_scope = {}
        return self

    def __exit__(self, *exc):
        global _half_scope
        _half_scope = self._outer
        return False


def drop_half_cache():
    """Forget what an open `half_cache_scope` holds: somebody has written the parameters in place (ParameterEMA.copy_to / restore), which
    neither their identity nor their version counter shows. The scope stays open and fills again. No scope open: nothing to do."""
    if _half_scope is not None:
        _half_scope.clear()


def _half_of(param):
    """fp16 copy of a parameter: a fresh conversion, unless a `half_cache_scope` is open (then one conversion per scope)."""
    if param.dtype == torch.half:
        return param.contiguous()
    if _half_scope is None:
        return param.detach().to(torch.half).contiguous()
    hit = _half_scope.get(id(param))
    if hit is not None and hit[0] is param and hit[1].device == param.device:
        if hit[2] is not None and _raw_stream_of(param.device) != hit[3]:
            torch.cuda.current_stream(param.device).wait_event(hit[2])      # made on another stream (staged render: chunks alternate streams)
        return hit[1]
    h = param.detach().to(torch.half).contiguous()
    ev = st = None
    if h.is_cuda:
        st = _raw_stream_of(h.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(h.device))         # the stream of the TENSOR's device: it need not be the current device
    _half_scope[id(param)] = (param, h, ev, st)
    return h


def scope_cached(key, owner, make):
    """`make()` -> tensor, once per open `half_cache_scope` for (key, owner) — `owner` is kept and compared by identity so that a recycled
    id() cannot alias. Like `_half_of`, a value made on one stream is handed to another stream behind an event. No scope: `make()`."""
    if _half_scope is None:
        return make()
    hit = _half_scope.get(key)
    if hit is not None and hit[0] is owner:
        if hit[2] is not None and _raw_stream_of(hit[1].device) != hit[3]:
            torch.cuda.current_stream(hit[1].device).wait_event(hit[2])
        return hit[1]
    v = make()
    ev = st = None
    if v.is_cuda:
        st = _raw_stream_of(v.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(v.device))
    _half_scope[key] = (owner, v, ev, st)
    return v


def _check_colour_branch(colour, B):
    """The colour branch of `_hashgrid_mlp`, checked before its first launch: foc_field_forward_train trusts these sizes."""
    cweights, shape, ray_sh, T, c_width, obj_feat = colour[:6]
    T = int(T)
    if not (ray_sh.dtype == torch.half and ray_sh.dim() == 2 and ray_sh.shape[1] == 16 and ray_sh.is_contiguous() and T > 0
            and B == ray_sh.shape[0] * T):
        raise RuntimeError(f"hashgrid_mlp colour branch: ray_sh must be a contiguous half [B / T, 16] tensor with B = {B}, T = {T}; got "
                           f"{tuple(ray_sh.shape)} {ray_sh.dtype}{'' if ray_sh.is_contiguous() else ' (strided)'}")
    if c_width not in (4, 16):
        raise RuntimeError(f"hashgrid_mlp colour branch: c_width must be 4 or 16, got {c_width}")
    if shape.input_dim not in (32, 48) or (obj_feat is not None) != (shape.input_dim == 48) or (obj_feat is not None and obj_feat.numel() != 16):
        raise RuntimeError(f"hashgrid_mlp colour branch: a {shape.input_dim}-wide colour input takes "
                           f"{'a 16-element object feature' if shape.input_dim == 48 else 'no object feature'}, got "
                           f"{'none' if obj_feat is None else f'{obj_feat.numel()} elements'}")
    if cweights.numel() != 64 * (shape.input_dim + 64 * (shape.num_layers - 1) + 16):
        raise RuntimeError(f"hashgrid_mlp colour branch: the colour weights hold {cweights.numel()} elements, a {shape.input_dim}-wide "
                           f"{shape.num_layers}-layer network has {64 * (shape.input_dim + 64 * (shape.num_layers - 1) + 16)}")


class _hashgrid_mlp(Function):
    @staticmethod
    @custom_fwd(device_type="cuda")
    def forward(ctx, x, embeddings, weights, offsets, grid, sigma, training, colour=None):
        # x [B,3] fp32 in [0,1]; embeddings [rows,2]; weights: FFMLP blob; grid: GridSpec; sigma: MlpShape of the blob
        # colour = (colour weights, colour MlpShape, ray_sh [B / T, 16] half, T, c_width, obj_feat or None[, input pad = the last column of
        # the colour input (47 of the 48-wide row, 31 of the 32-wide one), 0 when absent]): the colour network's forward runs in
        # the SAME kernel as the sigma network's (foc_field_forward_train) and its logits come back as a second, non-differentiable output — the
        # node that owns the colour network (fixedstep._render_tail) takes them instead of launching foc_color_head_forward, and computes every
        # gradient of the colour network in its own backward as before
        x = x.contiguous().float()
        B = x.shape[0]
        if colour is not None:
            _check_colour_branch(colour, B)
        S, H, (gridtype, align_corners, interp) = grid.log2_scale, grid.base_resolution, grid.tail()
        L = offsets.shape[0] - 1
        emb = _half_of(embeddings)                              # grid.py:41-44: half table under autocast (C even)
        w = _half_of(weights)                                   # ffmlp.py:23: custom_fwd(cast_inputs=half)
        enc = torch.empty(L, B, 2, device=x.device, dtype=torch.half)
        # training: the backward's count pass rides along in the forward launch (backend.grid_encode_forward_counted)
        ticket = _gridencoder.grid_encode_forward_counted(x, emb, offsets, enc, B, 3, 2, L, S, H, gridtype, align_corners, interp,
                                                          standalone=_gridencoder.precount_standalone()) if training else None
        if ticket is None:
            _gridencoder.grid_encode_forward(x, emb, offsets, enc, B, 3, 2, L, S, H, None, gridtype, align_corners, interp)
        h = torch.empty(B, 16, device=x.device, dtype=torch.half)
        c = None
        if colour is not None:
            from ._lib import ptr, stream_of, check
            cweights, cshape, ray_sh, T, c_width, obj_feat = colour[:6]
            pad = float(colour[6]) if len(colour) > 6 else 0.0
            wc = _half_of(cweights)
            obj16 = object_feature_half(obj_feat, "hashgrid_mlp colour branch")
            c = torch.empty(B, c_width, device=x.device, dtype=torch.half)
            args = (ptr(enc), ptr(w), sigma.num_layers, ptr(ray_sh), int(T), ptr(wc), int(cshape.num_layers), 64, int(sigma.activation), B, ptr(h),
                    ptr(c), int(c_width), ptr(obj16))
            fn, extra = pad_twin("foc_field_forward_train", pad, obj16 is not None)
            check(fn(*args, *extra, stream_of(enc)), "field_forward_train")
        else:
            _ffmlp.ffmlp_forward_planar(enc, w, B, sigma.input_dim, 16, sigma.hidden_dim, sigma.num_layers, sigma.activation, sigma.output_activation, h)
        if training:
            ctx.save_for_backward(x, emb, w, offsets, enc)
            ctx.cfg = (grid, sigma, B, L)
            ctx.ticket = ticket
        if c is None:
            return h
        ctx.mark_non_differentiable(c)
        ctx.set_materialize_grads(False)          # c's "gradient" arrives as None instead of a zero-filled [B, c_width] tensor (6 us per step)
        return h, c

    @staticmethod
    @custom_bwd(device_type="cuda")
    def backward(ctx, grad_h, _grad_c=None):
        x, emb, w, offsets, enc = ctx.saved_tensors
        grid, sigma, B, L = ctx.cfg
        if grad_h is None:                        # (set_materialize_grads(False): h took no part in the loss)
            return (None,) * 8
        grad_h = grad_h.contiguous().half()
        g_enc = torch.empty_like(enc)                           # [L,B,2]
        g_w = torch.empty_like(w)
        _ffmlp.ffmlp_backward_planar(grad_h, enc, w, B, sigma.input_dim, 16, sigma.hidden_dim, sigma.num_layers, sigma.activation,
                                     sigma.output_activation, True, g_enc, g_w)
        g_emb = torch.zeros_like(emb)
        _gridencoder.grid_encode_backward(g_enc, x, emb, offsets, g_emb, B, 3, 2, L, grid.log2_scale, grid.base_resolution, None, None, *grid.tail(),
                                          grad_bl=False, precount=ctx.ticket)
        return None, g_emb, g_w, None, None, None, None, None


@torch.no_grad()
def field_infer(model, xn, dirs, dir_div=1, dir_block=0, obj_feat=None):
    """xn [M,3] fp32 in [0,1] (already normalised), dirs [M / dir_div, 3] -> sigma [M] fp32, rgb [M,3] fp32 (no autograd).
    dir_block = 64: the rows stand in the block-interleaved order of `fixedstep.fixed_sample(..., ray_block=64)`.
    obj_feat [16]: the encoded object feature of an object-conditioned network (required iff `model.uses_object_feature`)."""
    from ._lib import ptr, stream_of, check
    enc, sn, cn = model.encoder, fused_mlp(model, "sigma_net"), fused_mlp(model, "color_net")
    grid = enc.spec()
    xn = xn.contiguous().float()
    dirs = dirs.contiguous().float()
    M = xn.shape[0]
    L = enc.offsets.shape[0] - 1
    emb, ws, wc = _half_of(enc.embeddings), _half_of(sn.weights), _half_of(cn.weights)
    planes = torch.empty(L, M, 2, device=xn.device, dtype=torch.half)
    _gridencoder.grid_encode_forward(xn, emb, enc.offsets, planes, M, 3, 2, L, grid.log2_scale, grid.base_resolution, None, *grid.tail())
    sigma = torch.empty(M, dtype=torch.float32, device=xn.device)
    rgb = torch.empty(M, 3, dtype=torch.float32, device=xn.device)
    obj16 = None
    if getattr(model, "uses_object_feature", False):
        if obj_feat is None:
            raise RuntimeError("field_infer: an object-conditioned network needs its encoded object feature")
        obj16 = object_feature_half(obj_feat, "field_infer")
    args = (ptr(planes), 1, ptr(dirs), int(dir_div), int(dir_block), dirs.shape[0], ptr(ws), sn.num_layers, ptr(wc), cn.num_layers, 64, sn.activation, M,
            ptr(sigma), ptr(rgb), ptr(obj16))
    # the tinycudann layouts (network_tcnn.py, network_tcnn_legacy.py): the last column of the colour input is a constant
    fn, extra = pad_twin("foc_nerf_field_inference", float(getattr(model, "colour_input_pad", 0.0)), obj16 is not None)
    check(fn(*args, *extra, stream_of(xn)), "nerf_field_inference")
    return sigma, rgb


def hashgrid_mlp(encoder, mlp, x, bound=1, colour=None):
    """x [...,3] in [-bound, bound] (bound None: already in [0,1]) -> [..., 16] half: mlp.forward_padded(encoder(x, bound)).
    colour: the colour branch of `_hashgrid_mlp` (the fixed-step training forward) -> (h [B,16], colour logits [B, c_width])."""
    prefix = list(x.shape[:-1])
    xn = (x if bound is None else (x + bound) / (2 * bound)).view(-1, 3)
    h = _hashgrid_mlp.apply(xn, encoder.embeddings, mlp.weights, encoder.offsets, encoder.spec(), MlpShape.of(mlp), mlp.training and torch.is_grad_enabled(),
                            colour)
    if colour is not None:
        h, c = h
        return h.view(prefix + [16]), c
    return h.view(prefix + [16])
