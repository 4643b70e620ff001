"""Fused occupancy-grid TRAINING path: what `NeRFRenderer.run_cuda` computes in training mode (legacy/nerf/renderer.py:256-322) for a
`focnerf_amd.network.NeRFNetwork`, as ONE autograd node over the kernels

    march_rays_train (field layout) -> grid_encode (+ the backward's count pass) -> sigma_net -> color_net (head form) -> tail

instead of the caller-side chain  march_rays_train -> (x + bound) / (2 bound) -> grid_encode -> sigma_net -> trunc_exp / SH / cat / pad
-> color_net -> sigmoid -> composite_rays_train -> background / depth normalisation  with an autograd node, a handful of torch kernels
and their Python per stage. Same sample list (bit for bit), same values as that chain (the colour network's input is never materialised:
its first k-chunk is one SH row per sample written by the march's emit pass, its second the density network's output row, csrc/ffmlp.hip
MlpHead; sigma, rgb and their gradients stay on the lane in csrc/occtrain.hip), same gradients up to fp32 summation order.

The step it replaces was bound by its launches: ~85 kernels, 0.9 ms of GPU time, 1.2 ms of host time to enqueue them from Python.
FOC_FUSED_OCC=0 keeps the chain (tests compare the two); `field.field_plan` decides which networks it serves (`plan.occ`, `plan.occ_object`).

ONE node, `_occ_train`, serves the three layouts of the colour input, and its configuration is one record, `OccTrainConfig`:
  * plain (32 wide, last column 0): foc_occ_train_forward / _backward;
  * a constant column 31 (`plan.colour_input_pad`: network_tcnn_legacy.py, 1.0): the *_pad31 entry points, the pad beside the node;
  * object-conditioned (network_foc.py, network_tcnn.py; 48 wide): the *_obj entry points. The encoded object feature is a tensor input
    with a gradient (the colour head returns it), column 47 of the colour input is the plan's pad, and the tail can return the per-ray
    sums of sigma^2 that FOC's outside-mask criterion needs.
Without an object feature the library calls, the buffers and the values are those of the plain node.

`want_dist` (run_cuda(..., distortion=True)): the tail also returns the per-ray distortion of mip-NeRF 360 (foc_occ_tail_forward_dist /
_backward_dist), differentiable. `want_depth_grad` (run_cuda(..., depth_grad=True)): `depth` carries a gradient (the tail also keeps
depth_raw = sum w t, foc_occ_tail_forward_depth / _backward_depth); without it `depth` is marked non-differentiable, as the reference's
composite ignores grad_depth. The buffers of both travel beside the node in a FocOccTrainTail, and with either keyword the one-call route is
foc_occ_train_forward_tail / _backward_tail for every layout; the call-by-call chain calls the tail entry points itself.
"""
import ctypes
import os
from dataclasses import dataclass

import torch
from torch.autograd import Function

from ._lib import lib, ptr, stream_of, check, FocOccTrainNode, FocOccTrainObject, FocOccTrainTail, FOC_F16
from .backend import _gridencoder, _ffmlp, _scratch
from .field import MlpShape, _half_of, fused_mlp, object_feature_half, pad_twin
from .fixedstep import _C_WIDTH, _background
from .gridencoder import GridSpec


def _round_up(count, align):
    return count + (align - count % align) if align > 0 else count            # raymarching.py:190,226


_zero_jitter = {}


def _no_jitter(n, dev):
    """A [n] block of zeros per device, made once (`perturb` off: the march adds 0 * dt to every ray's start)."""
    z = _zero_jitter.get(dev)
    if z is None or z.shape[0] < n:
        z = _zero_jitter[dev] = torch.zeros(max(n, 4096), dtype=torch.float32, device=dev)
    return z[:n]


_mlp_bytes = {}


def _native_plan(offsets, grid, L, M, sigma, colour, colour_in=32):
    """(grid workspace bytes, MLP workspace bytes) when the node can run as ONE library call each way (include/focnerf.h FocOccTrainNode:
    the encoder's counted forward and binned backward must apply, the switches that take other paths must be at their defaults), else None.
    FOC_OCC_NATIVE_NODE=0: always the call-by-call chain below (the tests compare the two). colour_in 48: the object-conditioned head,
    whose workspace starts with a 48-wide blob image."""
    if os.environ.get("FOC_OCC_NATIVE_NODE", "1") == "0" or _gridencoder.precount_standalone():
        return None
    grid_bytes = _gridencoder.binned_workspace_bytes(offsets, M, 3, 2, L, grid.log2_scale, grid.base_resolution, grid.gridtype, FOC_F16,
                                                     count_ahead=True)
    if not grid_bytes:
        return None
    key = (sigma.input_dim, sigma.hidden_dim, sigma.num_layers, colour.num_layers, colour_in)
    mlp_bytes = _mlp_bytes.get(key)
    if mlp_bytes is None:
        mlp_bytes = _mlp_bytes[key] = max(int(lib.foc_ffmlp_backward_workspace_bytes(colour_in, 64, colour.num_layers)),
                                          int(lib.foc_ffmlp_backward_workspace_bytes(sigma.input_dim, sigma.hidden_dim, sigma.num_layers)))
    return int(grid_bytes), mlp_bytes


def _a(t):
    return t.data_ptr() if t is not None else None


def _sample_block(cap, dev):
    """One block for the three sample arrays: enc_in [cap,3] fp32 | deltas [cap,2] fp32 | sh [cap,16] fp16 (every row written by the emit pass);
    sections start on 16-byte boundaries."""
    o1, o2 = -(-3 * cap // 4) * 4, -(-3 * cap // 4) * 4 + -(-2 * cap // 4) * 4
    block = torch.empty(o2 + 8 * cap, dtype=torch.float32, device=dev)
    return block[: 3 * cap].view(cap, 3), block[o1: o1 + 2 * cap].view(cap, 2), block[o2:].view(torch.float16).view(cap, 16)


@dataclass(frozen=True, eq=False)
class OccTrainConfig:
    """What one training forward takes besides its tensors; built in one place, `render_occupancy_train`."""
    bound: float
    cascade: int
    grid_size: int
    mean_count: int
    perturb: bool
    align: int
    force_all_rays: bool
    dt_gamma: float
    max_steps: int
    T_thresh: float
    density_scale: float
    bg_scalar: float
    min_near: float
    offsets: torch.Tensor               # the hash grid's level offsets (int32, on the device)
    grid: GridSpec
    sigma: MlpShape
    colour: MlpShape
    colour_input_pad: float             # the colour input's last column (plan.colour_input_pad): 31 of the 32-wide row, 47 with an object feature
    want_sumsq: bool                    # the tail also returns the per-ray sums of sigma^2 (an object-conditioned network with a ray mask)
    want_dist: bool = False             # the tail also returns the per-ray distortion
    want_depth_grad: bool = False       # `depth` carries a gradient (the tail also keeps depth_raw)


_NODE_FIELDS = frozenset(name for name, _ in FocOccTrainNode._fields_)


def _forward_node(cfg, n, M, grid_bytes, **buffers):
    """The FocOccTrainNode of one forward (include/focnerf.h): the shapes of `cfg` and the node's own buffers, tensors (or None) under the
    struct's field names."""
    assert buffers.keys() <= _NODE_FIELDS, sorted(buffers.keys() - _NODE_FIELDS)
    grid, sigma, colour = cfg.grid, cfg.sigma, cfg.colour
    gridtype, align_corners, interp = grid.tail()
    return FocOccTrainNode(
        struct_bytes=ctypes.sizeof(FocOccTrainNode), n_rays=n, max_steps=cfg.max_steps, cascade=cfg.cascade, grid_size=cfg.grid_size, cap=M, pad_align=0,
        bound=cfg.bound, dt_gamma=cfg.dt_gamma, min_near=cfg.min_near,
        levels=cfg.offsets.shape[0] - 1, base_resolution=int(grid.base_resolution), gridtype=int(gridtype), interp=int(interp),
        align_corners=int(bool(align_corners)), table_dtype=FOC_F16, per_level_scale_log2=float(grid.log2_scale),
        offsets=_a(cfg.offsets), offsets_host=_gridencoder._host_offsets(cfg.offsets), grid_workspace_bytes=grid_bytes,
        sigma_input_dim=sigma.input_dim, sigma_hidden=sigma.hidden_dim, sigma_layers=sigma.num_layers, sigma_activation=sigma.activation, sigma_output_activation=6,
        color_hidden=64, color_layers=colour.num_layers, color_activation=colour.activation, c_width=_C_WIDTH,
        T_thresh=cfg.T_thresh, density_scale=cfg.density_scale, bg_scalar=cfg.bg_scalar,
        **{name: _a(t) for name, t in buffers.items()})


class _occ_train(Function):
    """(embeddings, sigma weights, colour weights, obj, ...) -> (image, weights_sum, depth, ray_sumsq or None, ray_dist or None). obj None: a plain network
    (pad 0) or the legacy tinycudann layout (column 31 = pad). obj [16] (any float dtype): the 48-wide colour head with the encoded object
    feature, which is differentiable, column 47 = pad; with cfg.want_sumsq the tail also returns ray_sumsq [n] = the sum of sigma^2 over all
    of a ray's samples (include/focnerf.h foc_occ_tail_forward_sumsq), differentiable too. With cfg.want_dist ray_dist [n] = the ray's distortion
    (foc_occ_tail_forward_dist), differentiable, with or without ray_sumsq. With cfg.want_depth_grad `depth` is differentiable
    (foc_occ_tail_backward_depth), else marked non-differentiable. Two routes: the one-call node (foc_occ_train_forward / _backward, their
    _pad31 or _obj form; with want_dist or want_depth_grad the _tail pair) and the call-by-call chain (FOC_OCC_NATIVE_NODE=0, an
    unbudgeted list)."""

    @staticmethod
    def forward(ctx, emb, w_sigma, w_color, obj, o, d, aabb, bitfield, counter, bg_ray, cfg):
        grid, sigma, colour, offsets, pad, want_sumsq = cfg.grid, cfg.sigma, cfg.colour, cfg.offsets, cfg.colour_input_pad, cfg.want_sumsq
        S, H, (gridtype, align_corners, interp) = grid.log2_scale, grid.base_resolution, grid.tail()
        n, dev = o.shape[0], o.device
        st = stream_of(o)
        budgeted = cfg.mean_count > 0 and not cfg.force_all_rays
        cap = _round_up(cfg.mean_count, cfg.align) if budgeted else n * cfg.max_steps
        enc_in, deltas, sh = _sample_block(cap, dev)
        rays = torch.empty(n, 3, dtype=torch.int32, device=dev)
        nf = torch.empty(2, n, dtype=torch.float32, device=dev)         # nears, fars: written by the march's count pass (the box test of near_far_from_aabb)
        nears, fars = nf[0], nf[1]
        jitter = torch.rand(n, dtype=torch.float32, device=dev) if cfg.perturb else _no_jitter(n, dev)
        scratch = _scratch.get("march", lib.foc_march_rays_train_scratch_bytes(n, cfg.max_steps), dev)
        L = offsets.shape[0] - 1
        obj16 = object_feature_half(obj, "occupancy training node")
        emb16, ws16, wc16 = _half_of(emb), _half_of(w_sigma), _half_of(w_color)
        out = torch.empty(n * (9 if want_sumsq else 8), dtype=torch.float32, device=dev)
        ws, depth, image_raw, image = out[:n], out[n: 2 * n], out[2 * n: 5 * n].view(n, 3), out[5 * n: 8 * n].view(n, 3)
        sumsq = out[8 * n:] if want_sumsq else None
        want_dist, want_depth = cfg.want_dist, cfg.want_depth_grad
        plan = _native_plan(offsets, grid, L, cap, sigma, colour, 32 if obj is None else 48) if (budgeted and cap > 0 and n > 0) else None
        rays_out = torch.empty((2 * want_dist + want_depth) * n, dtype=torch.float32, device=dev) if (want_dist or want_depth) else None
        dist, wm = (rays_out[:n], rays_out[n: 2 * n]) if want_dist else (None, None)
        draw = rays_out[2 * n * want_dist:] if want_depth else None          # depth_raw: the composite's depth before its normalisation
        M = cap
        ctx.node = ctx.object = ctx.tail = None
        if plan is not None:
            # the whole forward as one library call (csrc/occtrain.hip foc_occ_train_forward): the same five entry points in the same order,
            # enqueued from C — the step's host time no longer depends on nine trips through the binding
            planes = torch.empty(L, M, 2, dtype=torch.float16, device=dev)
            hc = torch.empty(M * (16 + _C_WIDTH), dtype=torch.float16, device=dev)
            h, c = hc[: M * 16].view(M, 16), hc[M * 16:].view(M, _C_WIDTH)
            gws = _scratch.get("grid_bwd", plan[0], dev)
            nd = _forward_node(cfg, n, M, plan[0], rays_o=o, rays_d=d, aabb=aabb, jitter=jitter, bitfield=bitfield, nears=nears, fars=fars, enc_in=enc_in,
                               deltas=deltas, sh_rows=sh, rays=rays, counter=counter, march_scratch=scratch, embeddings=emb16, planes=planes, grid_workspace=gws,
                               w_sigma=ws16, w_color=wc16, h=h, c=c, bg_ray=bg_ray, weights_sum=ws, image_raw=image_raw, image=image, depth=depth)
            ob = None
            if obj is not None:                             # what the object adds travels beside the node
                ob = ctx.object = FocOccTrainObject()
                ob.struct_bytes, ob.input_pad, ob.obj_feat, ob.ray_sumsq = ctypes.sizeof(FocOccTrainObject), float(pad), _a(obj16), _a(sumsq)
            if rays_out is not None:                        # so do the tail's optional outputs: one entry point for the three layouts
                tl = ctx.tail = FocOccTrainTail()
                tl.struct_bytes, tl.ray_dist, tl.ray_wm, tl.depth_raw = ctypes.sizeof(FocOccTrainTail), _a(dist), _a(wm), _a(draw)
                check(lib.foc_occ_train_forward_tail(ctypes.byref(nd), ctypes.byref(ob) if ob is not None else None, pad, ctypes.byref(tl), st),
                      "occ_train_forward_tail")
            elif ob is not None:
                check(lib.foc_occ_train_forward_obj(ctypes.byref(nd), ctypes.byref(ob), st), "occ_train_forward_obj")
            elif pad != 0:                                  # column 31 of the colour input = pad: the node's twin, the pad beside the node
                check(lib.foc_occ_train_forward_pad31(ctypes.byref(nd), pad, st), "occ_train_forward_pad31")
            else:
                check(lib.foc_occ_train_forward(ctypes.byref(nd), st), "occ_train_forward")
            # the count pass rode in the encoder's forward: the ticket the backward checks, as backend.grid_encode_forward_counted issues it
            ticket = _gridencoder.issue_precount_ticket(enc_in, M, L, FOC_F16, gws)
            ctx.node, ctx.plan = nd, plan
        else:
            check(lib.foc_march_rays_train_field(ptr(o), ptr(d), ptr(bitfield), cfg.bound, cfg.dt_gamma, cfg.max_steps, n, cfg.cascade, cfg.grid_size, cap,
                                                 ptr(nears), ptr(fars), ptr(enc_in), ptr(sh), ptr(deltas), ptr(rays), ptr(counter), ptr(jitter), ptr(scratch),
                                                 0 if budgeted else max(cfg.align, 1), ptr(aabb), cfg.min_near, st), "march_rays_train_field")
            if not budgeted:                                        # raymarching.py:223-229: the list is cut to the samples marched (one device -> host copy)
                M = min(cap, _round_up(int(counter[0].item()), cfg.align))
                enc_in, deltas, sh = enc_in[:M], deltas[:M], sh[:M]
            planes = torch.empty(L, M, 2, dtype=torch.float16, device=dev)
            ticket = _gridencoder.grid_encode_forward_counted(enc_in, emb16, offsets, planes, M, 3, 2, L, S, H, gridtype, align_corners, interp) if M else None
            if ticket is None and M:
                _gridencoder.grid_encode_forward(enc_in, emb16, offsets, planes, M, 3, 2, L, S, H, None, gridtype, align_corners, interp)
            h = torch.empty(M, 16, dtype=torch.float16, device=dev)
            c = torch.empty(M, _C_WIDTH, dtype=torch.float16, device=dev)
            if M:
                _ffmlp.ffmlp_forward_planar(planes, ws16, M, sigma.input_dim, 16, sigma.hidden_dim, sigma.num_layers, sigma.activation, 6, h)
                fn, extra = pad_twin("foc_color_head_forward", pad, obj is not None)
                check(fn(ptr(h), ptr(sh), 1, ptr(wc16), M, 64, colour.num_layers, colour.activation, ptr(c), _C_WIDTH, ptr(obj16), *extra, st), "color_head_forward")
            tail = (ptr(h), ptr(c), _C_WIDTH, ptr(deltas), ptr(rays), M, n, cfg.T_thresh, cfg.density_scale, ptr(bg_ray), cfg.bg_scalar,
                    ptr(nears), ptr(fars), ptr(ws), ptr(image_raw), ptr(image), ptr(depth))
            if want_depth:
                check(lib.foc_occ_tail_forward_depth(*tail, ptr(sumsq), ptr(dist), ptr(wm), ptr(draw), st), "occ_tail_forward_depth")
            elif want_dist:
                check(lib.foc_occ_tail_forward_dist(*tail, ptr(sumsq), ptr(dist), ptr(wm), st), "occ_tail_forward_dist")
            elif want_sumsq:
                check(lib.foc_occ_tail_forward_sumsq(*tail, ptr(sumsq), st), "occ_tail_forward_sumsq")
            else:
                check(lib.foc_occ_tail_forward(*tail, st), "occ_tail_forward")
        ctx.save_for_backward(enc_in, emb16, ws16, wc16, offsets, planes, h, c, sh, deltas, rays, counter, ws, image_raw,
                              bg_ray if bg_ray is not None else torch.empty(0, device=dev), *((rays_out,) if rays_out is not None else ()))
        ctx.want = (want_dist, want_depth)
        ctx.obj16 = obj16
        ctx.obj_like = (obj.dtype, obj.shape) if obj is not None else None
        ctx.bg_grad = bg_ray is not None and ctx.needs_input_grad[9]
        ctx.has_bg = bg_ray is not None
        ctx.nears_fars = nf
        ctx.cfg = (M, n, cfg.T_thresh, cfg.density_scale, cfg.bg_scalar, grid, sigma, colour, pad)
        ctx.ticket = ticket
        if not want_depth:
            ctx.mark_non_differentiable(depth)
        ctx.set_materialize_grads(False)
        return image, ws, depth, sumsq, dist

    @staticmethod
    def backward(ctx, g_image, g_ws, g_depth, g_sumsq, g_dist=None):
        """-> the gradients of the embeddings, the two weight blobs, obj (in its dtype and shape) and a per-ray background."""
        enc_in, emb16, ws16, wc16, offsets, planes, h, c, sh, deltas, rays, counter, ws, image_raw, bg_ray, *rays_out = ctx.saved_tensors
        M, n, T_thresh, density_scale, bg_scalar, grid, sigma, colour, pad = ctx.cfg
        S, H, (gridtype, align_corners, interp) = grid.log2_scale, grid.base_resolution, grid.tail()
        obj16 = ctx.obj16
        dev = h.device
        st = stream_of(h)
        L = offsets.shape[0] - 1
        want_dist, want_depth = ctx.want
        if not want_depth:
            g_depth = None                                      # the reference's composite ignores grad_depth (raymarching.cu:601-693)
        dist, wm = (rays_out[0][:n], rays_out[0][n: 2 * n]) if want_dist else (None, None)
        draw = rays_out[0][2 * n * want_dist:] if want_depth else None

        def result(g_emb, g_wsig, g_wcol, g_obj, g_bg):
            if g_obj is not None:
                g_obj = g_obj.to(ctx.obj_like[0]).view(ctx.obj_like[1])
            return g_emb, g_wsig, g_wcol, g_obj, None, None, None, None, None, g_bg, None

        g_emb = torch.zeros_like(emb16)
        g_wsig, g_wcol = torch.empty_like(ws16), torch.empty_like(wc16)
        if M == 0 or (g_image is None and g_ws is None and g_sumsq is None and g_dist is None and g_depth is None):
            g_bg = g_image * (1 - ws).unsqueeze(-1) if ctx.bg_grad and g_image is not None else None
            return result(g_emb, g_wsig.zero_(), g_wcol.zero_(), (torch.zeros(16, dtype=torch.float32, device=dev) if obj16 is not None else None), g_bg)
        g_image = g_image.contiguous().float() if g_image is not None else torch.zeros(n, 3, dtype=torch.float32, device=dev)
        g_ws = g_ws.contiguous().float() if g_ws is not None else None
        g_sumsq = g_sumsq.contiguous().float() if g_sumsq is not None else None
        g_dist = g_dist.contiguous().float() if g_dist is not None else None
        g_depth = g_depth.contiguous().float() if g_depth is not None else None
        # a learned background (network_linear.py): image = raw + (1 - ws) bg
        g_bg = g_image * (1 - ws).unsqueeze(-1) if ctx.bg_grad else None
        g_obj = torch.empty(16, dtype=torch.float32, device=dev) if obj16 is not None else None
        gblock = torch.empty(M * (_C_WIDTH + 1), dtype=torch.float16, device=dev)      # grad_c [M,4] | grad_h0 [M]: every row written by the kernel
        grad_h = torch.empty_like(h)                            # its own block: 32-byte rows written with 16-byte stores, M need not be a multiple of 8
        g_planes = torch.empty_like(planes)
        nd = ctx.node
        if nd is not None:                                      # the whole backward as one library call (foc_occ_train_backward)
            gws = _scratch.get("grid_bwd", ctx.plan[0], dev)
            mws = _scratch.get("ffmlp_ws", ctx.plan[1], dev)
            nd.grad_image, nd.grad_ws = _a(g_image), _a(g_ws)
            nd.grad_c, nd.grad_h0, nd.grad_h = gblock.data_ptr(), gblock.data_ptr() + 2 * M * _C_WIDTH, _a(grad_h)
            nd.grad_planes, nd.grad_w_color, nd.grad_w_sigma, nd.grad_embeddings = _a(g_planes), _a(g_wcol), _a(g_wsig), _a(g_emb)
            nd.mlp_workspace, nd.mlp_workspace_bytes, nd.grid_workspace, nd.grid_workspace_bytes = _a(mws), mws.numel(), _a(gws), ctx.plan[0]
            nd.precounted = int(_gridencoder._precount_valid(ctx.ticket, enc_in, M, L, FOC_F16, gws))
            ob, tl = ctx.object, ctx.tail
            if ob is not None:
                ob.grad_sumsq, ob.grad_obj = _a(g_sumsq), _a(g_obj)
            if tl is not None:
                tl.grad_dist, tl.grad_depth = _a(g_dist), _a(g_depth)
                check(lib.foc_occ_train_backward_tail(ctypes.byref(nd), ctypes.byref(ob) if ob is not None else None, pad, ctypes.byref(tl), st),
                      "occ_train_backward_tail")
            elif ob is not None:
                check(lib.foc_occ_train_backward_obj(ctypes.byref(nd), ctypes.byref(ob), st), "occ_train_backward_obj")
            elif pad != 0:
                check(lib.foc_occ_train_backward_pad31(ctypes.byref(nd), pad, st), "occ_train_backward_pad31")
            else:
                check(lib.foc_occ_train_backward(ctypes.byref(nd), st), "occ_train_backward")
            _gridencoder._invalidate_precount(dev)              # the header now belongs to this pass (and a used ticket is spent)
            ctx.node = ctx.object = ctx.tail = None
            return result(g_emb, g_wsig, g_wcol, g_obj, g_bg)
        grad_c, grad_h0 = gblock[: M * _C_WIDTH].view(M, _C_WIDTH), gblock[M * _C_WIDTH:]
        tail = (ptr(g_image), ptr(g_ws), ptr(h), ptr(c), _C_WIDTH, ptr(deltas), ptr(rays), ptr(counter), ptr(ws), ptr(image_raw), M, n,
                T_thresh, density_scale, ptr(bg_ray if ctx.has_bg else None), bg_scalar, ptr(grad_c), ptr(grad_h0))
        if want_depth:
            nf = ctx.nears_fars
            check(lib.foc_occ_tail_backward_depth(*tail, ptr(g_sumsq), ptr(wm), ptr(dist), ptr(g_dist), ptr(nf[0]), ptr(nf[1]), ptr(draw), ptr(g_depth), st),
                  "occ_tail_backward_depth")
        elif g_dist is not None:
            check(lib.foc_occ_tail_backward_dist(*tail, ptr(g_sumsq), ptr(wm), ptr(dist), ptr(g_dist), st), "occ_tail_backward_dist")
        elif g_sumsq is not None:
            check(lib.foc_occ_tail_backward_sumsq(*tail, ptr(g_sumsq), st), "occ_tail_backward_sumsq")
        else:
            check(lib.foc_occ_tail_backward(*tail, st), "occ_tail_backward")
        wsb = _scratch.get("ffmlp_ws", lib.foc_ffmlp_backward_workspace_bytes(32 if obj16 is None else 48, 64, colour.num_layers), dev)
        fn, extra = pad_twin("foc_color_head_backward", pad, obj16 is not None)
        check(fn(ptr(grad_c), ptr(h), ptr(sh), 1, ptr(grad_h0), ptr(wc16), M, 64, colour.num_layers, colour.activation, ptr(grad_h), ptr(g_wcol),
                 ptr(wsb), wsb.numel(), _C_WIDTH, ptr(obj16), ptr(g_obj), *extra, st), "color_head_backward")
        _ffmlp.ffmlp_backward_planar(grad_h, planes, ws16, M, sigma.input_dim, 16, sigma.hidden_dim, sigma.num_layers, sigma.activation, 6, True,
                                     g_planes, g_wsig)
        _gridencoder.grid_encode_backward(g_planes, enc_in, emb16, offsets, g_emb, M, 3, 2, L, S, H, None, None, gridtype, align_corners, interp, grad_bl=False,
                                          precount=ctx.ticket)
        return result(g_emb, g_wsig, g_wcol, g_obj, g_bg)


def ray_mask(mask, n):
    """FOC's object mask for a ragged sample list -> bool [n], one entry per ray ([N], [1,N] or [1,N,1]). A per-sample mask has no meaning
    here: any other size raises, before anything is launched."""
    mask = torch.as_tensor(mask)
    if mask.numel() != n:
        raise ValueError(f"occupancy-grid path: the object mask must have one entry per ray ({n}), got shape {tuple(mask.shape)}")
    return mask.reshape(n).bool()


def render_occupancy_train(model, plan, o, d, counter, bg_color, perturb, force_all_rays, dt_gamma, max_steps, T_thresh, align, obj16=None, want_sumsq=False,
                           want_dist=False, want_depth_grad=False):
    """o, d [n,3] fp32 contiguous, counter int32[2] (zeroed by the caller) -> (image [n,3], weights_sum [n], depth [n], ray_sumsq [n] or None),
    with want_dist a fifth entry ray_dist [n] (the ray's distortion, differentiable); with want_depth_grad `depth` carries a gradient
    (module docstring),
    for a network whose `field.field_plan` is `plan` (plan.occ; plan.occ_object with obj16 [16], the encoded object feature, which receives
    a gradient); the rays' box test against the model's training box (near_far_from_aabb, min_near) happens inside the march."""
    if want_sumsq and obj16 is None:
        raise ValueError("render_occupancy_train: want_sumsq needs obj16 (only the object-conditioned node returns ray_sumsq)")
    enc = model.encoder
    bg_ray, bg_scalar = _background(bg_color, o.shape[0], o.device)
    cfg = OccTrainConfig(
        bound=float(model.bound), cascade=int(model.cascade), grid_size=int(model.grid_size), mean_count=int(model.mean_count), perturb=bool(perturb),
        align=int(align), force_all_rays=bool(force_all_rays), dt_gamma=float(dt_gamma), max_steps=int(max_steps), T_thresh=float(T_thresh),
        density_scale=float(model.density_scale), bg_scalar=float(bg_scalar), min_near=float(model.min_near), offsets=enc.offsets, grid=plan.grid,
        sigma=plan.sigma, colour=plan.colour, colour_input_pad=float(plan.colour_input_pad), want_sumsq=bool(want_sumsq), want_dist=bool(want_dist),
        want_depth_grad=bool(want_depth_grad))
    res = _occ_train.apply(enc.embeddings, fused_mlp(model, "sigma_net").weights, fused_mlp(model, "color_net").weights, obj16, o, d,
                           model._aabb().contiguous().float(), model.density_bitfield, counter, bg_ray, cfg)
    return res if want_dist else res[:4]
