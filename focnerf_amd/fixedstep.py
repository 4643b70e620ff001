"""Fused fixed-step render path (FOC's default: num_steps samples per ray, no occupancy grid).

`render_fixed_steps(model, rays_o, rays_d, ...)` computes what `NeRFRenderer.run` computes
(nerf/renderer.py:126-238 with upsample_steps=0) for a `focnerf_amd.network.NeRFNetwork`, with the torch
glue replaced by the kernels of csrc/fixedstep.hip:

    near_far_from_aabb -> fixed_sample -> grid_encode -> sigma_net -> [density head] -> color_net -> [composite]

The two bracketed stages are autograd Functions defined here. The colour network is evaluated on every
sample and masked by `weights > weight_thresh` inside the composite, which yields the same image and the
same gradients as the reference's gather -> MLP -> scatter (masked-out samples get rgb = 0 and no gradient).
SURVEY.md §8(f)-3. Parity is tested against `NeRFRenderer.run` on the same network (tests/test_gpu_fixedstep.py).
"""
import torch
from torch.autograd import Function

from . import raymarching
from ._lib import lib, ptr, stream_of, check
from .gridencoder import grid_encode


RAY_BLOCK = 64      # block-interleaved sample order of the inference path (csrc/fixedstep.hip, fs_block_row)


def ray_block_default():
    """Sample order of the fused inference path: 64-ray blocks unless FOC_RAY_BLOCK=0 (ray-major, the round-1 order)."""
    import os
    return RAY_BLOCK if os.environ.get("FOC_RAY_BLOCK", str(RAY_BLOCK)) != "0" else 0


def blocked_rows(N, T, ray_block):
    """Rows of the per-sample arrays of N rays x T samples in the given order (the last 64-ray block is padded)."""
    return N * T if not ray_block else -(-N // ray_block) * ray_block * T


def fixed_sample(rays_o, rays_d, nears, fars, aabb, noise, T, bound, want_xyzs=False, want_ray_sh=False, ray_block=0):
    """ray_block = 64: rows in the block-interleaved order (include/focnerf.h), `blocked_rows(N, T, 64)` of them."""
    N = rays_o.shape[0]
    dev = rays_o.device
    rows = blocked_rows(N, T, ray_block)
    enc_in = torch.empty(rows, 3, dtype=torch.float32, device=dev)
    xyzs = torch.empty(rows, 3, dtype=torch.float32, device=dev) if want_xyzs else None
    ray_sh = torch.empty(N, 16, dtype=torch.float16, device=dev) if want_ray_sh else None
    check(lib.foc_fixed_sample(ptr(rays_o), ptr(rays_d), ptr(nears), ptr(fars), ptr(aabb), ptr(noise), N, T, float(bound), ptr(xyzs), ptr(enc_in),
                               ptr(ray_sh), int(ray_block), stream_of(rays_o)), "fixed_sample")
    if want_ray_sh:
        return enc_in, xyzs, ray_sh
    return enc_in, xyzs


def ray_sh_rows(rays_d):
    """[N,3] directions -> [N,16] half: each ray's degree-4 SH values as they stand in the colour-net input."""
    rays_d = rays_d.contiguous().float()
    N, dev = rays_d.shape[0], rays_d.device
    zeros, ones = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    aabb = torch.tensor([-1., -1., -1., 1., 1., 1.], device=dev)
    return fixed_sample(torch.zeros_like(rays_d), rays_d, zeros, ones, aabb, None, 2, 1.0, want_ray_sh=True)[2]


class _density_head(Function):
    """h [M,16] half -> (weights [M], weights_sum [N], depth [N], sigma [M], cin [M,32] half)."""

    @staticmethod
    def forward(ctx, h, rays_d, nears, fars, noise, N, T, density_scale, obj_feat=None):
        """obj_feat: None -> cin [M,32]; [16] half (FOC network's encoded object feature) -> cin [M,48]."""
        from .field import object_feature_half
        h = h.contiguous()
        assert h.dtype == torch.float16 and h.shape == (N * T, 16)
        dev = h.device
        M = N * T
        sigma = torch.empty(M, dtype=torch.float32, device=dev)
        trans = torch.empty(M, dtype=torch.float32, device=dev)
        weights = torch.empty(M, dtype=torch.float32, device=dev)
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        width = 32 if obj_feat is None else 48
        obj_feat = object_feature_half(obj_feat, "_density_head")
        cin = torch.empty(M, width, dtype=torch.float16, device=dev)
        check(lib.foc_fixed_head_forward(ptr(h), ptr(rays_d), ptr(nears), ptr(fars), ptr(noise), N, T, float(density_scale), ptr(sigma), ptr(trans),
                                         ptr(weights), ptr(ws), ptr(depth), ptr(cin), ptr(obj_feat), width, stream_of(h)), "fixed_head_forward")
        ctx.save_for_backward(h, sigma, trans, nears, fars, noise if noise is not None else torch.empty(0, device=dev))
        ctx.has_noise = noise is not None
        ctx.dims = (N, T, float(density_scale))
        ctx.width = width
        ctx.mark_non_differentiable(sigma)
        ctx.set_materialize_grads(False)
        return weights, ws, depth, sigma, cin

    @staticmethod
    def backward(ctx, g_weights, g_ws, g_depth, g_sigma, g_cin):
        h, sigma, trans, nears, fars, noise = ctx.saved_tensors
        N, T, ds = ctx.dims
        noise = noise if ctx.has_noise else None
        g_weights = g_weights.contiguous().float() if g_weights is not None else None
        g_ws = g_ws.contiguous().float() if g_ws is not None else None
        g_depth = g_depth.contiguous().float() if g_depth is not None else None
        g_cin = g_cin.contiguous().half() if g_cin is not None else None
        grad_h = torch.empty_like(h)
        check(lib.foc_fixed_head_backward(ptr(h), ptr(sigma), ptr(trans), ptr(nears), ptr(fars), ptr(noise), ptr(g_weights), ptr(g_ws), ptr(g_depth),
                                          ptr(g_cin), N, T, ds, ptr(grad_h), ctx.width, stream_of(h)), "fixed_head_backward")
        g_obj = None
        if ctx.width == 48 and ctx.needs_input_grad[8] and g_cin is not None:
            g_obj = g_cin[:, 31:47].float().sum(0)                 # one feature vector feeds every sample
        return grad_h, None, None, None, None, None, None, None, g_obj


class _fixed_composite(Function):
    """c [M,16] half (colour-net output), weights [M] -> image [N,3] = sum w*sigmoid(c)*[w>thresh] + (1 - sum w)*bg.
    A per-ray bg_ray that needs a gradient (a learned background, network_linear.py) gets g_image * (1 - weights_sum): `weights_sum` [N]
    is then required."""

    @staticmethod
    def forward(ctx, c, weights, bg_ray, bg_scalar, N, T, thresh, weights_sum=None):
        c = c.contiguous()
        weights = weights.contiguous()
        assert c.dtype == torch.float16 and c.shape == (N * T, 16) and weights.dtype == torch.float32
        image = torch.empty(N, 3, dtype=torch.float32, device=c.device)
        check(lib.foc_fixed_composite_forward(ptr(c), ptr(weights), ptr(bg_ray), float(bg_scalar), N, T, float(thresh), ptr(image), stream_of(c)),
              "fixed_composite_forward")
        ctx.bg_grad = bg_ray is not None and ctx.needs_input_grad[2]
        if ctx.bg_grad and weights_sum is None:
            raise RuntimeError("_fixed_composite: a background that needs a gradient needs weights_sum")
        empty = torch.empty(0, device=c.device)
        ctx.save_for_backward(c, weights, bg_ray if bg_ray is not None else empty, weights_sum.detach() if ctx.bg_grad else empty)
        ctx.has_bg = bg_ray is not None
        ctx.dims = (N, T, float(thresh), float(bg_scalar))
        return image

    @staticmethod
    def backward(ctx, g_image):
        c, weights, bg_ray, weights_sum = ctx.saved_tensors
        N, T, thresh, bg_scalar = ctx.dims
        bg_ray = bg_ray if ctx.has_bg else None
        g_image = g_image.contiguous().float()
        grad_c = torch.empty_like(c)
        grad_w = torch.empty_like(weights)
        check(lib.foc_fixed_composite_backward(ptr(g_image), ptr(c), ptr(weights), ptr(bg_ray), bg_scalar, N, T, thresh, ptr(grad_c), ptr(grad_w),
                                               stream_of(c)), "fixed_composite_backward")
        g_bg = g_image * (1 - weights_sum).unsqueeze(-1) if ctx.bg_grad else None
        return grad_c, grad_w, g_bg, None, None, None, None, None


_C_WIDTH = 4        # columns of the colour network's output that exist in memory on the fused tail (rgb logits + one pad)


class _render_tail(Function):
    """Density head -> colour network -> composite as ONE node: h [M,16] half + the colour network's weight blob ->
    image [N,3], weights_sum [N], depth [N] (+ sigma [M], weights [M], c [M,4] = rgb logits + one pad column, not differentiable).

    Same values and gradients as `_density_head` -> `FFMLP.forward_padded` -> `_fixed_composite`, bit for bit, without the colour
    network's input: its kernels read h and one SH row per ray (foc_color_head_forward), and in the backward pass the colour
    network writes grad_h itself — its input gradient for columns 1..15 merged with the density path's column 0 — so neither
    cin [M,32] nor grad_cin [M,32] exists (0.5 GB of traffic per 2 M-sample step). Head and composite are one kernel per
    direction (foc_fixed_tail_forward / _backward). ray_sh [N,16] half: `fixed_sample(..., want_ray_sh=True)` or `ray_sh_rows`.

    obj_feat [16] (or None): FOC's encoded object feature — the colour network then has 48-wide W0 rows; the feature's share of layer 0
    is a constant per neuron inside the kernels, its gradient (for the object-feature encoder) comes back as one [16] vector.
    want_sumsq: a seventh, differentiable output sumsq [N] = sum_t sigma^2 per ray (the samples' share of the outside-mask criterion).
    input_pad: the last column of the colour input: 0, or 1.0 for the tinycudann layouts — column 47 of the 48-wide row with obj_feat
    (network_tcnn.py), column 31 of the 32-wide row without (network_tcnn_legacy.py); then the *_pad / *_pad31 twins of the colour-head
    kernels run.
    want_dist: one more differentiable output, after sumsq when both are asked for: dist [N] = the ray's distortion (loss.ray_distortion of
    the raw weights with m = (z - near) + delta / 2 and the interval delta; foc_fixed_tail_forward_dist / _backward_dist). Off: the calls, the
    buffers and the values of the node without it."""

    @staticmethod
    def forward(ctx, h, cweights, ray_sh, nears, fars, noise, bg_ray, bg_scalar, N, T, density_scale, thresh, num_layers, activation, obj_feat=None,
                want_sumsq=False, c_pre=None, w16_pre=None, input_pad=0.0, want_dist=False):
        # c_pre [M,4] half: the colour logits already computed from this h, these weights and this ray_sh by the encoder -> sigma node's fused
        # forward (field._hashgrid_mlp with `colour`, foc_field_forward_train: the bits foc_color_head_forward would give) — then no launch here
        from .field import _half_of, pad_twin, object_feature_half
        h = h.contiguous()
        assert h.dtype == torch.float16 and h.shape == (N * T, 16)
        assert ray_sh.dtype == torch.float16 and ray_sh.shape == (N, 16) and ray_sh.is_contiguous()
        dev, M = h.device, N * T
        st = stream_of(h)
        w16 = w16_pre if w16_pre is not None else _half_of(cweights)     # w16_pre: the half copy the fused forward already made of THESE weights
        # of the colour network's 16 padded outputs only the rgb logits are ever read: they travel as [M,4] rows (as does their gradient)
        obj16 = object_feature_half(obj_feat, "_render_tail")
        assert obj16 is None or w16.numel() == 64 * (48 + 64 * (int(num_layers) - 1) + 16)
        if c_pre is not None:
            assert c_pre.dtype == torch.float16 and c_pre.shape == (M, _C_WIDTH) and c_pre.is_contiguous()
            c = c_pre
        else:
            c = torch.empty(M, _C_WIDTH, dtype=torch.float16, device=dev)
            args = (ptr(h), ptr(ray_sh), T, ptr(w16), M, 64, int(num_layers), int(activation), ptr(c), _C_WIDTH, ptr(obj16))
            fn, extra = pad_twin("foc_color_head_forward", input_pad, obj16 is not None)
            check(fn(*args, *extra, st), "color_head_forward")
        sigma = torch.empty(M, dtype=torch.float32, device=dev)
        trans = torch.empty(M, dtype=torch.float32, device=dev)
        weights = torch.empty(M, dtype=torch.float32, device=dev)
        ws = torch.empty(N, dtype=torch.float32, device=dev)
        depth = torch.empty(N, dtype=torch.float32, device=dev)
        image = torch.empty(N, 3, dtype=torch.float32, device=dev)
        sumsq = torch.empty(N, dtype=torch.float32, device=dev) if want_sumsq else None
        tail = (ptr(h), ptr(c), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), float(bg_scalar), N, T, float(density_scale), float(thresh), ptr(sigma),
                ptr(trans), ptr(weights), ptr(ws), ptr(depth), ptr(image), _C_WIDTH, ptr(sumsq))
        dist = wm = None
        if want_dist:
            dist, wm = torch.empty(N, dtype=torch.float32, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
            check(lib.foc_fixed_tail_forward_dist(*tail, ptr(dist), ptr(wm), st), "fixed_tail_forward_dist")
        else:
            check(lib.foc_fixed_tail_forward(*tail, st), "fixed_tail_forward")
        empty = torch.empty(0, device=dev)
        ctx.bg_grad = bg_ray is not None and ctx.needs_input_grad[6]         # a learned background (network_linear.py): g_image * (1 - ws)
        ctx.save_for_backward(h, w16, sigma, trans, weights, c, ray_sh, nears, fars, noise if noise is not None else empty,
                              bg_ray if bg_ray is not None else empty, obj16 if obj16 is not None else empty,
                              ws if ctx.bg_grad or want_dist else empty, wm if want_dist else empty)
        ctx.outputs = (bool(want_sumsq), bool(want_dist))
        ctx.flags = (noise is not None, bg_ray is not None, obj16 is not None, obj_feat.dtype if obj_feat is not None else None,
                     tuple(obj_feat.shape) if obj_feat is not None else None)
        ctx.dims = (N, T, float(density_scale), float(thresh), float(bg_scalar), int(num_layers), int(activation), float(input_pad))
        ctx.mark_non_differentiable(sigma, weights, c)
        ctx.set_materialize_grads(False)          # unused outputs arrive as None in backward, not as five freshly zero-filled tensors (25 us)
        return (image, ws, depth, sigma, weights, c) + ((sumsq,) if want_sumsq else ()) + ((dist,) if want_dist else ())

    @staticmethod
    def backward(ctx, g_image, g_ws, g_depth, _g_sigma, _g_weights, _g_c, *g_extra):
        from .backend import _scratch
        from .field import pad_twin
        h, w16, sigma, trans, weights, c, ray_sh, nears, fars, noise, bg_ray, obj16, ws, wm = ctx.saved_tensors
        g_extra = list(g_extra)
        g_sumsq = g_extra.pop(0) if ctx.outputs[0] else None
        g_dist = g_extra.pop(0) if ctx.outputs[1] else None
        has_noise, has_bg, has_obj, obj_dtype, obj_shape = ctx.flags
        obj16 = obj16 if has_obj else None
        N, T, ds, thresh, bg_scalar, num_layers, activation, input_pad = ctx.dims
        noise = noise if has_noise else None
        bg_ray = bg_ray if has_bg else None
        dev, M = h.device, N * T
        st = stream_of(h)
        g_image = g_image.contiguous().float() if g_image is not None else torch.zeros(N, 3, dtype=torch.float32, device=dev)
        g_ws = g_ws.contiguous().float() if g_ws is not None else None
        g_depth = g_depth.contiguous().float() if g_depth is not None else None
        g_sumsq = g_sumsq.contiguous().float() if g_sumsq is not None else None
        grad_c = torch.empty_like(c)
        grad_h0 = torch.empty(M, dtype=torch.float16, device=dev)
        if g_dist is not None:
            g_dist = g_dist.contiguous().float()
            check(lib.foc_fixed_tail_backward_dist(ptr(g_image), ptr(g_ws), ptr(g_depth), ptr(c), ptr(sigma), ptr(trans), ptr(weights), ptr(ws), ptr(nears),
                                                   ptr(fars), ptr(noise), ptr(bg_ray), bg_scalar, N, T, ds, thresh, ptr(grad_c), ptr(grad_h0), _C_WIDTH,
                                                   ptr(g_sumsq), ptr(wm), None, ptr(g_dist), st), "fixed_tail_backward_dist")
        else:
            check(lib.foc_fixed_tail_backward(ptr(g_image), ptr(g_ws), ptr(g_depth), ptr(c), ptr(sigma), ptr(trans), ptr(weights), ptr(nears), ptr(fars),
                                              ptr(noise), ptr(bg_ray), bg_scalar, N, T, ds, thresh, ptr(grad_c), ptr(grad_h0), _C_WIDTH, ptr(g_sumsq), st),
                  "fixed_tail_backward")
        grad_h = torch.empty_like(h)
        g_w = torch.empty_like(w16)
        wsb = _scratch.get("ffmlp_ws", lib.foc_ffmlp_backward_workspace_bytes(48 if has_obj else 32, 64, num_layers), dev)
        g_obj32 = torch.empty(16, dtype=torch.float32, device=dev) if has_obj and ctx.needs_input_grad[14] else None
        args = (ptr(grad_c), ptr(h), ptr(ray_sh), T, ptr(grad_h0), ptr(w16), M, 64, num_layers, activation, ptr(grad_h), ptr(g_w), ptr(wsb),
                wsb.numel(), _C_WIDTH, ptr(obj16), ptr(g_obj32))
        fn, extra = pad_twin("foc_color_head_backward", input_pad, has_obj)
        check(fn(*args, *extra, st), "color_head_backward")
        g_obj = g_obj32.to(obj_dtype).view(obj_shape) if g_obj32 is not None else None
        g_bg = g_image * (1 - ws).unsqueeze(-1) if ctx.bg_grad else None
        return (grad_h, g_w, None, None, None, None, g_bg) + (None,) * 7 + (g_obj, None, None, None, None, None)


class _masked_norm(Function):
    """sqrt(sum(sumsq[outside])) with the subgradient 0 at 0 that torch.norm has: FOC's `criterion_outside_mask`
    (nerf/renderer.py:163-165: torch.norm(sigma[~mask_rays])) from the per-ray sums of sigma^2 the tail kernel returns."""

    @staticmethod
    def forward(ctx, sumsq, outside):
        crit = torch.sqrt((sumsq * outside).sum())
        ctx.save_for_backward(crit, outside)
        return crit

    @staticmethod
    def backward(ctx, g):
        crit, outside = ctx.saved_tensors
        coef = torch.where(crit > 0, g / (2 * crit), torch.zeros_like(crit))
        return outside * coef, None


def _unfused_distortion(weights, nears, fars, noise, N, T):
    """The distortion of the training route without the fused tail: loss.ray_distortion on the head's weights [N*T], with the sample depths of
    run() (torch's linspace and jitter expressions) and a ray that misses the box set to 0 like the tail kernels do."""
    from .loss import ray_distortion
    span = (fars - nears).unsqueeze(-1)
    z = span * torch.linspace(0.0, 1.0, T, device=weights.device).unsqueeze(0)         # z - near
    if noise is not None:
        z = z + (noise.view(N, T) - 0.5) * (span / T)
    delta = torch.cat([z[:, 1:] - z[:, :-1], span / T], dim=-1)
    live = (fars > nears).unsqueeze(-1)
    zero = torch.zeros_like(z)
    return ray_distortion(torch.where(live, weights.view(N, T), zero), torch.where(live, z + 0.5 * delta, zero), torch.where(live, delta, zero))


def _background(bg_color, N, dev):
    """bg_color None / scalar / tensor -> (per-ray [N,3] tensor or None, scalar)."""
    if bg_color is None:
        return None, 1.0
    if torch.is_tensor(bg_color):
        if bg_color.numel() > 1:
            return bg_color.to(dev, torch.float32).reshape(-1, 3).expand(N, 3).contiguous(), 0.0      # [3], [N,3] or the sampler's [1,N,3]
        return None, float(bg_color)
    return None, float(bg_color)


def render_fixed_steps(model, rays_o, rays_d, yolo_details=None, num_steps=512, bg_color=None, perturb=False, weight_thresh=1e-10,
                       return_fields=None, _out=None, distortion=False, **kwargs):
    """Drop-in for NeRFRenderer.run(..., upsample_steps=0) on a focnerf_amd NeRFNetwork (fp16 autocast semantics); same result
    dictionary (`return_fields` None = on in eval mode, like the reference's run(), off in training).

    distortion=True adds `results['distortion']`, shaped like `depth`: the per-ray distortion of mip-NeRF 360 (loss.ray_distortion of the raw
    weights, m = (z - near) + delta / 2, interval delta, world units; 0 on a ray that misses the box), differentiable — its mean is the
    reference's loss.eff_distloss. On the fused training tail it comes out of the tail kernels; on the training route without the tail from
    loss.ray_distortion on the head's weights. Without a gradient there are no weights to regularise: ValueError. Off (the default): every
    call, buffer and value is that of the path without the keyword."""
    import time
    if return_fields is None:
        return_fields = not model.training
    t_start = time.time()
    prefix = rays_o.shape[:-1]
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    N, T = rays_o.shape[0], int(num_steps)
    dev = rays_o.device
    aabb = model.aabb_train if model.training else model.aabb_infer
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, model.min_near)
    noise = torch.rand(N * T, dtype=torch.float32, device=dev) if perturb else None
    from .field import field_plan, field_infer
    plan = field_plan(model)
    if getattr(model, "bg_radius", 0) > 0:
        # the background model replaces bg_color (legacy/nerf/renderer.py:232-234); a learned one gets its gradient from the nodes below
        bg_color = model._background_colour(rays_o, rays_d, bg_color)
    want_tail = plan.tail and model.training and torch.is_grad_enabled()
    fused_infer = not torch.is_grad_enabled() and plan.infer
    if distortion and not torch.is_grad_enabled():
        raise ValueError("render_fixed_steps: distortion=True needs the training route (gradients enabled): the inference paths form no "
                         "differentiable weights; call it under torch.enable_grad() with model.train()")
    rb = ray_block_default() if fused_infer else 0
    enc_in, _, ray_sh = fixed_sample(rays_o, rays_d, nears, fars, aabb, noise, T, model.bound, want_ray_sh=True) if want_tail else \
        fixed_sample(rays_o, rays_d, nears, fars, aabb, noise, T, model.bound, ray_block=rb) + (None,)

    if fused_infer:
        # inference: sample -> encoder planes -> whole-field kernel -> weights + mask + composite kernel; between the kernels the samples
        # stand in 64-ray blocks (neighbouring rays at one depth on the lanes of a wave: the encoder's gathers share cache lines)
        obj_feat = model.encode_object_feature(yolo_details, dev) if plan.uses_object_feature else None
        sigma, rgb = field_infer(model, enc_in, rays_d, dir_div=T, dir_block=rb, obj_feat=obj_feat)
        bg_ray, bg_scalar = _background(bg_color, N, dev)
        # `_out` = (depth [N], image [N,3]) fp32 contiguous views of the caller's whole-view buffers (NeRFRenderer.render, staged)
        direct = (_out is not None and _out[0].dtype == torch.float32 and _out[1].dtype == torch.float32 and _out[0].is_contiguous()
                  and _out[1].is_contiguous() and _out[0].numel() == N and _out[1].numel() == 3 * N and _out[0].device == dev)
        depth, image = (_out[0].view(N), _out[1].view(N, 3)) if direct else (torch.empty(N, dtype=torch.float32, device=dev),
                                                                              torch.empty(N, 3, dtype=torch.float32, device=dev))
        weights_sum = torch.empty(N, dtype=torch.float32, device=dev)
        rgb_masked = densities = None
        if return_fields:
            # the whole-view field buffers of a staged render (`_out[2:]` = densities [N,T], rgbs [N,T,3] views): written in place
            if direct and len(_out) == 4 and all(t.dtype == torch.float32 and t.is_contiguous() and t.device == dev for t in _out[2:]) \
                    and _out[2].numel() == N * T and _out[3].numel() == 3 * N * T and rb:
                densities, rgb_masked = _out[2].view(N * T), _out[3].view(N * T, 3)
            else:
                rgb_masked = torch.empty(N * T, 3, dtype=torch.float32, device=dev)
                densities = torch.empty(N * T, dtype=torch.float32, device=dev) if rb else None
        check(lib.foc_fixed_render_inference(ptr(sigma), ptr(rgb), ptr(nears), ptr(fars), ptr(noise), ptr(bg_ray), float(bg_scalar), N, T,
                                             float(model.density_scale), float(weight_thresh), ptr(image), ptr(depth), ptr(weights_sum), ptr(rgb_masked),
                                             rb, ptr(densities), stream_of(sigma)), "fixed_render_inference")
        t_mid = time.time()
        results = {'depth': depth.view(*prefix), 'image': image.view(*prefix, 3), 'weights_sum': weights_sum, 'criterion_outside_mask': None,
                   'timing': [t_mid - t_start, time.time() - t_mid]}
        if return_fields:
            results['densities'] = (densities if rb else sigma).view(N, T, 1)
            results['rgbs'] = rgb_masked.view(N, T, 3)
        return results

    enc = model.encoder
    from .field import hashgrid_mlp, fused_mlp
    c_pre = obj_feat = None
    # the colour weight blob, read once per step (a packed blob, network_linear.py, is built on each read)
    cweights = fused_mlp(model, "color_net").weights if want_tail else None
    with torch.autocast("cuda", dtype=torch.float16):
        if plan.uses_object_feature:                                      # FOC network (network_foc.py): encoded YOLO feature in the colour input
            obj_feat = model.encode_object_feature(yolo_details, dev)
        if plan.field:
            # with the fused tail the colour network's forward rides in the sigma network's kernel (its logits reach _render_tail as `c_pre`)
            colour = wc16 = None
            if want_tail and plan.train_forward:
                from .field import _half_of
                wc16 = _half_of(cweights)                                 # ONE half copy per step for both nodes that read the colour weights
                colour = (wc16, plan.colour, ray_sh, T, _C_WIDTH, obj_feat, plan.colour_input_pad)
            h = hashgrid_mlp(enc, fused_mlp(model, "sigma_net"), enc_in, None, colour)
            if colour is not None:
                h, c_pre = h
        else:
            feats = grid_encode(enc_in, enc.embeddings, enc.offsets, enc.per_level_scale, enc.base_resolution, False, enc.gridtype_id,
                                enc.align_corners, enc.interp_id)
            h = fused_mlp(model, "sigma_net")(feats)                      # [M,16] half
        if h.shape[1] != 16:                                              # FFMLP slices to output_dim (= 16 here: 1 + geo_feat_dim 15)
            raise RuntimeError("render_fixed_steps expects a 16-wide sigma head (1 + geo_feat_dim = 16)")
        fused_tail = want_tail
        # nerf/renderer.py:163-165: in training with an object mask, the norm of the densities of the rays outside it
        want_crit = model.training and yolo_details is not None and yolo_details[0] is not None
        criterion_outside_mask = None
        if fused_tail:
            cn = fused_mlp(model, "color_net")
            bg_ray, bg_scalar = _background(bg_color, N, dev)
            outs = _render_tail.apply(h, cweights, ray_sh, nears, fars, noise, bg_ray, bg_scalar, N, T, model.density_scale, weight_thresh,
                                      cn.num_layers, cn.activation, obj_feat, want_crit and yolo_details[0].numel() == N, c_pre,
                                      wc16 if c_pre is not None else None, plan.colour_input_pad, *((True,) if distortion else ()))
            image, weights_sum, depth, sigma, weights, c = outs[:6]
            ray_dist = outs[-1] if distortion else None
            if len(outs) - bool(distortion) == 7:
                # a per-ray mask: the samples' sum of sigma^2 comes out of the tail kernel (no [M]-sized torch expression, no boolean-mask
                # indexing with its host sync); sigma here is the kernel's exp(h0) — density_scale == 1 in every FOC configuration, and the
                # criterion is taken on trunc_exp(h0) itself like the reference's
                criterion_outside_mask = _masked_norm.apply(outs[6], (~yolo_details[0].reshape(N)).to(torch.float32))
        else:
            weights, weights_sum, depth, sigma, cin = _density_head.apply(h, rays_d, nears, fars, noise, N, T, model.density_scale, obj_feat)
            if plan.colour_input_pad != 0:                                # the head kernel writes 0 in the last column (tinycudann layouts: the pad)
                cin = torch.cat([cin[:, :-1], cin.new_full((cin.shape[0], 1), plan.colour_input_pad)], dim=1)
            if distortion:
                ray_dist = _unfused_distortion(weights, nears, fars, noise, N, T)
        if want_crit and criterion_outside_mask is None:
            from .activation import trunc_exp
            criterion_outside_mask = torch.norm(trunc_exp(h[:, 0]).view(N, T)[~yolo_details[0].squeeze(0)] - 0)
        if not fused_tail:
            c = fused_mlp(model, "color_net").forward_padded(cin)          # [M,16] half, columns 0..2 = rgb logits
    t_mid = time.time()

    if not fused_tail:
        bg_ray, bg_scalar = _background(bg_color, N, dev)
        image = _fixed_composite.apply(c, weights, bg_ray, bg_scalar, N, T, weight_thresh, weights_sum)

    results = {'depth': depth.view(*prefix), 'image': image.view(*prefix, 3), 'weights_sum': weights_sum,
               'criterion_outside_mask': criterion_outside_mask, 'timing': [t_mid - t_start, time.time() - t_mid]}
    if distortion:
        results['distortion'] = ray_dist.view(*prefix)
    if return_fields:
        from .head import rgb_head
        c16 = c.detach()
        if c16.shape[1] != 16:                                                    # fused tail: [M,4] logits -> the 16-wide rows rgb_head reads
            c16 = torch.nn.functional.pad(c16, (0, 16 - c16.shape[1]))
        rgb = rgb_head(c16) * (weights > weight_thresh).unsqueeze(-1)            # half-rounded sigmoid, fp32 tensor (the composite's values)
        results['densities'] = sigma.view(N, T, 1)
        results['rgbs'] = rgb.view(N, T, 3)
    return results


@torch.no_grad()
def render_field4(model, rays_o, rays_d, num_steps=512, weight_thresh=1e-10, yolo_details=None, out=None, occupancy=None, placement=None,
                  scene_aabb=None, channels="rgb"):
    """What the combiner needs from one object for a chunk of rays — COMBINED.py's `run` (:451-534 with upsample_steps=0, perturb off):
    `densities` [N,T] and `rgbs` [N,T,3] (zero where the object's own compositing weight is <= 1e-10) — PACKED as field4 [N,T,4] fp32
    (sigma, r, g, b), written into `out` when given. Fused path: sample -> encoder -> whole-field kernel -> weights + mask + pack
    (foc_fixed_field_pack); other networks go through `model.run(..., return_fields=True)` and are packed with torch ops.

    occupancy (a `fixedcull.Occupancy`, default None = the dense path above, unchanged): the same T positions, but encoder and networks
    run only on the samples whose cell of the object's occupancy grid is set; every other sample is (0, 0, 0, 0). Sequence: near_far ->
    cull (csrc/fixedcull.hip) -> one host read of the occupied count -> encoder + whole-field kernel on that many rows -> culled pack.
    It is the approximation `run_cuda` makes: densities below the grid's threshold are dropped, so the transmittance behind such
    samples is slightly higher and a sample's own-weight mask can flip. The host read makes a call with `occupancy` uncapturable in a
    HIP graph (the dense path is as capturable as before). Needs a network the fused inference serves and no background model
    (ValueError otherwise: it never falls back to rendering dense), and a grid over the model's `bound`.

    placement (a `Placement`, default None = the paths above, unchanged; needs `occupancy`): the object stands rotated, scaled and moved
    in a scene. The T positions are those of the view's rays against `scene_aabb` (float32 [6] tensor, default the model's box); each is
    mapped into the object's frame, samples outside the object's own box are empty, and sigma is rescaled by 1 / scale
    (include/focnerf.h foc_fixed_cull_placed).

    channels ("rgb", the default: everything above, unchanged; or "normal"): "normal" puts the encoded surface normal 0.5 + 0.5 n where the
    colour stands (`normals.field_normals` in place of `field_infer`; with a placement the normal is rotated into the scene). Sigma, the
    own-weight mask and the pack are the same. Needs `field_plan(model).normals` (ValueError otherwise, never a fallback)."""
    from .field import field_plan, field_infer
    from .normals import check_channels, field_normals
    if placement is None and scene_aabb is not None:
        raise ValueError("render_field4: scene_aabb belongs to a placement; without one the object is rendered in its own box")
    if placement is not None and occupancy is None:
        raise ValueError("render_field4: placement needs occupancy= (the placed path is the occupancy-culled one): pass "
                         "fixedcull.Occupancy.of(model) for a cuda_ray network or fixedcull.Occupancy.estimate(model) for any other")
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    N, T = rays_o.shape[0], int(num_steps)
    dev = rays_o.device
    if out is None:
        out = torch.empty(N, T, 4, dtype=torch.float32, device=dev)
    assert out.shape == (N, T, 4) and out.dtype == torch.float32 and out.is_contiguous()
    plan = field_plan(model)
    want_normal = check_channels("render_field4", channels, plan)
    if placement is not None:
        from .fixedcull import render_field4_placed
        return render_field4_placed(model, plan, rays_o, rays_d, T, weight_thresh, yolo_details, out, occupancy, placement, scene_aabb, channels)
    if occupancy is not None:
        from .fixedcull import render_field4_culled
        return render_field4_culled(model, plan, rays_o, rays_d, T, weight_thresh, yolo_details, out, occupancy, channels)
    if want_normal and not (plan.infer and model.bg_radius <= 0):
        raise ValueError("render_field4: channels='normal' needs a network the fused inference serves (field_plan(model).infer) without a "
                         "background model")
    if plan.infer and model.bg_radius <= 0:
        aabb = model.aabb_train if model.training else model.aabb_infer
        nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, aabb, model.min_near)
        rb = ray_block_default()
        enc_in, _ = fixed_sample(rays_o, rays_d, nears, fars, aabb, None, T, model.bound, ray_block=rb)
        obj_feat = model.encode_object_feature(yolo_details, dev) if plan.uses_object_feature else None
        if want_normal:
            sigma, rgb = field_normals(model, enc_in)
        else:
            sigma, rgb = field_infer(model, enc_in, rays_d, dir_div=T, dir_block=rb, obj_feat=obj_feat)
        check(lib.foc_fixed_field_pack(ptr(sigma), ptr(rgb), ptr(nears), ptr(fars), None, None, 1.0, N, T, float(model.density_scale),
                                       float(weight_thresh), None, None, None, ptr(out), rb, stream_of(sigma)), "fixed_field_pack")
        return out
    from .combine import pack_field4
    with torch.autocast("cuda", dtype=torch.float16):
        res = model.run(rays_o[None], rays_d[None], yolo_details, num_steps=T, upsample_steps=0, perturb=False, weight_thresh=weight_thresh,
                        return_fields=True)
    out.copy_(pack_field4(res['densities'], res['rgbs']))
    return out
