"""The background model of torch-ngp's default network (legacy/nerf/network.py:145-160) as one kernel each way (csrc/background.hip):

    rgb = background_rgb(model, rays_d, rays_o=o, radius=R)      # == model.background(sph_from_ray(o, d, R), d) under fp16 autocast
    rgb = background_rgb(model, rays_d, coords=x)                # == model.background(x, d)

for a network whose `field.field_plan(model).background` holds (network_linear.py with bg_radius > 0). The result is [N,3] fp16, as the op
path's sigmoid under autocast. Gradients reach `encoder_bg.embeddings` (fp32, accumulated with fp32 atomics) and the bg_net blob (fp32,
fixed-order sums), from which autograd hands each nn.Linear layer its slice; the rays and coordinates take none.
"""
import torch
from torch.autograd import Function

from ._lib import lib, ptr, stream_of, check


class _background(Function):
    @staticmethod
    def forward(ctx, emb, blob, rays_o, rays_d, coords, radius, offsets, grid):
        from .field import _half_of
        rays_d = rays_d.contiguous().float()
        N = rays_d.shape[0]
        w16 = _half_of(blob)
        emb = emb.contiguous()
        assert emb.dtype == torch.float32 and emb.dim() == 2 and emb.shape[1] == 2 and offsets.numel() == 5 and w16.numel() == 64 * 32 + 16 * 64
        rgb = torch.empty(N, 3, dtype=torch.float16, device=rays_d.device)
        check(lib.foc_background_forward(ptr(rays_o), ptr(rays_d), ptr(coords), float(radius), N, ptr(emb), ptr(offsets), float(grid.log2_scale),
                                         int(grid.base_resolution), ptr(w16), ptr(rgb), stream_of(rays_d)), "background_forward")
        empty = torch.empty(0, device=rays_d.device)
        ctx.save_for_backward(emb, w16, rays_o if rays_o is not None else empty, rays_d, coords if coords is not None else empty, offsets)
        ctx.cfg = (N, float(radius), grid, rays_o is not None, coords is not None)
        return rgb

    @staticmethod
    def backward(ctx, g_rgb):
        from .backend import _scratch
        emb, w16, rays_o, rays_d, coords, offsets = ctx.saved_tensors
        N, radius, grid, has_o, has_coords = ctx.cfg
        dev = rays_d.device
        g_rgb = g_rgb.contiguous().half()
        g_emb = torch.zeros_like(emb) if ctx.needs_input_grad[0] else None
        g_w = torch.empty(w16.numel(), dtype=torch.float32, device=dev)
        ws = _scratch.get("background_ws", lib.foc_background_backward_workspace_bytes(N), dev)
        g_emb_buf = g_emb if g_emb is not None else torch.zeros_like(emb)
        check(lib.foc_background_backward(ptr(g_rgb), ptr(rays_o if has_o else None), ptr(rays_d), ptr(coords if has_coords else None), radius, N,
                                          ptr(emb), ptr(offsets), float(grid.log2_scale), int(grid.base_resolution), ptr(w16), ptr(g_emb_buf),
                                          ptr(g_w), ptr(ws), ws.numel(), stream_of(rays_d)), "background_backward")
        return g_emb, g_w if ctx.needs_input_grad[1] else None, None, None, None, None, None, None


def background_rgb(model, rays_d, rays_o=None, radius=None, coords=None):
    """rays_d [N,3] with either coords [N,2] (the sphere coordinates in [-1,1]) or rays_o [N,3] and the sphere's radius -> rgb [N,3] fp16."""
    from .field import fused_mlp
    enc = model.encoder_bg
    rays_d = rays_d.reshape(-1, 3)
    if coords is not None:
        coords = coords.reshape(-1, 2).contiguous().float()
        rays_o, radius = None, 0.0
    else:
        rays_o = rays_o.reshape(-1, 3).contiguous().float()
    return _background.apply(enc.embeddings, fused_mlp(model, "bg_net").weights, rays_o, rays_d, coords, float(radius), enc.offsets, enc.spec())
