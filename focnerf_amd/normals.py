"""Surface normals of the density field, n = -grad(sigma) / |grad(sigma)|, without autograd: csrc/normals.hip (`foc_field_normals`) computes
sigma, the position gradient of the density logit and the encoded normal per sample in one launch.

    sigma, grad = density_gradient(model, x)                 # world units; fused where field_plan(model).normals, else through autograd
    sigma, normal_rgb = field_normals(model, xn, rotation)   # the drop-in counterpart of field.field_infer: "rgb" = 0.5 + 0.5 n
    normal, opacity, encoded = render_normals(model, rays_o, rays_d)                       # 512 fixed steps per ray
    normal, opacity, encoded = render_normals(model, rays_o, rays_d, path="occupancy")     # the occupancy march's own samples

A normal encoded as 0.5 + 0.5 n is an ordinary colour to everything behind the field: `render_field4(..., channels="normal")`,
`fixedcull.culled_lists`, `combine.placed_field_fns`, `culled_field_fns` and `render_scene_culled` take `channels="normal"` and the packs,
the combiner, attribution and the exchange between ranks carry it unchanged. `decode_normal_map` turns the combiner's pair of images for
the backgrounds (1, 0) back into unit normals.
"""
import math

import numpy as np
import torch

from ._lib import lib, check, ptr, stream_of, FOC_F16

_CHANNELS = ("rgb", "normal")
_GRAD_CLAMP = 15.0                       # activation.py: trunc_exp's derivative is taken at the logit clamped to [-15, 15]


def check_channels(who, channels, plan=None):
    """`channels` is "rgb" or "normal"; "normal" needs a network the fused kernel serves (ValueError: never a silent fallback)."""
    if channels not in _CHANNELS:
        raise ValueError(f"{who}: channels must be 'rgb' or 'normal', got {channels!r}")
    if channels == "normal" and plan is not None and not plan.normals:
        raise ValueError(f"{who}: channels='normal' needs a network the fused normals kernel serves (field_plan(model).normals: fp16-able "
                         "hash grid with 16 levels of 2 features, linear, align_corners off; sigma network 32 -> 64 x 1..3 -> 16 with ReLU; "
                         "FOC_FUSED_NORMALS not 0); density_gradient() serves the others through autograd")
    return channels == "normal"


def rotation_tensor(rotation, device):
    """None, or the row-major 3x3 (object -> scene) as the kernel reads it: 9 fp32 on the device, rounded once from float64."""
    if rotation is None:
        return None
    if torch.is_tensor(rotation):
        R = rotation.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
    else:
        R = torch.from_numpy(np.asarray(rotation, dtype=np.float64).astype(np.float32).reshape(-1).copy()).to(device)
    if R.numel() != 9:
        raise ValueError(f"rotation must be 3x3, got {R.numel()} values")
    return R


def _launch(model, xn, rot, want_sigma=True, want_grad=False, want_rgb=False, want_enc=False):
    """`foc_field_normals` on xn [M,3] fp32 in [0,1] -> (sigma, grad_raw, normal_rgb, grad_enc), None where not asked for."""
    from .field import fused_mlp, _half_of
    enc, sn = model.encoder, fused_mlp(model, "sigma_net")
    grid = enc.spec()
    xn = xn.contiguous().float()
    M, dev = xn.shape[0], xn.device
    L = enc.offsets.shape[0] - 1
    emb, ws = _half_of(enc.embeddings), _half_of(sn.weights)
    gridtype, align_corners, interp = grid.tail()
    sigma = torch.empty(M, dtype=torch.float32, device=dev) if want_sigma else None
    grad_raw = torch.empty(M, 3, dtype=torch.float32, device=dev) if want_grad else None
    rgb = torch.empty(M, 3, dtype=torch.float32, device=dev) if want_rgb else None
    genc = torch.empty(M, 32, dtype=torch.float32, device=dev) if want_enc else None
    check(lib.foc_field_normals(ptr(xn), M, ptr(emb), ptr(enc.offsets), 3, int(enc.level_dim), L, float(grid.log2_scale), int(grid.base_resolution),
                                int(gridtype), int(align_corners), int(interp), FOC_F16, None, ptr(ws), int(sn.num_layers), int(sn.hidden_dim),
                                int(sn.activation), ptr(rot), ptr(sigma), ptr(grad_raw), ptr(rgb), ptr(genc), stream_of(xn)), "field_normals")
    return sigma, grad_raw, rgb, genc


@torch.no_grad()
def field_normals(model, xn, rotation=None):
    """xn [M,3] fp32 in [0,1] (already normalised) -> sigma [M] fp32 (the bits of `field.field_infer`'s), normal_rgb [M,3] fp32 =
    0.5 + 0.5 (rotation @) n. rotation: None or a 3x3 object -> scene rotation. Same half-cache scope for table and weights as field_infer.
    ValueError when `field_plan(model).normals` does not hold."""
    from .field import field_plan
    check_channels("field_normals", "normal", field_plan(model))
    sigma, _, rgb, _ = _launch(model, xn.view(-1, 3), rotation_tensor(rotation, xn.device), want_rgb=True)
    return sigma, rgb


def _autograd_gradient(model, x):
    """The fallback: torch.autograd.grad through the encoder (GridEncoder's general forward with dy_dx) and the sigma network, on a detached
    copy, under enable_grad. An FFMLP-shaped sigma network runs its training forward whatever the module's mode (the inference forward
    keeps nothing for a backward)."""
    from .activation import trunc_exp
    from .ffmlp import FFMLP, PackedMLP, ffmlp_forward
    from .field import fused_mlp
    with torch.enable_grad():
        xs = x.detach().clone().float().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=xs.is_cuda):
            enc = model.encoder(xs, bound=model.bound)
            mlp = fused_mlp(model, "sigma_net")
            if isinstance(mlp, (FFMLP, PackedMLP)) and enc.shape[-1] == mlp.input_dim:
                h = ffmlp_forward(enc, mlp.weights, mlp.input_dim, mlp.padded_output_dim, mlp.hidden_dim, mlp.num_layers, mlp.activation,
                                  mlp.output_activation, False, True)
            else:
                h = model.sigma_net(enc)
            sigma = trunc_exp(h[..., 0]).float()
        (grad,) = torch.autograd.grad(sigma.sum(), xs)
    return sigma.detach(), grad.detach().float()


def density_gradient(model, x):
    """x [...,3] in world units -> sigma [...] fp32 as `model.density(x)['sigma']` gives it, grad [...,3] fp32 = d sigma / d x.
    Fused (`field_plan(model).normals`): sigma' * grad_raw / (2 bound) with grad_raw from the kernel (no autograd, runs under no_grad) and
    sigma' = trunc_exp's derivative, exp of the logit clamped to [-15, 15] (activation.py). Otherwise the autograd route through
    GridEncoder's dy_dx and the FFMLP backward, whose input gradient is rounded to half."""
    from .field import field_plan
    prefix = list(x.shape[:-1])
    flat = x.reshape(-1, 3)
    if field_plan(model).normals and flat.is_cuda:
        with torch.no_grad():
            bound = float(model.bound)
            xn = (flat.float() + bound) / (2 * bound)
            sigma, grad_raw, _, _ = _launch(model, xn, None, want_grad=True)
            slope = sigma.clamp(min=math.exp(-_GRAD_CLAMP), max=math.exp(_GRAD_CLAMP))
            grad = slope[:, None] * grad_raw / (2 * bound)
    else:
        sigma, grad = _autograd_gradient(model, flat)
    return sigma.view(prefix), grad.view(prefix + [3])


def decode_normal_map(image4_pair):
    """The combiner's image4 [2,N,4] for the backgrounds (1.0, 0.0) of a `channels="normal"` render -> (normal [N,3], opacity [N]):
    opacity = 1 - (white.r - black.r) and sum_k w_k n_k = 2 black.rgb - opacity; the normal is that sum at unit length where opacity > 0
    and the sum is not zero, else 0. One approximation: samples whose own weight is <= weight_thresh are packed as rgb 0, not 0.5 (an
    encoded zero normal), so each moves the sum by at most its weight <= T * weight_thresh in all."""
    if image4_pair.dim() != 3 or image4_pair.shape[0] != 2 or image4_pair.shape[2] < 3:
        raise ValueError(f"decode_normal_map: the combiner's [2,N,4] for backgrounds (1, 0) expected, got {tuple(image4_pair.shape)}")
    white, black = image4_pair[0].double(), image4_pair[1].double()
    opacity = 1.0 - (white[:, 0] - black[:, 0])
    s = 2.0 * black[:, :3] - opacity[:, None]
    length = s.norm(dim=-1)
    ok = (opacity > 0) & (length > 0)
    normal = torch.where(ok[:, None], s / length.clamp_min(1e-300)[:, None], torch.zeros_like(s))
    return normal.float(), opacity.float()


def normal_map_finish(normal_acc, weights_sum):
    """The composite's accumulators of an encoded-normal payload -> (normal [N,3], unit or 0; normal_rgb [N,3], the encoded map on a white
    background): `foc_normal_map_finish`, one launch. normal_acc [N,3] = sum_k w_k (0.5 + 0.5 n_k), weights_sum [N], fp32 on the GPU."""
    acc, ws = normal_acc.contiguous().view(-1, 3), weights_sum.contiguous().view(-1)
    if acc.dtype != torch.float32 or ws.dtype != torch.float32 or not acc.is_cuda or acc.shape[0] != ws.shape[0]:
        raise ValueError(f"normal_map_finish: fp32 GPU tensors [N,3] and [N] expected, got {tuple(normal_acc.shape)} {normal_acc.dtype} and "
                         f"{tuple(weights_sum.shape)} {weights_sum.dtype} on {normal_acc.device}")
    normal, encoded = torch.empty_like(acc), torch.empty_like(acc)
    check(lib.foc_normal_map_finish(ptr(acc), ptr(ws), acc.shape[0], ptr(normal), ptr(encoded), stream_of(acc)), "normal_map_finish")
    return normal, encoded


@torch.no_grad()
def render_normals(model, rays_o, rays_d, num_steps=512, occupancy=None, placement=None, scene_aabb=None, path="fixed"):
    """A normal map of one object: `render_field4(channels="normal")`, the fixed-step composite against the backgrounds (1, 0) and
    `decode_normal_map`. -> normal [N,3] (unit or 0), opacity [N], encoded [N,3] (the 0.5 + 0.5 n image on the white background).
    path="occupancy": the same triple from the occupancy march instead (`model.run_cuda(normals="only")` with dt_gamma 0, max_steps 1024,
    T_thresh 1e-4; under autocast, as a colour view is rendered): the samples a colour view of the object takes, not num_steps per ray.
    One object in its own frame: `occupancy=` / `placement=` raise with it (placed scenes stay on the fixed-step combiner)."""
    if path not in ("fixed", "occupancy"):
        raise ValueError(f"render_normals: path must be 'fixed' or 'occupancy', got {path!r}")
    if path == "occupancy":
        if occupancy is not None or placement is not None:
            raise ValueError("render_normals: path='occupancy' renders one object in its own frame through its own occupancy grid; "
                             "occupancy= / placement= belong to path='fixed'")
        if not getattr(model, "cuda_ray", False):
            raise ValueError("render_normals: path='occupancy' needs a model built with cuda_ray=True (an occupancy grid to march)")
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        with torch.autocast("cuda", dtype=torch.float16):
            out = model.run_cuda(rays_o, rays_d, dt_gamma=0, max_steps=1024, T_thresh=1e-4, normals="only")
        return out["normal"], out["weights_sum"], out["normal_rgb"]
    from . import raymarching
    from .combine import combine_packed
    from .fixedstep import render_field4
    from .fixedcull import _scene_box
    rays_o = rays_o.contiguous().view(-1, 3).float()
    rays_d = rays_d.contiguous().view(-1, 3).float()
    field4 = render_field4(model, rays_o, rays_d, num_steps=num_steps, occupancy=occupancy, placement=placement, scene_aabb=scene_aabb, channels="normal")
    box = _scene_box(scene_aabb, model, rays_o.device) if placement is not None else (model.aabb_train if model.training else model.aabb_infer)
    nears, fars = raymarching.near_far_from_aabb(rays_o, rays_d, box, model.min_near)
    image4 = combine_packed([field4], nears, fars, bgs=(1.0, 0.0))[0]
    normal, opacity = decode_normal_map(image4)
    return normal, opacity, image4[0, :, :3].contiguous()
