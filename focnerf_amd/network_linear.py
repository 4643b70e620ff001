"""torch-ngp's default network (nerf/network.py = legacy/nerf/network.py; `main_nerf.py` without --ff / --tcnn, e.g. `--legacy -O`) with the
reference's parameters — bias-free nn.Linear layers — on the fused kernels:

    sigma-net   hash grid 32 -> 64 -> 16                          (trunc_exp on channel 0, 15 geometry features)
    colour-net  [SH16(d) | geo 15] = 31 -> 64 -> 64 -> 3, sigmoid
    background  (bg_radius > 0) [SH16(d) | 2-D hash grid 4 x 2] = 24 -> 64 -> 3, sigmoid, of the point where the ray leaves the sphere of
                radius bg_radius

Same constructor (legacy/nerf/network.py:11-25 plus the renderer's keywords), sub-module names and order (`encoder`, `sigma_net`,
`encoder_dir`, `color_net`, then `encoder_bg`, `bg_net`), so `state_dict()`, `parameters()` and `get_params()` are the reference's: its
checkpoints load with strict=True both ways, with the trainer's Adam and EMA states, and one seed initialises both to the same values.

On the CPU, without autocast or in fp32 the methods run the reference's torch expressions. Under fp16 autocast on the GPU they run the
fused kernels wherever `field.field_plan` says so: the kernels read FFMLP weight blobs, which `fused_mlp(name)` (ffmlp.PackedMLP) packs
from the layers on every read — the colour input padded from 31 to 32 with a zero column (so the plain entry points serve it, not the
*_pad31 twins), the background input from 24 to 32, each last layer to 16 output rows — and autograd hands each layer its slice of the
blob's gradient. The background model runs as one kernel each way (background.py, csrc/background.hip; plan.background, FOC_FUSED_BG=0
keeps the op chain), and its gradient comes back through the fused nodes (fixedstep._render_tail / _fixed_composite, occtrain._occ_train).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .activation import trunc_exp
from .encoding import get_encoder
from .ffmlp import PackedMLP
from .renderer import NeRFRenderer


def _linears(in_dim, hidden_dim, out_dim, num_layers):
    return nn.ModuleList([nn.Linear(in_dim if l == 0 else hidden_dim, out_dim if l == num_layers - 1 else hidden_dim, bias=False)
                          for l in range(num_layers)])


def _run(layers, h):
    for l, layer in enumerate(layers):
        h = layer(h)
        if l != len(layers) - 1:
            h = F.relu(h, inplace=True)
    return h


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="hashgrid", encoding_dir="sphere_harmonics", encoding_bg="hashgrid", num_layers=2, hidden_dim=64, geo_feat_dim=15,
                 num_layers_color=3, hidden_dim_color=64, num_layers_bg=2, hidden_dim_bg=64, bound=1, n_chunks=None, **kwargs):
        # n_chunks: main_nerf.py passes it in its non-legacy branch, which the reference's nerf/renderer.py does not accept (that branch
        # fails at construction there); taken and ignored, so one import swap serves both branches
        super().__init__(bound, **kwargs)
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.encoder, self.in_dim = get_encoder(encoding, desired_resolution=2048 * bound)
        self.sigma_net = _linears(self.in_dim, hidden_dim, 1 + geo_feat_dim, num_layers)

        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        self.encoder_dir, self.in_dim_dir = get_encoder(encoding_dir)
        self.color_net = _linears(self.in_dim_dir + geo_feat_dim, hidden_dim_color, 3, num_layers_color)

        if self.bg_radius > 0:
            self.num_layers_bg, self.hidden_dim_bg = num_layers_bg, hidden_dim_bg
            self.encoder_bg, self.in_dim_bg = get_encoder(encoding_bg, input_dim=2, num_levels=4, log2_hashmap_size=19, desired_resolution=2048)
            self.bg_net = _linears(self.in_dim_bg + self.in_dim_dir, hidden_dim_bg, 3, num_layers_bg)
        else:
            self.bg_net = None

    # ---- what the fused kernels read (field.fused_mlp)
    def fused_mlp(self, name):
        """The PackedMLP of `sigma_net`, `color_net` or `bg_net`, or None where the layers make no FFMLP (one layer, unequal hidden widths,
        more than 16 outputs, a hidden width the kernels lack): the plan then turns the fused paths off."""
        layers = getattr(self, name, None)
        if not isinstance(layers, nn.ModuleList) or len(layers) < 2:
            return None
        hidden = layers[0].out_features
        if (hidden not in (16, 32, 64, 128, 256) or layers[-1].out_features > 16 or any(l.bias is not None for l in layers)
                or any(l.in_features != hidden for l in layers[1:]) or any(l.out_features != hidden for l in layers[:-1])):
            return None
        return PackedMLP(layers, -(-layers[0].in_features // 16) * 16)

    def _plan(self, x):
        if not (x.is_cuda and torch.is_autocast_enabled()):
            return None
        from .field import field_plan
        return field_plan(self)

    def _geometry_rows(self, x, plan):
        """[M,3] -> [M,16] half: the density network's output through the fused MLP (network.NeRFNetwork._geometry_rows)."""
        from .field import hashgrid_mlp
        sigma = self.fused_mlp("sigma_net")
        if plan.field:
            return hashgrid_mlp(self.encoder, sigma, x, self.bound)
        return sigma.forward_padded(self.encoder(x, bound=self.bound))

    # ---- the reference's methods (legacy/nerf/network.py:95-206)
    def forward(self, x, d):
        plan = self._plan(x)
        if plan is not None and x.dim() == 2 and plan.head:
            from .field import field_infer
            from .head import rgb_head, sample_head
            if not torch.is_grad_enabled() and plan.infer:
                return field_infer(self, (x + self.bound) / (2 * self.bound), d)
            sigma, colour_rows = sample_head(self._geometry_rows(x, plan), d)      # column 31 of the rows is 0: this network's input
            return sigma, rgb_head(self.fused_mlp("color_net").forward_padded(colour_rows))
        field = self.density(x)
        return field['sigma'], self._shade(d, field['geo_feat'])

    def density(self, x):
        plan = self._plan(x)
        if plan is not None and x.dim() == 2 and plan.field:
            h = self._geometry_rows(x, plan)
        else:
            h = _run(self.sigma_net, self.encoder(x, bound=self.bound))
        return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

    def _shade(self, d, geo_feat):
        return torch.sigmoid(_run(self.color_net, torch.cat([self.encoder_dir(d), geo_feat], dim=-1)))

    def background(self, x, d):
        """x [N,2] sphere coordinates in [-1,1], d [N,3] -> rgb [N,3]."""
        plan = self._plan(x)
        if plan is not None and plan.background:
            from .background import background_rgb
            return background_rgb(self, d, coords=x)
        h = self.encoder_bg(x)
        return torch.sigmoid(_run(self.bg_net, torch.cat([self.encoder_dir(d), h], dim=-1)))

    def _background_colour(self, rays_o, rays_d, bg_color):
        """The renderer's background: with the background kernel, sph_from_ray runs inside it (the same arithmetic)."""
        if self.bg_radius > 0:
            plan = self._plan(rays_o)
            if plan is not None and plan.background:
                from .background import background_rgb
                return background_rgb(self, rays_d, rays_o=rays_o, radius=self.bg_radius)
        return super()._background_colour(rays_o, rays_d, bg_color)

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """Colour of the samples selected by `mask` (all if None); the others get 0 (legacy/nerf/network.py:163-192)."""
        if mask is None:
            return self._shade(d, geo_feat)
        rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
        if mask.any():
            rgbs[mask] = self._shade(d[mask], geo_feat[mask]).to(rgbs.dtype)
        return rgbs

    def run(self, rays_o, rays_d, yolo_details=None, fused=False, **kwargs):
        """`fused=True`: the fixed-step path through csrc/fixedstep.hip, with the background kernel when bg_radius > 0 (same image, depth
        and gradients as `NeRFRenderer.run`, which stays the default)."""
        if fused and kwargs.get("upsample_steps", 0) == 0 and (self.bg_radius <= 0 or getattr(self._plan(rays_o), "background", False)):
            from .fixedstep import render_fixed_steps
            kwargs.pop("upsample_steps", None)
            return render_fixed_steps(self, rays_o, rays_d, yolo_details=yolo_details, **kwargs)
        return super().run(rays_o, rays_d, yolo_details, **kwargs)

    def get_params(self, lr):
        """The reference's optimizer groups (legacy/nerf/network.py:194-206)."""
        params = [{'params': m.parameters(), 'lr': lr} for m in (self.encoder, self.sigma_net, self.encoder_dir, self.color_net)]
        if self.bg_radius > 0:
            params += [{'params': self.encoder_bg.parameters(), 'lr': lr}, {'params': self.bg_net.parameters(), 'lr': lr}]
        return params
