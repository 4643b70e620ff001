"""The NeRF field FOC trains per object: hash-grid encoder -> density MLP -> (direction encoding, geometry features) -> colour MLP.

Same constructor arguments, sub-module names (`encoder`, `sigma_net`, `encoder_dir`, `color_net` — hence the same state_dict keys),
methods (`forward`, `density`, `color`, `get_params`) and numerics as the reference's nerf/network_ff.py:10-148:
    h     = sigma_net(encoder(x))                     32 -> 64 -> 64 -> 16
    sigma = trunc_exp(h[:, 0]);  geo = h[:, 1:16]
    rgb   = sigmoid(color_net([SH16(d) | geo | 0]))    32 -> 64 -> 64 -> 64 -> 3 (padded to 16)
The reference file itself cannot be constructed from its own tree (it imports an `encoding` module the tree lacks); with
focnerf_amd/dropin on PYTHONPATH it can (tests/test_dropin.py).

Under fp16 autocast on flat [M,3] GPU inputs the glue between the kernels (trunc_exp, SH, concatenation + padding, sigmoid) runs as
fused kernels too (csrc/head.hip; FOC_FUSED_HEAD=0 keeps the torch expressions; `field.field_plan` says which apply), and without autograd the whole field is one kernel
after the encoder (csrc/ffmlp.hip, k_nerf_infer).
"""
import torch

from .activation import trunc_exp
from .encoding import get_encoder
from .ffmlp import FFMLP
from .renderer import NeRFRenderer


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="hashgrid", encoding_dir="sphere_harmonics", num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3,
                 hidden_dim_color=64, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color
        # density branch: finest level of the grid resolves 1/2048 of a unit box whatever the bound
        self.encoder, self.in_dim = get_encoder(encoding, desired_resolution=2048 * bound)
        self.sigma_net = FFMLP(self.in_dim, 1 + geo_feat_dim, hidden_dim, num_layers)
        # colour branch: direction encoding + geometry features, one zero column to reach a multiple of 16 (network_ff.py:44)
        self.encoder_dir, dir_width = get_encoder(encoding_dir)
        self.in_dim_color = dir_width + geo_feat_dim + 1
        self.color_net = FFMLP(self.in_dim_color, 3, hidden_dim_color, num_layers_color)

    # ---- torch expressions (any dtype / device / shape)
    def _colour_input(self, d, geo_feat):
        return torch.cat([self.encoder_dir(d).to(geo_feat.dtype), geo_feat, torch.zeros_like(geo_feat[..., :1])], dim=-1)

    def _shade(self, d, geo_feat):
        return torch.sigmoid(self.color_net(self._colour_input(d, geo_feat)))

    # ---- fused kernels (field.field_plan: which ones serve this network)
    def _geometry_rows(self, x, plan):
        """[M,3] -> [M,16] half: the density network's padded output, the encoding kept in the encoder's [L,B,C] planes when possible."""
        from .field import hashgrid_mlp
        if plan.field:
            return hashgrid_mlp(self.encoder, self.sigma_net, x, self.bound)
        return self.sigma_net.forward_padded(self.encoder(x, bound=self.bound))

    def forward(self, x, d):
        """positions x in [-bound, bound]^3 and unit directions d -> (sigma [...], rgb [..., 3])."""
        from .field import field_plan
        plan = field_plan(self)
        if not (x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled() and plan.head):
            field = self.density(x)
            return field['sigma'], self._shade(d, field['geo_feat'])
        from .field import field_infer
        from .head import rgb_head, sample_head
        if not torch.is_grad_enabled() and plan.infer:
            return field_infer(self, (x + self.bound) / (2 * self.bound), d)
        sigma, colour_rows = sample_head(self._geometry_rows(x, plan), d)
        return sigma, rgb_head(self.color_net.forward_padded(colour_rows))

    def density(self, x):
        from .field import field_plan
        plan = field_plan(self)
        if x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled() and plan.field:
            h = self._geometry_rows(x, plan)
        else:
            h = self.sigma_net(self.encoder(x, bound=self.bound))
        return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """Colour of the samples selected by `mask` (all if None); the others get 0 — what `run()` asks for (network_ff.py:95-134)."""
        if mask is None:
            return self._shade(d, geo_feat)
        rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
        if mask.any():
            rgbs[mask] = self._shade(d[mask], geo_feat[mask]).to(rgbs.dtype)
        return rgbs

    def run(self, rays_o, rays_d, yolo_details=None, fused=False, **kwargs):
        """`fused=True`: the fixed-step path through csrc/fixedstep.hip (same image, depth and gradients as `NeRFRenderer.run`, which
        stays the default). Keywords go through to either: `distortion=True` adds results['distortion'] on both routes."""
        if fused and kwargs.get("upsample_steps", 0) == 0 and self.bg_radius <= 0:
            from .fixedstep import render_fixed_steps
            kwargs.pop("upsample_steps", None)
            return render_fixed_steps(self, rays_o, rays_d, yolo_details=yolo_details, **kwargs)
        return super().run(rays_o, rays_d, yolo_details, **kwargs)

    def get_params(self, lr):
        """One optimizer group per sub-module, as the reference trainer expects (network_ff.py:137-148)."""
        return [{'params': m.parameters(), 'lr': lr} for m in (self.encoder, self.sigma_net, self.encoder_dir, self.color_net)]
