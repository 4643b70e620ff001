"""torch-ngp's tinycudann network as legacy/nerf/network_tcnn.py builds it (`main_nerf.py --legacy --tcnn`), on the fused kernels: the same
topology, constructor, methods and state_dict as that file running through the tinycudann drop-in (tcnn.py), so checkpoints move between
the two in both directions.

    sigma-net   hash grid 32 -> 64 -> 16                  (tcnn n_hidden_layers = num_layers - 1; trunc_exp on channel 0, 15 geometry features)
    colour-net  [SH16(d) | geo 15 | 1.0] = 32 -> 64 -> 64 -> 16 (n_hidden_layers = num_layers_color - 1), sigmoid

What differs from `network.NeRFNetwork` (whose methods this class inherits):
  * one hidden layer fewer in each network at the same `num_layers` / `num_layers_color`: tcnn counts hidden layers, FFMLP counts
    matrices - 1;
  * column 31 of the colour input is tcnn.PAD_VALUE = 1.0, not 0: a constant input, i.e. a bias for every first-layer neuron. The fused
    kernels take it as `colour_input_pad` (field.FieldPlan), through the *_pad31 twins of the colour-head, field-forward, field-inference,
    occupancy-training and occupancy-render entry points; the plan turns off the paths that write a zero there (head.sample_head);
  * the parameters are tcnn's: one flat fp32 `params` per module (`encoder.params`, `sigma_net.params`, `encoder_dir.params` (empty),
    `color_net.params`) with the layouts of tcnn.py's docstring, and at construction the drop-in's values (its seeded initialisation,
    seed 1337). The modules keep this package's parameter names (`embeddings`, `weights`) inside, which the kernels read; state_dict /
    load_state_dict translate (network_tcnn.py's modules);
  * SH is taken of d itself; the drop-in maps d to (d + 1) / 2 for tcnn and back, SH(2 ((d + 1) / 2) - 1), which rounds differently in
    the last bits;
  * no background model: `bg_radius > 0` is refused at construction, as the reference's command line refuses it for --tcnn
    (main_nerf.py).
"""
import torch

from . import tcnn
from .network import NeRFNetwork as _PlainNetwork
from .network_tcnn import TcnnHashGrid, TcnnMLP, TcnnSH
from .renderer import NeRFRenderer


class NeRFNetwork(_PlainNetwork):
    colour_input_pad = tcnn.PAD_VALUE         # column 31 of the colour input (field.field_plan hands it to the kernels)

    def __init__(self, encoding="HashGrid", encoding_dir="SphericalHarmonics", num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3,
                 hidden_dim_color=64, bound=1, **kwargs):
        if kwargs.get("bg_radius", -1) > 0:
            raise ValueError("network_tcnn_legacy.NeRFNetwork: the background model is not implemented for the tcnn network (bg_radius must be <= 0)")
        NeRFRenderer.__init__(self, bound, **kwargs)            # not network.py's constructor: its FFMLPs count layers the other way
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim

        self.encoder = TcnnHashGrid(bound)                                                       # legacy/nerf/network_tcnn.py:30-41
        self.in_dim = self.encoder.output_dim
        self.sigma_net = TcnnMLP(32, 1 + self.geo_feat_dim, hidden_dim, num_layers - 1)          # :43-53

        self.num_layers_color, self.hidden_dim_color = num_layers_color, hidden_dim_color        # :56-57
        self.encoder_dir = TcnnSH()                                                              # :59-65
        self.in_dim_color = self.encoder_dir.output_dim + self.geo_feat_dim                      # 31, :67
        self.color_net = TcnnMLP(self.in_dim_color, 3, hidden_dim_color, num_layers_color - 1)   # :69-79

    def forward(self, x, d):
        """As network.NeRFNetwork.forward; without autograd the whole-field kernel serves it even though the head kernels do not (they
        write a 0 in column 31), so the occupancy grid's Python inference loop evaluates what the native loop evaluates."""
        from .field import field_plan, field_infer
        if x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled() and not torch.is_grad_enabled() and field_plan(self).infer:
            return field_infer(self, (x + self.bound) / (2 * self.bound), d)
        return super().forward(x, d)

    def _colour_input(self, d, geo_feat):
        pad = geo_feat.new_full(geo_feat.shape[:-1] + (self.color_net.input_dim - self.in_dim_color,), self.colour_input_pad)
        return torch.cat([self.encoder_dir(d).to(geo_feat.dtype), geo_feat, pad], dim=-1)
