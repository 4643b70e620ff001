"""FOC's network as nerf/network_tcnn.py:451-681 builds it on tinycudann, on the fused kernels: the same topology, constructor, methods and
state_dict as that file running through the tinycudann drop-in (tcnn.py), so checkpoints move between the two in both directions.

    sigma-net   hash grid 32 -> 64 -> 16                   (tcnn n_hidden_layers = num_layers - 1; trunc_exp on channel 0, 15 geometry features)
    yolo_feat_encoder   144 -> 16 (ReLU) -> 16, no biases   (one vector per image)
    colour-net  [SH16(d) | geo 15 | encoded object feature 16 | 1.0] = 48 -> 64 -> 64 -> 16 (n_hidden_layers = num_layers_color - 1), sigmoid

What differs from `network_foc.NeRFNetwork` (whose methods this class inherits):
  * one hidden layer fewer in the sigma network at the same `num_layers`: tcnn counts hidden layers, FFMLP counts matrices - 1;
  * column 47 of the colour input is tcnn.PAD_VALUE = 1.0, not 0: a constant input, i.e. a bias for every first-layer neuron. The fused
    kernels take it as `colour_input_pad` (field.FieldPlan), through the *_pad twins of the colour-head, field-forward and field-inference
    entry points; the plan turns off the paths that write a zero there (head.sample_head);
  * the parameters are tcnn's: one flat fp32 `params` per module (`encoder.params`, `sigma_net.params`, `yolo_feat_encoder.params`,
    `encoder_dir.params` (empty), `color_net.params`) with the layouts of tcnn.py's docstring, and at construction the drop-in's values
    (its seeded initialisation, seed 1337). The modules keep this package's parameter names (`embeddings`, `weights`) inside, which the
    kernels read; state_dict / load_state_dict translate;
  * SH is taken of d itself; the drop-in maps d to (d + 1) / 2 for tcnn and back, SH(2 ((d + 1) / 2) - 1), which rounds differently in
    the last bits.
"""
import numpy as np
import torch
import torch.nn as nn

from . import tcnn
from .ffmlp import FFMLP
from .gridencoder import GridEncoder
from .network_foc import NeRFNetwork as _FocNetwork, _tiny_mlp_vec
from .renderer import NeRFRenderer
from .shencoder import SHEncoder

SEED = 1337                          # tcnn's default seed (tcnn.Encoding / tcnn.Network)


def _mlp_config(n_neurons, n_hidden_layers):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": n_neurons,
            "n_hidden_layers": n_hidden_layers}


def _as_tcnn_params(name):
    """A state_dict hook that stores the parameter `name` as tcnn's flat `params`."""
    def hook(module, state_dict, prefix, local_metadata):
        state_dict[prefix + "params"] = state_dict.pop(prefix + name).reshape(-1)
    return hook


def _from_tcnn_params(name, shape):
    """A load_state_dict pre-hook that reads tcnn's `params` into the parameter `name` (of `shape`); a wrong size is left for load_state_dict
    to report."""
    def hook(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        if prefix + "params" in state_dict:
            v = state_dict.pop(prefix + "params")
            state_dict[prefix + name] = v.view(shape()) if v.numel() == int(np.prod(shape())) else v
    return hook


class TcnnHashGrid(GridEncoder):
    """tcnn.Encoding(3, HashGrid: 16 levels x 2 features, 2^19 rows, base 16, FOC's per_level_scale) as a GridEncoder: the same table,
    kept as `embeddings` [rows, 2] for the kernels and saved as `params` [rows * 2]; the level offsets are not saved (tcnn saves none)."""

    def __init__(self, bound, seed=SEED):
        per_level_scale = float(np.exp2(np.log2(2048 * bound / 16) / (16 - 1)))         # network_tcnn.py:476
        super().__init__(input_dim=3, num_levels=16, level_dim=2, per_level_scale=per_level_scale, base_resolution=16, log2_hashmap_size=19,
                         gridtype='hash', align_corners=False)
        offsets = self.offsets
        del self.offsets
        self.register_buffer('offsets', offsets, persistent=False)
        with torch.no_grad():                                                               # tcnn.py's U(-1e-4, 1e-4) draw
            self.embeddings.copy_(torch.empty(self.n_params).uniform_(-1e-4, 1e-4, generator=torch.Generator().manual_seed(seed)).view_as(self.embeddings))
        self._register_state_dict_hook(_as_tcnn_params('embeddings'))
        self.register_load_state_dict_pre_hook(_from_tcnn_params('embeddings', lambda: tuple(self.embeddings.shape)))


class TcnnMLP(FFMLP):
    """tcnn.Network(FullyFusedMLP, ReLU) as an FFMLP, one hidden layer allowed: `num_layers` is tcnn's n_hidden_layers, the input is padded
    to a multiple of 16 (the caller writes the pad columns), the blob is saved as `params`."""
    min_layers = 1

    def __init__(self, n_input_dims, n_output_dims, n_neurons, n_hidden_layers, seed=SEED):
        spec = tcnn._MlpSpec(n_input_dims, n_output_dims, _mlp_config(n_neurons, n_hidden_layers))
        super().__init__(spec.in_pad, n_output_dims, n_neurons, n_hidden_layers)
        self.n_input_dims = int(n_input_dims)
        with torch.no_grad():
            self.weights.copy_(spec.init(torch.Generator().manual_seed(seed)))
        self._register_state_dict_hook(_as_tcnn_params('weights'))
        self.register_load_state_dict_pre_hook(_from_tcnn_params('weights', lambda: tuple(self.weights.shape)))


class TcnnSH(SHEncoder):
    """tcnn.Encoding(3, SphericalHarmonics degree 4): no parameters, but an empty `params` as tcnn has. Takes d in [-1, 1] (not (d + 1) / 2)."""

    def __init__(self):
        super().__init__(3, 4)
        self.params = nn.Parameter(torch.empty(0))


class TcnnObjectEncoder(nn.Module):
    """tcnn.Network(n_in, n_out, FullyFusedMLP, 16 neurons, one hidden layer): W1 relu(W0 [x | 1.0 pad]), no biases, fp32. `params` is the
    blob [16 x padded n_in] | [16 x 16]; the one-vector GPU case runs as two matrix-vector products (network_foc._tiny_mlp_vec)."""

    def __init__(self, n_input_dims, n_output_dims, seed=SEED):
        super().__init__()
        spec = tcnn._MlpSpec(n_input_dims, n_output_dims, _mlp_config(16, 1))
        self.n_input_dims, self.n_output_dims, self.in_pad = int(n_input_dims), int(n_output_dims), spec.in_pad
        self.params = nn.Parameter(spec.init(torch.Generator().manual_seed(seed)))

    def forward(self, x):
        if self.in_pad != self.n_input_dims:
            x = torch.cat([x, x.new_full(x.shape[:-1] + (self.in_pad - self.n_input_dims,), tcnn.PAD_VALUE)], dim=-1)
        n0 = 16 * self.in_pad
        w0, w1 = self.params[:n0].view(16, self.in_pad), self.params[n0:].view(16, 16)
        if x.dim() == 2 and x.shape[0] == 1 and x.is_cuda:
            with torch.autocast("cuda", enabled=False):
                y = _tiny_mlp_vec.apply(x[0].float(), w0, w1).unsqueeze(0)
        else:
            y = torch.relu(x.to(w0.dtype) @ w0.t()) @ w1.t()
        return y[..., :self.n_output_dims]


class NeRFNetwork(_FocNetwork):
    colour_input_pad = tcnn.PAD_VALUE         # column 47 of the colour input (field.field_plan hands it to the kernels)

    def __init__(self, encoding="HashGrid", encoding_dir="SphericalHarmonics", num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3,
                 hidden_dim_color=64, yolo_encoding_dim=16, bound=1, n_chunks=5, yolo_feats_encoder_dim=144, **kwargs):
        NeRFRenderer.__init__(self, bound, **kwargs)            # not network_foc's constructor: its FFMLPs count layers the other way
        self.num_layers, self.hidden_dim, self.geo_feat_dim = num_layers, hidden_dim, geo_feat_dim
        self.yolo_encoding_dim, self.yolo_feats_encoder_dim, self.n_chunks = yolo_encoding_dim, yolo_feats_encoder_dim, n_chunks

        self.encoder = TcnnHashGrid(bound)                                                           # :476-488
        self.in_dim = self.encoder.output_dim
        self.sigma_net = TcnnMLP(self.in_dim, 1 + self.geo_feat_dim, hidden_dim, num_layers - 1)     # :490-500
        self.yolo_feat_encoder = self.get_yolo_feat_encoder(yolo_feats_encoder_dim)                 # :502-514

        self.num_layers_color = 2                                                                   # :517 (the attribute; the net uses the argument)
        self.hidden_dim_color = 64
        self.encoder_dir = TcnnSH()                                                                 # :520-526
        self.in_dim_color = self.encoder_dir.output_dim + self.geo_feat_dim                         # 31, :528
        self.color_in = self.in_dim_color + self.yolo_encoding_dim                                  # 47
        self.color_in_padded = (self.color_in + 15) // 16 * 16                                      # 48
        self.color_net = TcnnMLP(self.color_in, 3, hidden_dim_color, num_layers_color - 1)          # :533-543

    def get_yolo_feat_encoder(self, yolo_feats_encoder_dim):
        return TcnnObjectEncoder(yolo_feats_encoder_dim, self.yolo_encoding_dim)

    def forward(self, x, d, yolo_details=None):
        """As network_foc's. With an encoded object feature and without autograd the whole-field kernel serves it even though the head
        kernels do not (they write a 0 in column 47), so the occupancy grid's Python inference loop evaluates what the native loop
        evaluates (network_tcnn_legacy.py does the same); without a feature the call is what it always was.
        This holds for any direct `net(x, d, (_, _, obj16))` call under no_grad and autocast, on a `cuda_ray=False` model too (the renderer's
        fixed-step path never makes one): such a call now returns the whole-field kernel's values, which agree with the torch colour path
        it ran before within the fp16 bound of the other whole-field comparisons (tests/test_gpu_occ_object.py), not bit for bit."""
        if yolo_details is not None and x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled() and not torch.is_grad_enabled():
            from .field import field_plan, field_infer
            obj = torch.as_tensor(yolo_details[2], device=x.device)
            if obj.numel() == self.yolo_encoding_dim and field_plan(self).infer:
                return field_infer(self, (x + self.bound) / (2 * self.bound), d, obj_feat=obj)
        return super().forward(x, d, yolo_details)

    def _color_torch(self, d, geo_feat, obj_feat):
        d = self.encoder_dir(d)
        obj = obj_feat.to(geo_feat.dtype)
        if obj.dim() == 1:
            obj = obj.unsqueeze(0).expand(geo_feat.shape[0], -1)
        pad = geo_feat.new_full((geo_feat.shape[0], self.color_in_padded - self.color_in), self.colour_input_pad)
        h = torch.cat([d.to(geo_feat.dtype), geo_feat, obj, pad], dim=-1)
        return torch.sigmoid(self.color_net(h))
