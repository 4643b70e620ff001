"""Drop-in for tiny-cuda-nn's PyTorch bindings (`import tinycudann as tcnn`), on this package's kernels.

FOC's own networks (nerf/network_tcnn.py, legacy/nerf/network_tcnn.py of the reference) build everything from three classes; this module
provides them, written from tcnn's public interface and the configs those two files pass:

  * Encoding(n_input_dims, encoding_config, seed=1337, dtype=None)
      "HashGrid" / "TiledGrid" / "Grid" (type "Hash" or "Tiled"): n_levels, n_features_per_level, log2_hashmap_size, base_resolution,
          per_level_scale, interpolation "Linear" | "Smoothstep". Served by `grid_encode` (csrc/gridencoder.hip: counted forward, binned
          backward where GridEncoder gets them) on the table layout of this package's GridEncoder (gridencoder.level_offsets).
          Inputs are in [0, 1] — no `bound` mapping; a coordinate outside [0, 1] encodes to zeros (what this package's encoder returns).
      "SphericalHarmonics" degree 4 (n_input_dims 3): inputs in [0, 1] are mapped to 2 x - 1 and encoded with the degree-4 basis of
          shencoder.py (one HIP kernel when no input gradient is wanted).
      The result has `dtype` (default half); the hash table is read as fp16 when dtype is half.
  * Network(n_input_dims, n_output_dims, network_config, seed=1337)
      otype "FullyFusedMLP", activation "ReLU" | "None", output_activation "None", n_neurons 16 / 32 / 64 / 128, n_hidden_layers >= 1,
      n_output_dims <= 16. Served by the fused MLP kernels (csrc/ffmlp.hip; one hidden layer is their num_layers = 1). Inputs of any dtype
      are cast to half and padded with PAD_VALUE columns to a multiple of 16; the output is half, [..., n_output_dims].
  * NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding_config, network_config, seed=1337): the two above in one module.

Every module holds ONE flat fp32 nn.Parameter named `params` (state_dict keys `encoder.params`, `sigma_net.params`, ... as with tcnn);
a parameter-free encoding holds an empty one. Construction runs on the CPU (the reference builds the model before moving it); a
configuration the kernels cannot serve is refused there, with the reason, never at launch.

Parameter layout and initialisation:
  * grid: the table rows of gridencoder.level_offsets x n_features_per_level, row-major; U(-1e-4, 1e-4);
  * MLP: the fused MLP's weight blob, [n_neurons x padded_input] | (n_hidden_layers - 1) x [n_neurons x n_neurons] |
    [16 x n_neurons], every matrix row-major with the output neuron as the row; each matrix Xavier-uniform, U(+-sqrt(6 / (fan_in +
    fan_out))) with the padded widths, drawn in that order from a torch.Generator seeded with `seed`;
  * NetworkWithInputEncoding: the network's parameters first, then the encoding's.

UNPINNED (tinycudann does not run on this platform): tcnn's own arithmetic (its hash function, level resolutions and
table sizes, fp16 accumulation), its parameter layout and its initialisation are ASSUMED, not verified. The parameter COUNTS follow the
published formulas (for the networks FOC builds they are tcnn's), but checkpoints trained with NVIDIA tcnn are not supported: an MLP
`params` of the same size has a different layout, and a grid table a different hash. PAD_VALUE = 1.0 is what tcnn is believed to pad
network inputs with (a constant input column acts as a free bias); it is pinned by tests/test_gpu_tcnn.py, not checked against tcnn.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from ._autograd import rows, unrows
from .ffmlp import ACTIVATIONS, NO_ACTIVATION, FusedMLP
from .gridencoder import GRID_TYPES, INTERPOLATIONS, grid_encode, level_offsets
from .shencoder import SHEncoder

PAD_VALUE = 1.0                      # network input columns past n_input_dims
MLP_NEURONS = (16, 32, 64, 128)      # tcnn's FullyFusedMLP widths (hidden 256 of ffmlp_wide.hip is not one of them)
MAX_HIDDEN_LAYERS = 16               # the fused MLP's C ABI limit
_LDS_BYTES = 160 * 1024


def _name(v):
    return "none" if v is None else str(v).lower()


class _GridSpec:
    def __init__(self, n_input_dims, cfg):
        otype = cfg["otype"]
        kind = {"hashgrid": "hash", "tiledgrid": "tiled"}.get(otype.lower())
        if kind is None:
            kind = _name(cfg.get("type", "Hash"))
            if kind not in GRID_TYPES:
                raise ValueError(f"tinycudann drop-in: Grid type {cfg.get('type')!r} is not supported (Hash or Tiled)")
        self.gridtype = GRID_TYPES[kind]
        self.n_levels = int(cfg.get("n_levels", 16))
        self.n_features = int(cfg.get("n_features_per_level", 2))
        self.log2_hashmap_size = int(cfg.get("log2_hashmap_size", 19))
        self.base_resolution = int(cfg.get("base_resolution", 16))
        self.per_level_scale = float(cfg.get("per_level_scale", 2.0))
        interp = _name(cfg.get("interpolation", "Linear"))
        if interp not in INTERPOLATIONS:
            raise ValueError(f"tinycudann drop-in: grid interpolation {cfg.get('interpolation')!r} is not supported (Linear or Smoothstep)")
        self.interp = INTERPOLATIONS[interp]
        if not 2 <= n_input_dims <= 5:
            raise ValueError(f"tinycudann drop-in: a grid encodes 2 to 5 input dimensions (got {n_input_dims})")
        if self.n_features not in (1, 2, 4, 8):
            raise ValueError(f"tinycudann drop-in: n_features_per_level must be 1, 2, 4 or 8 (got {self.n_features})")
        if not 1 <= self.n_levels <= 32:
            raise ValueError(f"tinycudann drop-in: n_levels must be in [1, 32] (got {self.n_levels})")
        if self.per_level_scale <= 0 or self.base_resolution < 1:
            raise ValueError("tinycudann drop-in: per_level_scale must be > 0 and base_resolution >= 1")
        self.offsets = level_offsets(n_input_dims, self.n_levels, self.per_level_scale, self.base_resolution, self.log2_hashmap_size)
        self.n_params = int(self.offsets[-1]) * self.n_features
        self.n_output_dims = self.n_levels * self.n_features

    def init(self, gen):
        return torch.empty(self.n_params).uniform_(-1e-4, 1e-4, generator=gen)

    def run(self, x, params, offsets, dtype):
        table = params.view(-1, self.n_features)
        if dtype == torch.half:
            table = table.to(torch.half)
        y = grid_encode(x.float().contiguous(), table, offsets, self.per_level_scale, self.base_resolution, x.requires_grad, self.gridtype,
                        False, self.interp)
        return y.to(dtype)


class _SHSpec:
    def __init__(self, n_input_dims, cfg):
        degree = int(cfg.get("degree", 4))
        if n_input_dims != 3 or degree != 4:
            raise ValueError(f"tinycudann drop-in: SphericalHarmonics is served for 3 inputs at degree 4 (got {n_input_dims} inputs, "
                             f"degree {degree})")
        self.n_params, self.n_output_dims = 0, 16
        self.sh = SHEncoder(3, 4)

    def init(self, gen):
        return torch.empty(0)

    def run(self, x, params, offsets, dtype):
        return self.sh(x.float() * 2 - 1).to(dtype)


def _encoding_spec(n_input_dims, cfg):
    otype = cfg.get("otype")
    if otype in ("HashGrid", "TiledGrid", "Grid"):
        return _GridSpec(n_input_dims, cfg)
    if otype == "SphericalHarmonics":
        return _SHSpec(n_input_dims, cfg)
    raise ValueError(f"tinycudann drop-in: encoding {otype!r} is not supported (HashGrid, TiledGrid, Grid, SphericalHarmonics)")


class _MlpSpec:
    def __init__(self, n_input_dims, n_output_dims, cfg):
        otype = cfg.get("otype")
        if otype != "FullyFusedMLP":
            raise ValueError(f"tinycudann drop-in: network {otype!r} is not supported (FullyFusedMLP)")
        act, out_act = _name(cfg.get("activation", "ReLU")), _name(cfg.get("output_activation", "None"))
        if act not in ("relu", "none"):
            raise ValueError(f"tinycudann drop-in: hidden activation {cfg.get('activation')!r} is not supported (ReLU or None)")
        if out_act != "none":
            raise ValueError(f"tinycudann drop-in: output activation {cfg.get('output_activation')!r} is not supported (None)")
        self.act = ACTIVATIONS["relu"] if act == "relu" else NO_ACTIVATION
        self.hidden = int(cfg.get("n_neurons", 128))
        self.layers = int(cfg.get("n_hidden_layers", 5))
        self.n_input_dims, self.n_output_dims = int(n_input_dims), int(n_output_dims)
        if self.hidden not in MLP_NEURONS:
            raise ValueError(f"tinycudann drop-in: FullyFusedMLP n_neurons must be one of {MLP_NEURONS} (got {self.hidden})")
        if not 1 <= self.layers <= MAX_HIDDEN_LAYERS:
            raise ValueError(f"tinycudann drop-in: n_hidden_layers must be in [1, {MAX_HIDDEN_LAYERS}] (got {self.layers})")
        if not 1 <= self.n_output_dims <= 16:
            raise ValueError(f"tinycudann drop-in: n_output_dims must be in [1, 16] (got {self.n_output_dims})")
        self.in_pad = -(-self.n_input_dims // 16) * 16
        if not 16 <= self.in_pad <= 256:
            raise ValueError(f"tinycudann drop-in: n_input_dims must be in [1, 256] (got {self.n_input_dims})")
        lds = self._lds_bytes()
        if lds > _LDS_BYTES:
            raise ValueError(f"tinycudann drop-in: a {self.in_pad}-input, {self.layers} x {self.hidden} FullyFusedMLP needs {lds} B of LDS "
                             f"per workgroup, more than the {_LDS_BYTES} B of a CU")
        self.shapes = [(self.hidden, self.in_pad)] + [(self.hidden, self.hidden)] * (self.layers - 1) + [(16, self.hidden)]
        self.n_params = sum(o * i for o, i in self.shapes)

    def _lds_bytes(self):
        """The weight images the kernels stage (csrc/ffmlp.hip mlp_fwd_lds / mlp_bwd_lds / mlp_bwd_fused_launch), in 1-KiB fragments."""
        MT, KC, I, L = (self.hidden + 31) // 32, self.hidden // 16, self.in_pad, self.layers
        fwd = MT * (I // 16) + (L - 1) * MT * KC + KC
        bwd = MT + (L - 1) * MT * KC + ((I + 31) // 32) * KC
        need = max(fwd, bwd) * 1024
        if self.hidden <= 64 and I <= 64 and L <= 4:       # the single-pass backward adds its row tiles and the forward image
            wd = max(32, self.hidden) + 8
            wa = max(I, max(32, self.hidden)) + 8
            need = max(need, bwd * 1024 + 4 * 32 * (wd + wa) * 2 + (MT * (I // 16) + (L - 1) * MT * KC) * 1024)
        return need

    def init(self, gen):
        parts = []
        for o, i in self.shapes:
            bound = math.sqrt(6.0 / (o + i))
            parts.append(torch.empty(o * i).uniform_(-bound, bound, generator=gen))
        return torch.cat(parts)

    def run(self, x, params):
        flat, lead = rows(x, self.n_input_dims)
        if not flat.is_cuda:
            raise RuntimeError(f"tinycudann drop-in: Network runs on the GPU (inputs are on {flat.device})")
        h = flat.to(torch.half)
        if self.in_pad != self.n_input_dims:
            h = torch.cat([h, h.new_full((h.shape[0], self.in_pad - self.n_input_dims), PAD_VALUE)], dim=1)
        blob = params.to(torch.half)
        train = torch.is_grad_enabled() and (blob.requires_grad or h.requires_grad)
        y = FusedMLP.apply(h, blob, self.in_pad, 16, self.hidden, self.layers, self.act, NO_ACTIVATION, not train, h.requires_grad)
        return unrows(y[:, :self.n_output_dims], lead)


def _generator(seed):
    return torch.Generator().manual_seed(int(seed))


class Encoding(nn.Module):
    def __init__(self, n_input_dims, encoding_config, seed=1337, dtype=None):
        super().__init__()
        if dtype not in (None, torch.half, torch.float):
            raise ValueError(f"tinycudann drop-in: Encoding dtype must be torch.half or torch.float (got {dtype})")
        self.n_input_dims, self.encoding_config, self.seed = int(n_input_dims), dict(encoding_config), seed
        self.dtype = torch.half if dtype is None else dtype
        self._spec = _encoding_spec(self.n_input_dims, self.encoding_config)
        self.n_output_dims = self._spec.n_output_dims
        self.params = nn.Parameter(self._spec.init(_generator(seed)))
        offsets = torch.from_numpy(np.asarray(getattr(self._spec, "offsets", np.zeros(1, np.int32))))
        self.register_buffer("_offsets", offsets, persistent=False)

    def forward(self, x):
        flat, lead = rows(x, self.n_input_dims)
        return unrows(self._spec.run(flat, self.params, self._offsets, self.dtype), lead)

    def extra_repr(self):
        return f"n_input_dims={self.n_input_dims}, n_output_dims={self.n_output_dims}, otype={self.encoding_config.get('otype')}, n_params={self.params.numel()}"


class Network(nn.Module):
    def __init__(self, n_input_dims, n_output_dims, network_config, seed=1337):
        super().__init__()
        self.n_input_dims, self.n_output_dims, self.network_config, self.seed = int(n_input_dims), int(n_output_dims), dict(network_config), seed
        self._spec = _MlpSpec(n_input_dims, n_output_dims, self.network_config)
        self.params = nn.Parameter(self._spec.init(_generator(seed)))

    def forward(self, x):
        return self._spec.run(x, self.params)

    def extra_repr(self):
        s = self._spec
        return (f"{self.n_input_dims} (padded {s.in_pad}) -> " + " -> ".join([str(s.hidden)] * s.layers) + f" -> {self.n_output_dims}, "
                f"activation={self.network_config.get('activation', 'ReLU')}, n_params={s.n_params}")


class NetworkWithInputEncoding(nn.Module):
    def __init__(self, n_input_dims, n_output_dims, encoding_config, network_config, seed=1337):
        super().__init__()
        self.n_input_dims, self.n_output_dims, self.seed = int(n_input_dims), int(n_output_dims), seed
        self.encoding_config, self.network_config = dict(encoding_config), dict(network_config)
        self._enc = _encoding_spec(self.n_input_dims, self.encoding_config)
        self._net = _MlpSpec(self._enc.n_output_dims, n_output_dims, self.network_config)
        gen = _generator(seed)
        self.params = nn.Parameter(torch.cat([self._net.init(gen), self._enc.init(gen)]))
        offsets = torch.from_numpy(np.asarray(getattr(self._enc, "offsets", np.zeros(1, np.int32))))
        self.register_buffer("_offsets", offsets, persistent=False)

    def forward(self, x):
        flat, lead = rows(x, self.n_input_dims)
        n = self._net.n_params
        encoded = self._enc.run(flat, self.params[n:], self._offsets, torch.half)
        return unrows(self._net.run(encoded, self.params[:n]), lead)
