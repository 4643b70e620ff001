"""GPU: the tinycudann drop-in (focnerf_amd/tcnn.py) on this package's kernels.

  * HashGrid / TiledGrid equal `grid_encode` on the same (fp16-read) table, bit for bit, forward and table gradient (the gradient where
    grid_encode itself is deterministic, see the test);
  * SphericalHarmonics equals sh_encode_deg4(2 x - 1) to fp16 rounding;
  * Network equals the CPU oracle's MLP chain on the padded input (pad column PAD_VALUE = 1.0, pinned here), forward and backward;
  * a network written to FOC's declared tcnn topology (sigma 32 -> 64 -> 16, yolo encoder 144 -> 16 -> 16, colour 47 -> 64 -> 64 -> 3:
    nerf/network_tcnn.py's defaults; written here on focnerf_amd.renderer.NeRFRenderer, not copied) runs `run()` forward + backward on
    4096 rays x 512 samples within a stated fp16 bound of the same network in fp32 torch ops, and trains.
Nothing here reads the reference tree."""
import math

import numpy as np
import pytest
import torch

import oracle
from util import assert_half_close, to_np

pytestmark = pytest.mark.gpu

HASH = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": float(np.exp2(np.log2(2048 * 2 / 16) / 15))}
SH = {"otype": "SphericalHarmonics", "degree": 4}
FP16_EPS = 2.0 ** -10
LOSS_SCALE = 4096.0


def _mlp(hidden, layers, activation="ReLU"):
    return {"otype": "FullyFusedMLP", "activation": activation, "output_activation": "None", "n_neurons": hidden, "n_hidden_layers": layers}


@pytest.mark.parametrize("cfg,B", [(dict(HASH), 1000), (dict(HASH), 300_000), (dict(HASH, interpolation="Smoothstep"), 1000),
                                   (dict(HASH, interpolation="Smoothstep"), 300_000), (dict(HASH, otype="Grid", type="Hash", n_levels=8), 300_000),
                                   (dict(HASH, otype="TiledGrid", log2_hashmap_size=17), 1000),
                                   (dict(HASH, otype="Grid", type="Tiled", log2_hashmap_size=17), 1000)])
def test_grid_equals_grid_encode_bit_for_bit(cfg, B):
    """Forward: the same bits at every batch. Table gradient: the same bits where grid_encode's own backward is run-to-run deterministic
    (hash grids, B <= 1000); above that, segments of more than 65 536 records meet in half2 atomics whose order is not fixed, and tiled grids
    take the scattered-atomic backward throughout (fp16 atomics, so they are compared at 1000 points only): there the bound is the one
    tests/test_gpu_gridencoder.py allows between two launches."""
    from focnerf_amd import tcnn
    from focnerf_amd.gridencoder import GRID_TYPES, INTERPOLATIONS, grid_encode
    enc = tcnn.Encoding(3, cfg).cuda()
    with torch.no_grad():
        enc.params.uniform_(-1, 1)                               # table values that make every level visible
    x = torch.rand(B, 3, device="cuda")
    g = torch.randn(x.shape[0], enc.n_output_dims, device="cuda").half()
    y = enc(x)
    assert y.dtype == torch.float16 and y.shape == (x.shape[0], enc.n_output_dims)
    y.backward(g)
    table = enc.params.detach().view(-1, cfg["n_features_per_level"]).half().requires_grad_(True)
    gridtype = GRID_TYPES["tiled" if cfg["otype"] == "TiledGrid" or cfg.get("type") == "Tiled" else "hash"]
    ref = grid_encode(x, table, enc._offsets, cfg["per_level_scale"], cfg["base_resolution"], False, gridtype, False,
                      INTERPOLATIONS[cfg.get("interpolation", "Linear").lower()])
    ref.backward(g)
    assert torch.equal(y.view(torch.int16), ref.view(torch.int16))
    got, want = enc.params.grad.view_as(table), table.grad.float()
    if B <= 1000 and gridtype == GRID_TYPES["hash"]:
        assert torch.equal(got, want)
    else:
        assert_half_close(to_np(got), to_np(want), ulps=2.0, atol=4 * 2.0 ** -10 * float(want.abs().max()), what="table gradient")
    # inputs outside [0, 1] encode to zeros (this package's encoder; tcnn's behaviour there is not pinned)
    with torch.no_grad():
        out = enc(torch.tensor([[1.5, 0.5, 0.5], [-0.25, 0.5, 0.5]], device="cuda"))
    assert torch.count_nonzero(out) == 0


def test_spherical_harmonics_on_unit_cube_inputs():
    from focnerf_amd import tcnn
    from focnerf_amd.shencoder import sh_encode_deg4
    enc = tcnn.Encoding(3, SH).cuda()
    d = torch.nn.functional.normalize(torch.randn(4097, 3, device="cuda"), dim=-1)
    u = (d + 1) / 2                                              # what FOC feeds it (network_tcnn.py: "inputs in [0, 1]")
    y = enc(u)
    assert y.dtype == torch.float16 and y.shape == (4097, 16)
    want = sh_encode_deg4(u.float() * 2 - 1)
    assert_half_close(to_np(y), to_np(want), ulps=1.0, atol=1e-6, what="SH")
    assert enc(u.unsqueeze(0)).shape == (1, 4097, 16)


@pytest.mark.parametrize("n_in,n_out,hidden,layers,act", [(32, 16, 64, 1, "ReLU"), (47, 3, 64, 2, "ReLU"), (144, 16, 16, 1, "ReLU"),
                                                           (31, 3, 64, 2, "ReLU"), (3, 4, 32, 1, "None"), (100, 7, 128, 1, "ReLU")])
@pytest.mark.parametrize("B", [1, 127, 4097])
def test_network_equals_the_oracle_chain(n_in, n_out, hidden, layers, act, B):
    from focnerf_amd import tcnn
    net = tcnn.Network(n_in, n_out, _mlp(hidden, layers, act)).cuda()
    pad = -(-n_in // 16) * 16
    rng = np.random.default_rng(n_in + B)
    x = torch.from_numpy(rng.standard_normal((B, n_in)).astype(np.float32)).cuda().requires_grad_(True)
    y = net(x)
    assert y.dtype == torch.float16 and y.shape == (B, n_out)
    g = torch.from_numpy((rng.standard_normal((B, n_out)) * 0.05).astype(np.float16)).cuda()
    y.backward(g)
    xp = np.concatenate([to_np(x.detach().half()), np.full((B, pad - n_in), tcnn.PAD_VALUE, np.float16)], axis=1)
    W = to_np(net.params.detach().half())
    code = 0 if act == "ReLU" else 6
    ref_out, ref_fb = oracle.ffmlp_forward(xp, W, pad, hidden, layers, code)
    assert_half_close(to_np(y), ref_out[:, :n_out], ulps=2.0 * (layers + 1), atol=4e-3, what="outputs")
    gp = np.zeros((B, 16), np.float16)
    gp[:, :n_out] = to_np(g)
    # the oracle's backward on the kernels' forward activations (the stored buffer of the same training forward)
    from focnerf_amd.backend import _ffmlp as be
    fb = torch.empty(layers, B, hidden, dtype=torch.float16, device="cuda")
    be.ffmlp_forward(torch.from_numpy(xp).cuda(), torch.from_numpy(W).cuda(), B, pad, 16, hidden, layers, code, 6, fb,
                     torch.empty(B, 16, dtype=torch.float16, device="cuda"))
    gw_r, gi_r, _ = oracle.ffmlp_backward(gp, xp, W, to_np(fb), pad, hidden, layers, code, True)
    assert_half_close(to_np(x.grad), gi_r[:, :n_in].astype(np.float32), ulps=2.0 * (layers + 1), atol=5e-4, what="input gradient")
    assert_half_close(to_np(net.params.grad), gw_r, ulps=4.0, atol=2e-3 * max(1.0, B / 1024), what="parameter gradient")
    # the pad value is part of the result: with the pad column at 0 the first layer's last weight column would not count
    if pad != n_in and B > 100:
        xz = xp.copy()
        xz[:, n_in:] = 0
        assert not np.array_equal(oracle.ffmlp_forward(xz, W, pad, hidden, layers, code, training=False)[:, :n_out], to_np(y))
    with torch.no_grad():
        assert torch.equal(net(x.detach()), y.detach()), "inference and training forms agree"


def test_network_takes_any_dtype_and_empty_batches():
    from focnerf_amd import tcnn
    net = tcnn.Network(32, 16, _mlp(64, 1)).cuda()
    x = torch.rand(64, 32, device="cuda")
    y = net(x)
    assert torch.equal(net(x.double()), y) and torch.equal(net(x.half()), y)
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.equal(net(x), y)
    e = net(torch.empty(0, 32, device="cuda"))
    assert e.shape == (0, 16) and e.dtype == torch.float16


# ---------------------------------------------------------------- FOC's tcnn topology, end to end
def _foc_network(bound):
    from focnerf_amd import tcnn
    from focnerf_amd.activation import trunc_exp
    from focnerf_amd.renderer import NeRFRenderer

    def lin(x, w, o, i):
        return x @ w.view(o, i).t()

    def mlp32(spec, params, x):
        """the tcnn.Network's arithmetic in fp32 torch ops on its parameters (pad column, ReLU, output rows past n_output_dims dropped)"""
        h = torch.cat([x.float(), torch.full((x.shape[0], spec.in_pad - spec.n_input_dims), tcnn.PAD_VALUE, device=x.device)], dim=1)
        off = 0
        for k, (o, i) in enumerate(spec.shapes):
            h = lin(h, params[off:off + o * i], o, i)
            off += o * i
            if k + 1 < len(spec.shapes):
                h = torch.relu(h)
        return h[:, :spec.n_output_dims]

    class FocTcnnNetwork(NeRFRenderer):
        """FOC's declared tcnn network (sigma 32 -> 64 -> 16, SH(d), object feature 144 -> 16 -> 16, colour 47 -> 64 -> 64 -> 3) in the
        order of operations the FOC trainer calls it; `fp32` switches every module to fp32 torch ops on the same parameters."""

        def __init__(self):
            super().__init__(bound, cuda_ray=False, density_scale=1, min_near=0.05)
            self.encoder = tcnn.Encoding(3, dict(HASH, per_level_scale=float(np.exp2(np.log2(2048 * bound / 16) / 15))))
            self.sigma_net = tcnn.Network(32, 16, _mlp(64, 1))
            self.yolo_feat_encoder = tcnn.Network(144, 16, _mlp(16, 1))
            self.encoder_dir = tcnn.Encoding(3, SH)
            self.color_net = tcnn.Network(47, 3, _mlp(64, 2))
            self.fp32 = False

        def _encode(self, x):
            if not self.fp32:
                return self.encoder(x)
            from focnerf_amd.gridencoder import grid_encode
            s = self.encoder._spec
            return grid_encode(x, self.encoder.params.view(-1, 2), self.encoder._offsets, s.per_level_scale, s.base_resolution, False)

        def _net(self, m, x):
            return mlp32(m._spec, m.params, x) if self.fp32 else m(x)

        def _sh(self, u):
            from focnerf_amd.shencoder import sh_encode_deg4
            return sh_encode_deg4(u.float() * 2 - 1) if self.fp32 else self.encoder_dir(u)

        def density(self, x, yolo_details=None):
            x = (x + self.bound) / (2 * self.bound)
            h = self._net(self.sigma_net, self._encode(x))
            return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

        def color(self, x, d, yolo_details=None, mask=None, geo_feat=None, **kwargs):
            obj = self._net(self.yolo_feat_encoder, yolo_details[2].unsqueeze(0))
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
            h = torch.cat([self._sh((d + 1) / 2), geo_feat, obj.squeeze(0).repeat(d.shape[0], 1)], dim=-1)
            rgbs[mask] = torch.sigmoid(self._net(self.color_net, h)).to(rgbs.dtype)
            return rgbs

    return FocTcnnNetwork()


def test_foc_topology_run_against_fp32_and_training():
    """4096 rays x 512 samples through NeRFRenderer.run, forward + backward: the image and every parameter gradient within a bound derived
    from fp16 rounding (FP16_EPS = 2^-10) of the same network in fp32 torch ops; then twenty Adam steps lower the loss (by 10 % at least) and stay finite.
    Bounds: image max |difference| <= 16 eps (a handful of fp16 roundings per sample, weights summing to <= 1); per-parameter-tensor
    relative gradient error ||g16 - g32|| / ||g32|| <= 32 eps (the fp16 deltas of each layer, each a few roundings deep). The loss is scaled
    by LOSS_SCALE before the backward pass, as the trainer's GradScaler does: unscaled, the hash table's gradients (~1e-9) are below fp16."""
    from focnerf_amd import synthetic
    torch.manual_seed(0)
    bound = 1
    net = _foc_network(bound).cuda()
    with torch.no_grad():
        net.encoder.params.uniform_(-0.5, 0.5)
    rays_o, rays_d = synthetic.make_view_rays(64, 64, bound, 1, seed=0, device="cuda")
    rays_o, rays_d = rays_o[0].contiguous(), rays_d[0].contiguous()
    n, T = rays_o.shape[0], 512
    assert n == 4096
    gen = torch.Generator(device="cuda").manual_seed(1)
    mask = torch.rand(1, n, T, device="cuda", generator=gen) < 0.9
    feat = torch.rand(144, device="cuda", generator=gen)
    yolo = (mask, None, feat)
    target = 0.5 + 0.4 * torch.sin(3 * rays_d)

    def step(fp32):
        net.fp32 = fp32
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16, enabled=not fp32):
            out = net.run(rays_o, rays_d, yolo_details=yolo, num_steps=T, perturb=False)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        (loss * LOSS_SCALE).backward()
        return out["image"].detach().float(), {k: p.grad.detach().clone() / LOSS_SCALE for k, p in net.named_parameters() if p.numel()}

    img16, g16 = step(False)
    img32, g32 = step(True)
    diff = float((img16 - img32).abs().max())
    assert diff <= 16 * FP16_EPS, f"image: max |fp16 - fp32| = {diff:.3g}"
    assert float(img32.std()) > 1e-2, "degenerate scene"
    for k in g32:
        rel = float((g16[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30))
        assert float(g32[k].norm()) > 0 and rel <= 32 * FP16_EPS, f"{k}: relative gradient error {rel:.3g}"

    net.fp32 = False
    opt = torch.optim.Adam(net.parameters(), lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")                      # the reference trainer's fp16 mode
    losses = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.run(rays_o, rays_d, yolo_details=yolo, num_steps=T, perturb=True)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    assert all(math.isfinite(v) for v in losses) and all(torch.isfinite(p).all() for p in net.parameters())
    assert losses[-1] < 0.9 * losses[0], f"loss {losses[0]:.4g} -> {losses[-1]:.4g}"
