#!/usr/bin/env python3
"""One hidden layer against two, and FOC's tcnn-topology network through the tinycudann drop-in (focnerf_amd/tcnn.py). GPU only:
    python tools/time_tcnn.py [reps]
Prints one JSON line:
  * mlp: fused MLP forward + backward (training forward with nothing kept, re-evaluating single-pass backward with input gradients: what
    FusedMLP runs) at 2 097 152 rows for 32 -> 64 -> 16 and 48 -> 64 -> 16, num_layers 1 and 2 timed alternately in one process: median
    microseconds per forward + backward and useful TFLOP/s (2 flops per multiply-add of the network's matrices, x3 for forward + both
    backward products, the re-evaluated forward not counted);
  * foc_tcnn_step: one training step at configs[1] size (4096 rays x 512 samples, fixed-step NeRFRenderer.run, fp16 autocast, Adam over
    the five parameter groups) of a network in FOC's tcnn topology built from tcnn.Encoding / tcnn.Network and called in the order of the
    reference's network_tcnn.py; samples/s beside `dropin_ops_path` of BENCH_r05 (4.7e8: nerf/network_ff.py on the same public ops);
  * fused_step: the same step of network_tcnn.NeRFNetwork (that topology with the drop-in's parameter layout) and of network_foc.NeRFNetwork
    through run(fused=True) (fixed-step fused path, upsample_steps 0), the three legs timed alternately in one process."""
import json
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DROPIN_OPS_PATH_R05 = 4.7e8


def _events(fn, reps):
    """microseconds per call of `fn`, `reps` back-to-back calls between two events"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / reps


def time_mlp(reps):
    from focnerf_amd.ffmlp import ffmlp_forward
    M, dev = 4096 * 512, torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    out = {}
    for I in (32, 48):
        x = (torch.rand(M, I, device=dev, generator=g) - 0.5).half().requires_grad_(True)
        dy = (torch.randn(M, 16, device=dev, generator=g) * 0.01).half()
        calls = {}
        for nl in (1, 2):
            w = ((torch.rand(64 * (I + 64 * (nl - 1) + 16), device=dev, generator=g) - 0.5) * 0.4).half().requires_grad_(True)

            def step(w=w, nl=nl):
                y = ffmlp_forward(x, w, I, 16, 64, nl, 0, 6, False, True)
                y.backward(dy)
            calls[nl] = (step, 2 * 3 * M * 64 * (I + 64 * (nl - 1) + 16))
        for fn, _ in calls.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = {1: [], 2: []}
        for _ in range(7):                                  # alternating bursts: both forms see the same clocks and neighbours
            for nl in (1, 2):
                ts[nl].append(_events(calls[nl][0], reps))
        for nl in (1, 2):
            us = statistics.median(ts[nl])
            out[f"{I}->64x{nl}->16"] = {"us": round(us, 1), "us_min": round(min(ts[nl]), 1), "tflops": round(calls[nl][1] / us * 1e-6, 2)}
    return out


def _dropin_network():
    """FOC's tcnn topology on tcnn.Encoding / tcnn.Network, called op by op in the order of the reference's network_tcnn.py"""
    from focnerf_amd import tcnn
    from focnerf_amd.activation import trunc_exp
    from focnerf_amd.renderer import NeRFRenderer

    def mlp(n_in, n_out, hidden):
        return tcnn.Network(n_in, n_out, {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": hidden,
                                          "n_hidden_layers": 1 if n_in in (32, 144) else 2})

    class Net(NeRFRenderer):
        def __init__(self, bound):
            super().__init__(bound, cuda_ray=False, density_scale=1, min_near=0.05)
            self.encoder = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                                             "base_resolution": 16, "per_level_scale": float(np.exp2(np.log2(2048 * bound / 16) / 15))})
            self.sigma_net, self.yolo_feat_encoder = mlp(32, 16, 64), mlp(144, 16, 16)
            self.encoder_dir = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})
            self.color_net = mlp(47, 3, 64)

        def density(self, x, yolo_details=None):
            h = self.sigma_net(self.encoder((x + self.bound) / (2 * self.bound)))
            return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

        def color(self, x, d, yolo_details=None, mask=None, geo_feat=None, **kwargs):
            obj = self.yolo_feat_encoder(yolo_details[2].unsqueeze(0))
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
            h = torch.cat([self.encoder_dir((d + 1) / 2), geo_feat, obj.squeeze(0).repeat(d.shape[0], 1)], dim=-1)
            rgbs[mask] = torch.sigmoid(self.color_net(h)).to(rgbs.dtype)
            return rgbs

    return Net


def _training_step(net, fused, bound=2, T=512):
    """one Adam step at configs[1] size (4096 rays x 512 samples) of `net`, through run(fused=True) or NeRFRenderer.run"""
    from focnerf_amd import synthetic
    dev = torch.device("cuda")
    rays_o, rays_d = synthetic.make_view_rays(64, 64, bound, 1, seed=0, device=dev)
    rays_o, rays_d = rays_o[0].contiguous(), rays_d[0].contiguous()
    yolo = (torch.ones(1, rays_o.shape[0], T, dtype=torch.bool, device=dev), None, torch.rand(144, device=dev))
    target = torch.rand(rays_o.shape[0], 3, device=dev)
    opt = torch.optim.Adam([{'params': m.parameters(), 'lr': 1e-2} for m in (net.encoder, net.sigma_net, net.encoder_dir, net.color_net,
                                                                              net.yolo_feat_encoder)], betas=(0.9, 0.99), eps=1e-15)
    scaler = torch.amp.GradScaler("cuda")
    kw = dict(fused=True, upsample_steps=0) if fused else {}

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            out = net.run(rays_o, rays_d, yolo_details=yolo, num_steps=T, perturb=True, **kw)
            loss = torch.nn.functional.mse_loss(out["image"].float(), target)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    return step, rays_o.shape[0] * T


def time_steps(steps):
    """foc_tcnn_step (drop-in, op by op) and fused_step (network_tcnn / network_foc under run(fused=True)), in alternating bursts"""
    from focnerf_amd import network_foc, network_tcnn
    dev, bound = torch.device("cuda"), 2
    torch.manual_seed(0)
    legs = {"dropin_ops": _training_step(_dropin_network()(bound).to(dev), False),
            "network_tcnn_fused": _training_step(network_tcnn.NeRFNetwork(bound=bound, cuda_ray=False, density_scale=1, min_near=0.05).to(dev), True),
            "network_foc_fused": _training_step(network_foc.NeRFNetwork(bound=bound, cuda_ray=False, density_scale=1, min_near=0.05).to(dev), True)}
    for step, _ in legs.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(3):
        for k, (step, _) in legs.items():
            ts[k].append(_events(step, steps))
    out = {}
    for k, (_, n) in legs.items():
        ms = statistics.median(ts[k]) * 1e-3
        sps = n / (ms * 1e-3)
        out[k] = {"ms_per_step": round(ms, 3), "samples_per_sec": sps, "vs_dropin_ops_path_r05": round(sps / DROPIN_OPS_PATH_R05, 3)}
    out["network_tcnn_fused"]["vs_dropin_ops"] = round(out["network_tcnn_fused"]["samples_per_sec"] / out["dropin_ops"]["samples_per_sec"], 3)
    out["network_tcnn_fused"]["vs_network_foc_fused"] = round(out["network_tcnn_fused"]["samples_per_sec"] / out["network_foc_fused"]["samples_per_sec"], 3)
    out.update(rays=4096, samples_per_ray=512, bound=bound)
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_tcnn.py needs a GPU")
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    print(json.dumps({"tool": "time_tcnn", "rows": 4096 * 512, "mlp": time_mlp(reps), "steps": time_steps(max(5, reps // 2))}))


if __name__ == "__main__":
    main()
