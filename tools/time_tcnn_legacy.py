#!/usr/bin/env python3
"""torch-ngp's tcnn network (legacy/nerf/network_tcnn.py, `main_nerf.py --legacy --tcnn -O`) on the occupancy grid. GPU only:
    python tools/time_tcnn_legacy.py [steps]
Prints one JSON line with, for three networks, one configs[2]-size training step (bound 2, 4096 rays, NeRFRenderer.render -> run_cuda,
fp16 autocast, MSE, GradScaler, fused Adam, the sample budget set as update_extra_state would) and one 800 x 800 occupancy render
(device_compaction=True):
  * dropin_ops: the legacy topology built from tcnn.Encoding / tcnn.Network, called op by op in the reference file's order (march_rays_train,
    the network's forward, composite_rays_train; the Python inference loop with the list compacted on the device);
  * legacy_fused: network_tcnn_legacy.NeRFNetwork (the occupancy node and the native loop through the *_pad31 entry points);
  * network: network.NeRFNetwork (torch-ngp's FFMLP network, one sigma hidden layer more).
The three legs run alternately in one process (median of the rounds, milliseconds)."""
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import numpy as np  # noqa: E402
import torch  # noqa: E402

BOUND, RAYS, VIEW = 2, 4096, 800


def _dropin_legacy():
    from focnerf_amd import tcnn
    from focnerf_amd.activation import trunc_exp
    from focnerf_amd.renderer import NeRFRenderer
    mlp = lambda l: {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": l}

    class Net(NeRFRenderer):
        def __init__(self):
            super().__init__(BOUND, cuda_ray=True, density_scale=1)
            self.encoder = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                                             "base_resolution": 16, "per_level_scale": float(np.exp2(np.log2(2048 * BOUND / 16) / 15))})
            self.sigma_net = tcnn.Network(32, 16, mlp(1))
            self.encoder_dir = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})
            self.color_net = tcnn.Network(31, 3, mlp(2))

        def forward(self, x, d):
            f = self.density(x)
            return f['sigma'], torch.sigmoid(self.color_net(torch.cat([self.encoder_dir((d + 1) / 2), f['geo_feat']], dim=-1)))

        def density(self, x):
            h = self.sigma_net(self.encoder((x + self.bound) / (2 * self.bound)))
            return {'sigma': trunc_exp(h[..., 0]), 'geo_feat': h[..., 1:]}

        def get_params(self, lr):
            return [{'params': m.parameters(), 'lr': lr} for m in (self.encoder, self.sigma_net, self.encoder_dir, self.color_net)]

    return Net()


def _legs():
    from focnerf_amd import synthetic
    from focnerf_amd.network import NeRFNetwork as Plain
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork as Legacy
    legs = {"dropin_ops": _dropin_legacy(), "legacy_fused": Legacy(bound=BOUND, cuda_ray=True, density_scale=1),
            "network": Plain(bound=BOUND, cuda_ray=True, density_scale=1)}
    grid = synthetic.analytic_density_grid(BOUND, device="cuda")
    for m in legs.values():
        m.cuda().set_density_grid(grid)
    legs["legacy_fused"].load_state_dict(legs["dropin_ops"].state_dict(), strict=True)     # the same parameters in the two tcnn legs
    return legs


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    from focnerf_amd import synthetic
    torch.manual_seed(0)
    legs = _legs()
    o, d = synthetic.make_view_rays(VIEW, VIEW, BOUND, 4, seed=1, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    batches = []
    for v in range(4):
        pick = torch.randint(0, VIEW * VIEW, (RAYS,), device="cuda", generator=g)
        batches.append((o[v:v + 1, pick].contiguous(), d[v:v + 1, pick].contiguous(), (0.5 + 0.4 * torch.sin(3 * d[v:v + 1, pick])).contiguous()))
    state = {}
    for name, m in legs.items():
        m.train()
        opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
        state[name] = (opt, torch.amp.GradScaler("cuda"))

    def step(name, i):
        m, (opt, scaler) = legs[name], state[name]
        ro, rd, target = batches[i % 4]
        with torch.autocast("cuda", dtype=torch.float16):
            out = m.render(ro, rd, staged=False, perturb=True, force_all_rays=False, dt_gamma=1 / 128, max_steps=1024, bg_color=None)
            loss = torch.nn.functional.mse_loss(out["image"], target)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    for name, m in legs.items():                               # warm-up, then the sample budget update_extra_state would set
        for i in range(17):
            step(name, i)
        m.mean_count = int(m.step_counter[:16, 0].sum().item() / 16)
    train = {n: [] for n in legs}
    for r in range(5):
        for name, m in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                step(name, i)
            torch.cuda.synchronize()
            train[name].append(1e3 * (time.perf_counter() - t0) / steps)
    samples = {n: float(m.step_counter[:, 0].float().mean()) for n, m in legs.items()}

    render = {n: [] for n in legs}
    ro, rd = o[:1].contiguous(), d[:1].contiguous()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for m in legs.values():
            m.eval()
            m.render(ro, rd, staged=False, perturb=False, dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4, device_compaction=True)
        for r in range(3):
            for name, m in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.render(ro, rd, staged=False, perturb=False, dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4, device_compaction=True)
                torch.cuda.synchronize()
                render[name].append(1e3 * (time.perf_counter() - t0))
    out = {n: {"train_ms_per_step": round(statistics.median(train[n]), 3), "train_ms_min": round(min(train[n]), 3), "samples_per_step": round(samples[n]),
               "render_ms_per_view": round(statistics.median(render[n]), 2), "render_ms_min": round(min(render[n]), 2)} for n in legs}
    print(json.dumps({"tool": "time_tcnn_legacy", "bound": BOUND, "rays": RAYS, "view": VIEW, "steps": steps, "legs": out}))


if __name__ == "__main__":
    main()
