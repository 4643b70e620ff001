#!/usr/bin/env python3
"""torch-ngp's default network (network_linear.NeRFNetwork: legacy/nerf/network.py, `main_nerf.py --legacy -O`), op route against fused
route. GPU only:
    python tools/time_linear.py [steps]
Prints one JSON line. Routes: `ops` = every FOC_FUSED_* switch off (nn.Linear GEMMs, the drop-in encoders, torch glue, the background
op chain); `fused` = the defaults (fused nodes, packed weight blobs, csrc/background.hip). Each leg with the background off and with
bg_radius = 32; the routes run alternately in one process, median of the rounds, milliseconds:
  * fixed_train: one fixed-step training step, 4096 rays x 512 samples, bound 1 (run(fused=True) / run()), fp16 autocast, MSE, GradScaler,
    fused Adam;
  * occ_train: one configs[2]-size occupancy training step (bound 2, 4096 rays, render -> run_cuda), the sample budget set as
    update_extra_state would, fused Adam inside the step;
  * fixed_render / occ_render: one 800 x 800 view (render(staged=True, fused=True), 512 samples; run_cuda with device_compaction);
  * bg_train_4096 (forward + backward) and bg_infer_640000 (forward): the background alone, kernel against its op chain.
"""
import json
import os
import statistics
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
import torch  # noqa: E402

RAYS, VIEW = 4096, 800
SWITCHES = ("FOC_FUSED_FIELD", "FOC_FUSED_TAIL", "FOC_FUSED_INFER", "FOC_FUSED_OCC", "FOC_FUSED_HEAD", "FOC_RENDER_NATIVE", "FOC_FUSED_BG")
ROUTES = ("ops", "fused")


def _route(name):
    for k in SWITCHES:
        os.environ[k] = "1" if name == "fused" else "0"


def _timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def _alternate(fns, n, rounds):
    """fns: route -> fn(i); one warm-up call each, then `rounds` rounds of n calls per route, alternating -> route -> median ms."""
    for r, fn in fns.items():
        _route(r)
        fn(0)
    out = {r: [] for r in fns}
    for _ in range(rounds):
        for r, fn in fns.items():
            _route(r)
            out[r].append(_timed(fn, n))
    return {r: round(statistics.median(v), 3) for r, v in out.items()}


def _model(bound, bg, cuda_ray):
    from focnerf_amd import synthetic
    from focnerf_amd.network_linear import NeRFNetwork
    torch.manual_seed(0)
    m = NeRFNetwork(bound=bound, cuda_ray=cuda_ray, density_scale=1, bg_radius=bg).cuda()
    with torch.no_grad():
        m.encoder.embeddings.uniform_(-0.5, 0.5)
    if cuda_ray:
        m.set_density_grid(synthetic.analytic_density_grid(bound, device="cuda"))
    return m


def _train_leg(bound, bg, occ, steps):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(VIEW, VIEW, bound, 4, seed=1, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    batches = []
    for v in range(4):
        pick = torch.randint(0, VIEW * VIEW, (RAYS,), device="cuda", generator=g)
        batches.append((o[v:v + 1, pick].contiguous(), d[v:v + 1, pick].contiguous(), (0.5 + 0.4 * torch.sin(3 * d[v:v + 1, pick])).contiguous()))
    fns = {}
    for route in ROUTES:
        m = _model(bound, bg, occ).train()
        opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
        scaler = torch.amp.GradScaler("cuda")

        def step(i, m=m, opt=opt, scaler=scaler, route=route):
            ro, rd, target = batches[i % 4]
            with torch.autocast("cuda", dtype=torch.float16):
                if occ:
                    out = m.render(ro, rd, staged=False, perturb=True, dt_gamma=1 / 128, max_steps=1024)
                else:
                    out = m.run(ro[0], rd[0], None, fused=route == "fused", num_steps=512, upsample_steps=0, perturb=True)
                loss = torch.nn.functional.mse_loss(out["image"].float().view(-1, 3), target.view(-1, 3))
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        if occ:
            _route(route)
            for i in range(17):
                step(i)
            m.mean_count = int(m.step_counter[:16, 0].sum().item() / 16)
        fns[route] = step
    return _alternate(fns, steps, 5)


def _render_leg(bound, bg, occ):
    from focnerf_amd import synthetic
    o, d = synthetic.make_view_rays(VIEW, VIEW, bound, 1, seed=3, device="cuda")
    fns = {}
    for route in ROUTES:
        m = _model(bound, bg, occ).eval()

        def view(i, m=m, route=route):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                if occ:
                    m.render(o, d, staged=False, perturb=False, dt_gamma=1 / 128, max_steps=1024, T_thresh=1e-4, device_compaction=True)
                else:
                    m.render(o, d, staged=True, max_ray_batch=4096, fused=route == "fused", num_steps=512, upsample_steps=0, perturb=False,
                             return_fields=False)
        fns[route] = view
    return _alternate(fns, 1, 3)


def _background_legs(steps):
    m = _model(1, 32.0, False)
    out = {}
    for N, train in ((4096, True), (640000, False)):
        g = torch.Generator(device="cuda").manual_seed(N)
        o = (torch.rand(N, 3, generator=g, device="cuda") * 2 - 1) * 0.9
        d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g, device="cuda"), dim=-1)
        grad = torch.rand(N, 3, generator=g, device="cuda").half()

        def call(i):
            with torch.set_grad_enabled(train), torch.autocast("cuda", dtype=torch.float16):
                rgb = m._background_colour(o, d, None)
            if train:
                rgb.backward(grad)
        out[f"bg_{'train' if train else 'infer'}_{N}"] = _alternate({r: call for r in ROUTES}, steps, 5)
    return out


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    legs = {}
    for bg in (-1.0, 32.0):
        tag = "bg" if bg > 0 else "nobg"
        legs[f"fixed_train_{tag}"] = _train_leg(1, bg, False, steps)
        legs[f"occ_train_{tag}"] = _train_leg(2, bg, True, steps)
        legs[f"fixed_render_{tag}"] = _render_leg(1, bg, False)
        legs[f"occ_render_{tag}"] = _render_leg(2, bg, True)
        print(f"time_linear: {tag} legs done", file=sys.stderr, flush=True)      # progress (the legs take minutes)
    legs.update(_background_legs(steps))
    for k in SWITCHES:
        os.environ.pop(k, None)
    share = {k: round((legs[f"{k}_train_bg"]["fused"] - legs[f"{k}_train_nobg"]["fused"]) / legs[f"{k}_train_bg"]["fused"], 4) for k in ("fixed", "occ")}
    print(json.dumps({"tool": "time_linear", "rays": RAYS, "view": VIEW, "steps": steps, "legs": legs, "background_share_of_fused_train": share}))


if __name__ == "__main__":
    main()
