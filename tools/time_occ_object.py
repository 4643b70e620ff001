"""One occupancy-grid training step and one 800 x 800 inference view of the object-conditioned networks (network_foc.py, network_tcnn.py),
timed with device events; the plain network's step at the same size rides along as the yardstick.

Step: 4096 rays of the bench's bound-2 scene, dt_gamma 1/128, max_steps 1024, synthetic.analytic_density_grid, a sample budget
(mean_count from one counting pass: the node runs as one library call), fp16 autocast, GradScaler, fused Adam over the network's
parameter groups, FOC's loss (MSE + 1e-8 x outside-mask criterion where the render returns one). View: staged=False, perturb off.
Every shape is warmed up first; each repeat is timed on its own and the median is reported. A tree that ignores yolo_details on the
marching path runs the same script (it renders with a zero feature through the op chain and the Python loop): the baseline.

    python tools/time_occ_object.py [--reps 30] [--view-reps 5] [--out result.json]
prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from focnerf_amd import synthetic

RENDER = dict(staged=False, dt_gamma=1 / 128, max_steps=1024)


def timed(fn, warmup, reps):
    """Median and all samples (ms) of `reps` runs of fn, each between its own pair of device events, after `warmup` untimed runs."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    marks = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        marks.append((s, e))
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e in marks]
    return statistics.median(ms), ms


def build(kind, dev):
    from focnerf_amd import network, network_foc, network_tcnn
    cls = {"network": network.NeRFNetwork, "network_foc": network_foc.NeRFNetwork, "network_tcnn": network_tcnn.NeRFNetwork}[kind]
    torch.manual_seed(0)
    m = cls(bound=2, cuda_ray=True).to(dev)
    m.set_density_grid(synthetic.analytic_density_grid(2, device=dev))
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--view-reps", type=int, default=5)
    ap.add_argument("--kinds", default="network_foc,network_tcnn,network")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_occ_object.py times GPU work: no device, no number"
    dev = torch.device("cuda", 0)
    bench.NUM_RAYS = 4096
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=0)
    o, d, target = bench.sample_batch(poses, intr, dev, torch.Generator().manual_seed(1))
    vo, vd = synthetic.get_rays(poses[:1], intr, 800, 800)
    result = {"rays": 4096, "reps": args.reps, "view_reps": args.view_reps}
    for kind in args.kinds.split(","):
        m = build(kind, dev).train()
        obj = kind != "network"
        yolo = bench.foc_yolo_details(dev, 4096, 7) if obj else None
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
            m.render(o, d, perturb=False, force_all_rays=True, **RENDER)                 # the counting pass
        marched = int(m.step_counter[(m.local_step - 1) % 16, 0])
        m.mean_count = marched + marched // 8                                            # a budget with room: no ray is dropped
        opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
        scaler = torch.amp.GradScaler("cuda")

        def step():
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.render(o, d, yolo, perturb=True, force_all_rays=False, bg_color=None, **RENDER) if obj else \
                    m.render(o, d, perturb=True, force_all_rays=False, bg_color=None, **RENDER)
                loss = torch.nn.functional.mse_loss(out["image"], target)
                if out.get("criterion_outside_mask") is not None:
                    loss = loss + 1e-8 * out["criterion_outside_mask"]
            opt.zero_grad(set_to_none=True)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
        med, ms = timed(step, 10, args.reps)
        entry = {"samples": marched, "train_step_ms": round(med, 4), "train_step_all_ms": [round(v, 4) for v in ms]}
        if obj:
            m.eval()
            view_yolo = (None, None, yolo[2])

            def view():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
                    m.render(vo, vd, view_yolo, perturb=False, bg_color=1.0, T_thresh=1e-4, **RENDER)
            med, ms = timed(view, 2, args.view_reps)
            entry.update({"view_ms": round(med, 3), "view_all_ms": [round(v, 3) for v in ms]})
        result[kind] = entry
        del m, opt
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
