"""What the ray distortion costs: the headline fixed-step step (bench.py's shape) and the configs[2] occupancy step, each with the keyword off
and on, alternating round by round in ONE process on the same inputs (whatever else the box is doing falls on both), plus the only
alternative a user had before the keyword: the torch formulation (focnerf_amd.loss.ray_distortion) on the route without the fused tail
(FOC_FUSED_TAIL=0; fixed-step only — the unfused occupancy chain forms no per-sample weights). Per variant: the median of the rounds and
their spread (min .. max); times are device events around a block of steps. Run on the GPU box:

    python tools/time_distortion.py [--rounds 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

dev = torch.device("cuda", 0)
LAMBDA = 1e-2


def timed(fn, calls):
    """ms per call of `calls` back-to-back calls (device events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(calls):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def _setup(cuda_ray):
    m = bench.build_model(2, dev, cuda_ray=cuda_ray, seed=0).train()
    opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
    sc = torch.amp.GradScaler("cuda")
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=0)
    gen = torch.Generator().manual_seed(0)
    return m, opt, sc, [bench.sample_batch(poses, intr, dev, gen) for _ in range(4)]


def _step(m, opt, sc, batch, distortion, **kw):
    """bench.train_step / cuda_ray_train_step with the keyword and lambda * mean(distortion) in the loss."""
    rays_o, rays_d, target = batch
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(rays_o, rays_d, staged=False, perturb=True, bg_color=None, **kw, **({"distortion": True} if distortion else {}))
        loss = torch.nn.functional.mse_loss(out["image"], target)
        if distortion:
            loss = loss + LAMBDA * out["distortion"].mean()
    sc.scale(loss).backward()
    sc.step(opt)
    sc.update()


def headline_variants():
    m, opt, sc, batches = _setup(False)
    kw = dict(num_steps=bench.NUM_STEPS, upsample_steps=0, fused=True)

    def unfused(i):
        os.environ["FOC_FUSED_TAIL"] = "0"
        try:
            _step(m, opt, sc, batches[i % 4], True, **kw)
        finally:
            del os.environ["FOC_FUSED_TAIL"]
    return {"off": lambda i: _step(m, opt, sc, batches[i % 4], False, **kw), "on": lambda i: _step(m, opt, sc, batches[i % 4], True, **kw),
            "torch_on_unfused_tail": unfused}


def occupancy_variants():
    m, opt, sc, batches = _setup(True)
    kw = dict(force_all_rays=False, dt_gamma=1 / 128, max_steps=1024)
    for i in range(17):                                     # bench.py's occupancy leg: the sample budget comes from the first 16 marches
        _step(m, opt, sc, batches[i % 4], False, **kw)
        if i == 15:
            m.mean_count = int(m.step_counter[:16, 0].sum().item() / 16)
    return {"off": lambda i: _step(m, opt, sc, batches[i % 4], False, **kw), "on": lambda i: _step(m, opt, sc, batches[i % 4], True, **kw)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    result = {"rounds": args.rounds, "lambda": LAMBDA, "cases": {}}
    for name, make, calls in (("headline_step", headline_variants, 20), ("occupancy_step", occupancy_variants, 40)):
        variants = make()
        for fn in variants.values():                        # every variant warms up its own shapes and workspaces first
            timed(fn, 5)
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                times[k].append(timed(fn, calls))
        row = {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for k, t in times.items()}
        result["cases"][name] = row
        print(name + ": " + "; ".join("%s %.4f ms (%.4f .. %.4f) x%.3f" % (k, r["median_ms"], r["min_ms"], r["max_ms"], r["median_ms"] / row["off"]["median_ms"])
                                      for k, r in row.items()), flush=True)
    print(json.dumps(result), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
