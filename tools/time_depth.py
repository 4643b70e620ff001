"""What the differentiable depth of the occupancy-grid training step costs, and what the one-call route does for the distortion: the
configs[2] occupancy step (bench.py's occupancy leg) with the keywords off, with depth_grad=True, with distortion=True and with both,
alternating round by round in ONE process on the same inputs (whatever else the box is doing falls on all of them). Per variant: the median
of the rounds and their spread (min .. max); times are device events around a block of steps. `--variants off,dist` restricts the set, so
that the same file runs in a tree without the depth keyword; `depth_key_only` (not in the default set) is the keyword without a loss term on
the depth (the backward then receives no grad_depth and runs the kernel without the depth term). Run on the GPU box:

    python tools/time_depth.py [--rounds 5] [--variants off,depth,dist,both] [--json out.json]
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


def _setup():
    m = bench.build_model(2, dev, cuda_ray=True, seed=0).train()
    opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
    sc = torch.amp.GradScaler("cuda")
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=0)
    gen = torch.Generator().manual_seed(0)
    return m, opt, sc, [bench.sample_batch(poses, intr, dev, gen) for _ in range(4)]


def _step(m, opt, sc, batch, depth, distortion, depth_term=True):
    """bench.cuda_ray_train_step with the keywords and lambda * (mse(depth, 1/2) + mean(distortion)) in the loss; depth_term=False: the
    depth keyword without its loss term (the term's own torch kernels, forward and backward, are part of the `depth` figure)."""
    rays_o, rays_d, target = batch
    opt.zero_grad(set_to_none=True)
    kw = dict(force_all_rays=False, dt_gamma=1 / 128, max_steps=1024)
    if depth:
        kw["depth_grad"] = True
    if distortion:
        kw["distortion"] = True
    with torch.autocast("cuda", dtype=torch.float16):
        out = m.render(rays_o, rays_d, staged=False, perturb=True, bg_color=None, **kw)
        loss = torch.nn.functional.mse_loss(out["image"], target)
        if depth and depth_term:
            loss = loss + LAMBDA * torch.mean((out["depth"] - 0.5) ** 2)
        if distortion:
            loss = loss + LAMBDA * out["distortion"].mean()
    sc.scale(loss).backward()
    sc.step(opt)
    sc.update()


VARIANTS = {"off": (False, False), "depth": (True, False), "dist": (False, True), "both": (True, True), "depth_key_only": (True, False, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--variants", default="off,depth,dist,both")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    m, opt, sc, batches = _setup()
    for i in range(17):                                     # bench.py's occupancy leg: the sample budget comes from the first 16 marches
        _step(m, opt, sc, batches[i % 4], False, False)
        if i == 15:
            m.mean_count = int(m.step_counter[:16, 0].sum().item() / 16)
    variants = {k: (lambda i, _f=VARIANTS[k]: _step(m, opt, sc, batches[i % 4], *_f)) for k in args.variants.split(",")}
    for fn in variants.values():                            # every variant warms up its own shapes and workspaces first
        timed(fn, 5)
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, 40))
    row = {k: {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)} for k, t in times.items()}
    first = next(iter(row.values()))["median_ms"]
    print("occupancy_step: " + "; ".join("%s %.4f ms (%.4f .. %.4f) x%.3f" % (k, r["median_ms"], r["min_ms"], r["max_ms"], r["median_ms"] / first)
                                         for k, r in row.items()), flush=True)
    result = {"rounds": args.rounds, "lambda": LAMBDA, "occupancy_step": row}
    print(json.dumps(result), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
