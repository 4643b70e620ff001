"""What deterministic mode (FOC_DETERMINISTIC) costs: the grid backward alone at the benchmark's size, the headline step and the occupancy
step, each timed with the option off and on (and 2: the per-chunk-plane variant of the grid backward) in ONE process on the same inputs.
The modes alternate round by round, so that whatever else the box is doing falls on all of them; per mode: the median of the rounds and
their spread (min .. max). Times are device events around a block of calls. Run on the GPU box:

    python tools/time_deterministic.py [--rounds 7] [--modes 0,1,2] [--json out.json]

With FOCNERF_LIB_PATH pointing at another build of the library (tools/ab_libs.sh does the same) and --modes 0 the default path of two
builds can be compared by running the tool once per build, alternating."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import _lib  # noqa: E402
from focnerf_amd.backend import _gridencoder  # noqa: E402

OPT = "FOC_DETERMINISTIC"
dev = torch.device("cuda", 0)


def timed(fn, calls):
    """ms per call of `calls` back-to-back calls (device events)."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(calls):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls


def grid_backward_case(B=bench.NUM_RAYS * bench.NUM_STEPS):
    """The encoder backward of the headline step on its own: FOC's grid (16 levels, C 2, 2^19 rows, fp16), B uniform points, a seeded half gradient."""
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    enc = NeRFNetwork(bound=2, cuda_ray=False).to(dev).encoder
    L, C = enc.num_levels, enc.level_dim
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, 3, device=dev, generator=gen)
    g = (torch.randn(L, B, C, device=dev, generator=gen) * 0.1).half()
    emb = enc.embeddings.detach().half()
    ge = torch.zeros_like(emb)
    spec = enc.spec()
    S, H = spec.log2_scale, spec.base_resolution
    gridtype, ac, interp = spec.tail()

    def call(_):
        _gridencoder.grid_encode_backward(g, x, emb, enc.offsets, ge, B, 3, C, L, S, H, None, None, gridtype, ac, interp)
    return call


def headline_case():
    m = bench.build_model(2, dev, cuda_ray=False, seed=0).train()
    opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
    sc = torch.amp.GradScaler("cuda")
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=0)
    gen = torch.Generator().manual_seed(0)
    batches = [bench.sample_batch(poses, intr, dev, gen) for _ in range(4)]
    return lambda i: bench.train_step(m, opt, sc, *batches[i % 4], fused=True)


def occupancy_case():
    m = bench.build_model(2, dev, cuda_ray=True, seed=0).train()
    opt = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15, fused=True)
    sc = torch.amp.GradScaler("cuda")
    poses, intr = bench.make_training_rays(dev, 2, 8, seed=0)
    gen = torch.Generator().manual_seed(0)
    batches = [bench.sample_batch(poses, intr, dev, gen) for _ in range(4)]
    for i in range(17):                                     # bench.py's occupancy leg: the sample budget comes from the first 16 marches
        bench.cuda_ray_train_step(m, opt, sc, *batches[i % 4])
        if i == 15:
            m.mean_count = int(m.step_counter[:16, 0].sum().item() / 16)
    return lambda i: bench.cuda_ray_train_step(m, opt, sc, *batches[i % 4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--modes", default="0,1,2")
    ap.add_argument("--cases", default="grid_backward,headline_step,occupancy_step")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    modes = [int(v) for v in args.modes.split(",")]
    try:
        _lib.get_option(OPT)
        set_mode = lambda mode: _lib.set_option(OPT, mode)
    except RuntimeError:                                    # a build from before the option (an A/B against an older library): default path only
        assert modes == [0], f"{_lib.LIB_PATH} has no {OPT}: --modes 0"
        set_mode = lambda mode: None
    makers = {"grid_backward": (grid_backward_case, 20), "headline_step": (headline_case, 20), "occupancy_step": (occupancy_case, 40)}
    result = {"lib": _lib.LIB_PATH, "rounds": args.rounds, "cases": {}}
    for name in args.cases.split(","):
        make, calls = makers[name]
        fn = make()
        for mode in modes:                                  # every mode warms up its own shapes and workspaces first
            set_mode(mode)
            timed(fn, 5)
        times = {mode: [] for mode in modes}
        for _ in range(args.rounds):
            for mode in modes:
                set_mode(mode)
                times[mode].append(timed(fn, calls))
        set_mode(0)
        row = {}
        for mode in modes:
            t = times[mode]
            row[str(mode)] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t)}
        result["cases"][name] = row
        base = row[str(modes[0])]["median_ms"]
        parts = []
        for mode in modes:
            r = row[str(mode)]
            ratio = "" if mode == modes[0] else " x%.3f" % (r["median_ms"] / base)
            parts.append("%s=%d: %.4f ms (%.4f .. %.4f)%s" % (OPT, mode, r["median_ms"], r["min_ms"], r["max_ms"], ratio))
        print(name + ": " + "; ".join(parts), flush=True)
    print(json.dumps(result), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
