"""The optimizer step on the headline parameter set (bench.py's configs[1] model, bound 1) with seeded grads, three legs alternating in
one process: (a) torch.optim.Adam(fused=True) under torch's GradScaler (step + update) — the baseline; (b) focnerf_amd.FusedAdam under
torch's GradScaler; (c) FusedAdam.step(scaler=LossScaler). Per leg: the median over the rounds of the time per step (device events
around a window of steps), the kernels one step launches (torch's profiler, a run of its own), the bytes the leg's algorithm moves over
that time; then the same three legs inside bench.train_step as ms per step. One JSON line.

usage: python tools/time_optimizer.py [--rounds 9] [--window 50] [--step-rounds 5] [--step-window 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import FusedAdam, LossScaler  # noqa: E402

LR, BETAS, EPS = 1e-2, (0.9, 0.99), 1e-15
LEGS = ("torch_adam_gradscaler", "fusedadam_gradscaler", "fusedadam_lossscaler")


class _LossScalerInTrainStep:
    """bench.train_step's three scaler lines for route (c): scale(loss) as is, step(opt) = opt.step(scaler=...), update() = nothing."""

    def __init__(self, scaler):
        self.scaler = scaler

    def scale(self, loss):
        return self.scaler.scale(loss)

    def step(self, opt):
        return opt.step(scaler=self.scaler)

    def update(self):
        pass


def make_leg(leg, params):
    if leg == LEGS[0]:
        opt, sc = torch.optim.Adam(params, betas=BETAS, eps=EPS, fused=True), torch.amp.GradScaler("cuda")
    elif leg == LEGS[1]:
        opt, sc = FusedAdam(params, betas=BETAS, eps=EPS), torch.amp.GradScaler("cuda")
    else:
        opt, sc = FusedAdam(params, betas=BETAS, eps=EPS), _LossScalerInTrainStep(LossScaler())
    return opt, sc


def window_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1000.0 * s.elapsed_time(e) / n


def count_launches(fn):
    """Kernels one call enqueues, from torch's profiler; None where the profiler reports no device activity on this build."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA and not ev.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-window", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_optimizer.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)

    # ---- the optimizer step alone: three copies of the headline model's parameters, the same seeded scaled grads
    steps, scalers = {}, {}
    n_elements = n_tensors = 0
    for leg in LEGS:
        model = bench.build_model(1, dev, seed=0).train()
        groups = [dict(g, params=list(g["params"])) for g in model.get_params(LR)]
        params = [p for g in groups for p in g["params"]]
        n_elements, n_tensors = sum(p.numel() for p in params), len(params)
        opt, sc = make_leg(leg, groups)
        scale = float(sc.scaler.get_scale() if isinstance(sc, _LossScalerInTrainStep) else 65536.0)
        g0 = torch.Generator().manual_seed(1)
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g0) * 1e-3 * scale).to(dev)
        sc.scale(torch.zeros((), device=dev))

        def one(opt=opt, sc=sc):
            sc.step(opt)
            sc.update()
        steps[leg] = one
    for _ in range(20):                                          # warm-up: state, workspaces, code objects, clocks
        for leg in LEGS:
            steps[leg]()
    torch.cuda.synchronize()
    samples = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            samples[leg].append(window_us(steps[leg], args.window))
    # floats per element the leg's algorithm moves: Adam reads p, g, m, v and writes p, m, v (7); torch's inf check reads AND rewrites the
    # grads (g * 1.0 in place: 2), the library's check reads them (1)
    floats = {LEGS[0]: 9, LEGS[1]: 9, LEGS[2]: 8}
    result = {"tool": "time_optimizer", "device": torch.cuda.get_device_name(0), "n_tensors": n_tensors, "n_elements": n_elements,
              "rounds": args.rounds, "window": args.window, "optimizer_step": {}}
    for leg in LEGS:
        us = statistics.median(samples[leg])
        result["optimizer_step"][leg] = {"us": round(us, 2), "us_min": round(min(samples[leg]), 2), "us_max": round(max(samples[leg]), 2),
                                         "bytes": floats[leg] * 4 * n_elements, "TB_per_s": round(floats[leg] * 4 * n_elements / us * 1e-6, 3)}

    # ---- the same three legs inside the headline training step (bench.train_step, fused path)
    poses, intr = bench.make_training_rays(dev, 1, 8, seed=0)
    bgen = torch.Generator().manual_seed(1000)
    batches = [bench.sample_batch(poses, intr, dev, bgen) for _ in range(8)]
    train = {}
    for leg in LEGS:
        model = bench.build_model(1, dev, seed=0).train()
        opt, sc = make_leg(leg, model.get_params(LR))
        counter = [0]

        def one(model=model, opt=opt, sc=sc, counter=counter):
            bench.train_step(model, opt, sc, *batches[counter[0] % len(batches)], fused=True)
            counter[0] += 1
        train[leg], scalers[leg] = one, sc
    for _ in range(10):
        for leg in LEGS:
            train[leg]()
    torch.cuda.synchronize()
    tsamples = {leg: [] for leg in LEGS}
    for _ in range(args.step_rounds):
        for leg in LEGS:
            tsamples[leg].append(window_us(train[leg], args.step_window) / 1000.0)
    result["train_step_ms"] = {leg: {"ms": round(statistics.median(tsamples[leg]), 4), "ms_min": round(min(tsamples[leg]), 4),
                                     "ms_max": round(max(tsamples[leg]), 4)} for leg in LEGS}
    # a step the scaler skips is a cheaper step: the legs are comparable when their scales have settled at the same value
    result["train_step_scale_end"] = {leg: float((sc.scaler if isinstance(sc, _LossScalerInTrainStep) else sc).get_scale()) for leg, sc in scalers.items()}
    result["baseline"] = LEGS[0]
    for leg in LEGS:                                             # last: the profiler slows the host, no timing runs after it
        n = count_launches(steps[leg])
        result["optimizer_step"][leg]["launches"] = n if n is not None else "not measured"
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
