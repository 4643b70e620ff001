"""The parameter EMA on the headline parameter set (bench.py's configs[1] model, bound 1) with seeded grads, four legs alternating in one
process: (a) FusedAdam.step(scaler=LossScaler) followed by torch_ema's update, three torch ops and a temporary per tensor — what the
reference does after every step; (b) FusedAdam.step(scaler=LossScaler, ema=ParameterEMA), the EMA inside the update launch; (c) the step
without an EMA; (d) the bare ParameterEMA.update(). Per leg: the median over the rounds of the time per call (device events around a
window of calls), its minimum and maximum. `spread_us`: the larger max - min of (a) and (b); (b) beats (a) when the medians differ by more
than that. (b) - (c), the cost of the EMA in the step, stands beside the traffic estimate it should track: the shadow's read and write
are 2 floats per element on top of the update's 7, so 2 / 7 of (c). One JSON line.

usage: python tools/time_ema.py [--rounds 9] [--window 50]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import FusedAdam, LossScaler, ParameterEMA  # noqa: E402

LR, BETAS, EPS, DECAY = 1e-2, (0.9, 0.99), 1e-15, 0.95
LEGS = ("step_then_torch_ema", "step_with_ema", "step_alone", "ema_update_alone")


class _TorchEma:
    """torch_ema 0.3's update: the count and the decay on the host, three torch ops per tensor."""

    def __init__(self, params, decay):
        self.params, self.decay, self.num_updates = params, decay, 0
        self.shadow_params = [p.clone().detach() for p in params]

    def update(self):
        self.num_updates += 1
        one_minus_decay = 1.0 - min(self.decay, (1 + self.num_updates) / (10 + self.num_updates))
        with torch.no_grad():
            for s, p in zip(self.shadow_params, self.params):
                tmp = s - p
                tmp.mul_(one_minus_decay)
                s.sub_(tmp)


def window_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1000.0 * s.elapsed_time(e) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=int, default=50)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ema.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)

    calls = {}
    n_elements = n_tensors = 0
    for leg in LEGS:                                             # a copy of the headline model's parameters per leg, the same seeded scaled grads
        model = bench.build_model(1, dev, seed=0).train()
        groups = [dict(g, params=list(g["params"])) for g in model.get_params(LR)]
        params = [p for g in groups for p in g["params"]]
        n_elements, n_tensors = sum(p.numel() for p in params), len(params)
        opt, scaler = FusedAdam(groups, betas=BETAS, eps=EPS), LossScaler()
        g0 = torch.Generator().manual_seed(1)
        for p in params:
            p.grad = (torch.randn(p.shape, generator=g0) * 1e-3 * scaler.get_scale()).to(dev)
        ema = _TorchEma(params, DECAY) if leg == LEGS[0] else ParameterEMA(params, DECAY)
        if leg == LEGS[0]:
            def one(opt=opt, scaler=scaler, ema=ema):
                opt.step(scaler=scaler)
                ema.update()
        elif leg == LEGS[1]:
            def one(opt=opt, scaler=scaler, ema=ema):
                opt.step(scaler=scaler, ema=ema)
        elif leg == LEGS[2]:
            def one(opt=opt, scaler=scaler):
                opt.step(scaler=scaler)
        else:
            def one(ema=ema):
                ema.update()
        calls[leg] = (one, model)
    for _ in range(20):                                          # warm-up: state, workspaces, code objects, clocks
        for leg in LEGS:
            calls[leg][0]()
    torch.cuda.synchronize()
    samples = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            samples[leg].append(window_us(calls[leg][0], args.window))

    # floats per element each leg's algorithm moves: the check reads g (1), Adam reads p, g, m, v and writes p, m, v (7), the shadow is
    # read and written (2); torch_ema's three ops read s, p, write tmp; read and write tmp; read s, tmp, write s (8); the bare update 3
    floats = {LEGS[0]: 8 + 8, LEGS[1]: 8 + 2, LEGS[2]: 8, LEGS[3]: 3}
    us = {leg: statistics.median(samples[leg]) for leg in LEGS}
    result = {"tool": "time_ema", "device": torch.cuda.get_device_name(0), "n_tensors": n_tensors, "n_elements": n_elements,
              "rounds": args.rounds, "window": args.window, "legs": {}}
    for leg in LEGS:
        result["legs"][leg] = {"us": round(us[leg], 2), "us_min": round(min(samples[leg]), 2), "us_max": round(max(samples[leg]), 2),
                               "bytes": floats[leg] * 4 * n_elements, "TB_per_s": round(floats[leg] * 4 * n_elements / us[leg] * 1e-6, 3)}
    spread = max(max(samples[leg]) - min(samples[leg]) for leg in LEGS[:2])
    result["spread_us"] = round(spread, 2)
    result["with_ema_faster_than_torch_ema_by_us"] = round(us[LEGS[0]] - us[LEGS[1]], 2)
    result["with_ema_beats_torch_ema_beyond_spread"] = bool(us[LEGS[0]] - us[LEGS[1]] > spread)
    result["ema_cost_in_step_us"] = round(us[LEGS[1]] - us[LEGS[2]], 2)
    result["ema_cost_traffic_estimate_us"] = round(us[LEGS[2]] * 2.0 / 7.0, 2)      # the shadow's 2 floats per element on the update's 7, as a share of (c)
    result["ema_bytes"] = 2 * 4 * n_elements
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
