"""Generates tests/golden/eff_distloss.npz from the reference's `loss.eff_distloss(w, m, interval)` on the CPU (float64).

    python tests/golden/make_golden_distortion.py <path of the reference checkout>      (or FOCNERF_REFERENCE=<path>)

Run where the reference lies; no test runs this. Nothing of the reference is copied: the fixture holds data only — per case the inputs
w, m [B,N], the interval ([B,N], or a scalar stored as a 0-d array), the loss (the reference's mean over the B rays) and the gradient of
the loss with respect to w for grad_output = 1. tests/test_distortion_ref.py compares the float64 reference of the tail kernels'
per-ray distortion (tests/distortion_ref.py), times 1 / B, and focnerf_amd.loss.ray_distortion against it.
"""
import os
import sys

import numpy as np
import torch

# (B, N, interval form, seed): one sample, a handful, a 64-sample step and its neighbours; weights of a composite (they sum to < 1)
CASES = [(1, 1, "tensor", 0), (2, 2, "scalar", 1), (3, 7, "tensor", 2), (2, 64, "tensor", 3), (2, 65, "scalar", 4), (1, 129, "tensor", 5)]


def draw(B, N, form, seed):
    rng = np.random.default_rng(seed)
    interval = rng.uniform(1e-3, 5e-2, (B, N))
    if form == "scalar":
        interval = np.full((B, N), 1.0 / N)
    edges = np.concatenate([np.zeros((B, 1)), np.cumsum(interval, -1)], -1) + rng.uniform(0.0, 0.5, (B, 1))
    m = 0.5 * (edges[:, 1:] + edges[:, :-1])
    alpha = rng.uniform(0.0, 0.3, (B, N)) * (rng.random((B, N)) < 0.8)
    w = alpha * np.cumprod(np.concatenate([np.ones((B, 1)), 1 - alpha[:, :-1]], -1), -1)
    return w, m, (np.float64(1.0 / N) if form == "scalar" else interval)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FOCNERF_REFERENCE")
    if not ref or not os.path.exists(os.path.join(ref, "loss.py")):
        raise SystemExit(__doc__)
    sys.path.insert(0, ref)
    from loss import eff_distloss
    out = {"n_cases": np.int64(len(CASES))}
    for k, (B, N, form, seed) in enumerate(CASES):
        w, m, interval = draw(B, N, form, seed)
        wt = torch.tensor(w, requires_grad=True)
        loss = eff_distloss(wt, torch.tensor(m), torch.tensor(interval) if form == "tensor" else float(interval))
        grad, = torch.autograd.grad(loss, wt)
        out.update({f"w{k}": w, f"m{k}": m, f"interval{k}": np.asarray(interval), f"loss{k}": loss.detach().numpy(), f"grad{k}": grad.numpy()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "eff_distloss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
