"""Scoring one combined view at 800 x 800 with two backgrounds: focnerf_amd.score.score_view against the host route a user has without
it. Run on the GPU box; prints one JSON line, milliseconds:

    device_ms        the two launches of score_view (score_raw: quantise, then SSIM and squared error), by device events around a
                     batch of BATCH back-to-back calls, per call; the median of REPS batches after WARMUP (a single call is too
                     short to time on its own)
    score_view_ms    score_view as a user calls it: launches, the read of its [B,4] result and the host arithmetic; a host clock around
                     work that ends in that read, median of REPS after WARMUP
    host_route_ms    the copy of image4, depth and gt to the host plus the float64 statement (quantise, PSNR, SSIM for both
                     backgrounds) with `host_filter`: scipy.ndimage.gaussian_filter when scipy imports, the filter of
                     tests/metrics_ref.py otherwise; host clock, median of HOST_REPS after one warm-up
    host_copy_ms     the copy alone
    agree            the two routes' byte images equal, SSIM within 1e-9, PSNR within 1e-9 dB on the timed inputs
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import metrics_ref  # noqa: E402
from focnerf_amd import score  # noqa: E402

WARMUP, REPS, BATCH, HOST_REPS = 3, 9, 20, 3

try:
    from scipy.ndimage import gaussian_filter as _scipy_filter
    HOST_FILTER = "scipy.ndimage.gaussian_filter"
    metrics_ref.gaussian_filter = lambda a, sigma: _scipy_filter(a, sigma)      # the statement's flow, the reference's own filter
except ImportError:
    HOST_FILTER = "tests/metrics_ref.py"


def make_view(H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    N = H * W
    colour, alpha = torch.rand(N, 3, generator=g), (torch.rand(N, 1, generator=g) * 1.6 - 0.3).clamp(0, 1)
    image4 = torch.stack([torch.cat([(colour * alpha + bg * (1 - alpha)).clamp(0, 1), alpha], -1) for bg in (1.0, 0.0)])
    gt = torch.cat([(colour + 0.05 * torch.randn(N, 3, generator=g)).clamp(0, 1), (torch.rand(N, 1, generator=g) < 0.7).float()], -1)
    return image4.to(dev), torch.rand(N, generator=g).to(dev), gt.view(H, W, 4).to(dev)


def host_route(image4, depth, gt, H, W):
    a, d, g = image4.cpu().numpy(), depth.cpu().numpy(), gt.cpu().numpy()
    return metrics_ref.score(a, d, g, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=800)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_score.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    H, W = args.height, args.width
    image4, depth, gt = make_view(H, W, dev)
    out = {"H": H, "W": W, "B": 2, "warmup": WARMUP, "reps": REPS, "batch": BATCH, "host_reps": HOST_REPS, "host_filter": HOST_FILTER}

    batches = []
    for rep in range(WARMUP + REPS):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(BATCH):
            score.score_raw(image4, depth, gt, H, W)
        stop.record()
        stop.synchronize()
        if rep >= WARMUP:
            batches.append(start.elapsed_time(stop) / BATCH)
    out["device_ms"], out["device_ms_all"] = statistics.median(batches), batches

    calls = []
    for rep in range(WARMUP + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = score.score_view(image4, depth, gt, H, W)
        if rep >= WARMUP:
            calls.append((time.perf_counter() - t0) * 1e3)
    out["score_view_ms"], out["score_view_ms_all"] = statistics.median(calls), calls

    host, copies = [], []
    for rep in range(1 + HOST_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = host_route(image4, depth, gt, H, W)
        if rep >= 1:
            host.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        image4.cpu(), depth.cpu(), gt.cpu()
        if rep >= 1:
            copies.append((time.perf_counter() - t0) * 1e3)
    out["host_route_ms"], out["host_route_ms_all"] = statistics.median(host), host
    out["host_copy_ms"] = statistics.median(copies)

    out["psnr"], out["ssim"] = s.psnr, s.ssim
    out["agree"] = bool(np.array_equal(s.rgba_u8.cpu().numpy(), ref["rgba_u8"]) and np.array_equal(s.gt_u8.cpu().numpy(), ref["gt_u8"])
                        and np.array_equal(s.depth_u8.cpu().numpy(), ref["depth_u8"])
                        and max(abs(a - b) for a, b in zip(s.ssim, ref["ssim"])) <= 1e-9 and max(abs(a - b) for a, b in zip(s.psnr, ref["psnr"])) <= 1e-9)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
