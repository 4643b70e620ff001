"""What attribution costs in the fused combine: `select_composite` against `select_composite_attr` on one 16384 x 512 piece (the
combiner's default `max_ray_batch` at the workload's sample count) with K = 4, 8 and 16 objects — the three instantiations of the
attribution kernel — alternated in ONE process. Run on the GPU box; prints one JSON line:

    K<k>.plain_ms / attr_ms     median of 5 launches after a warm-up launch, device events around each launch; the pair is walked twice
                                (..._again) so that neither owes its number to its place in the run
    K<k>.ratio                  attr_ms / plain_ms
    K<k>.field_bytes            bytes of packed fields one launch reads (K x 16384 x 512 x 16)

`--plain-only` times `select_composite` alone and calls nothing this tool's commit added: with FOCNERF_LIB_PATH pointing at a library
built from an earlier commit it times that commit's kernel on the same box (alternate the two libraries like tools/ab_libs.sh does)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from focnerf_amd.combine import HipCombineOps  # noqa: E402

N, T, WARMUP, REPS = 16384, 512, 1, 5


def time_launch(fn):
    times = []
    for rep in range(WARMUP + REPS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        if rep >= WARMUP:
            times.append(start.elapsed_time(end))
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--objects", type=int, nargs="+", default=[4, 8, 16])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_attribution.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    nears = torch.rand(N, device=dev, generator=g) * 0.5 + 0.2
    fars = nears + torch.rand(N, device=dev, generator=g) * 2 + 0.5
    out = {"rays": N, "samples": T, "launches_timed": REPS, "warmup_launches": WARMUP}
    fields = []
    for K in sorted(args.objects):
        while len(fields) < K:                                            # 537 MB per object: the fields of the smaller K are reused
            f = torch.rand(N, T, 4, device=dev, generator=g)
            f[..., 0] = f[..., 0] ** 4 * 40 * (torch.rand(N, T, device=dev, generator=g) < 0.5)
            fields.append(f)
        fs = fields[:K]
        plain = lambda: HipCombineOps.select_composite(fs, nears, fars, (1.0, 0.0))
        row = {"field_bytes": K * N * T * 16}
        row["plain_ms"], row["plain_ms_all"] = time_launch(plain)
        if not args.plain_only:
            attr = lambda: HipCombineOps.select_composite_attr(fs, nears, fars, (1.0, 0.0), K)
            row["attr_ms"], row["attr_ms_all"] = time_launch(attr)
            row["plain_ms_again"], _ = time_launch(plain)
            row["attr_ms_again"], _ = time_launch(attr)
            row["ratio"] = row["attr_ms"] / row["plain_ms"]
            a, b = plain(), attr()
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].nan_to_num(), b[1].nan_to_num()), "the two variants must render the same image"
        out[f"K{K}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
