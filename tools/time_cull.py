"""Dense against occupancy-culled `render_field4` for ONE object over an 800 x 800 x 512 view of the analytic sphere scene
(synthetic.analytic_density_grid installed with set_density_grid, the scene of bench.py's occupancy legs), in chunks of 16384 rays:
what a rank of the combined render spends per object per view. Run on the GPU box; prints one JSON line:

    dense_ms / culled_ms   milliseconds per view, median of 5 timed views after 1 warm-up view, device events around the whole view
    occupied_share         occupied samples / (rays x 512) over the view
    image_delta            max and mean |difference| of the composited image (combine_packed, backgrounds 1 and 0) between the two
    own_grid               culled_ms / occupied_share / image_delta with a grid estimated from the network's own density instead

`--dense-only` times the dense path alone and imports nothing this tool's commit added: copy the file into a checkout of an earlier
commit (with its library built) and run it there on the same box to compare the dense path across commits, alternating the runs
like tools/ab_libs.sh does."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import raymarching, synthetic  # noqa: E402
from focnerf_amd.field import half_cache_scope  # noqa: E402
from focnerf_amd.fixedstep import render_field4  # noqa: E402

SIDE, T, CHUNK, WARMUP, VIEWS = bench.VIEW, bench.NUM_STEPS, 16384, 1, 5      # 800 x 800 x 512


def time_view(fn, n):
    """Median milliseconds of VIEWS walks of the view's chunks after WARMUP, each between two device events."""
    times = []
    for rep in range(WARMUP + VIEWS):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for lo in range(0, n, CHUNK):
            fn(lo, min(lo + CHUNK, n))
        end.record()
        end.synchronize()
        if rep >= WARMUP:
            times.append(start.elapsed_time(end))
    return statistics.median(times), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense-only", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_cull.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    model = bench.build_model(1, dev, cuda_ray=True, seed=0).eval()          # the sphere grid is installed by build_model
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    poses, intr = bench.make_training_rays(dev, 1, 8, seed=0)
    o, d = synthetic.get_rays(poses[:1], intr, SIDE, SIDE)
    o, d = o[0].contiguous(), d[0].contiguous()
    n = o.shape[0]
    buf = torch.empty(CHUNK, T, 4, dtype=torch.float32, device=dev)
    out = {"view": [SIDE, SIDE, T], "chunk": CHUNK, "views_timed": VIEWS, "warmup_views": WARMUP}
    with torch.no_grad(), half_cache_scope():
        dense = lambda lo, hi: render_field4(model, o[lo:hi], d[lo:hi], num_steps=T, out=buf[: hi - lo])
        out["dense_ms"], out["dense_ms_all"] = time_view(dense, n)
        if not args.dense_only:
            from focnerf_amd.combine import combine_packed
            from focnerf_amd.fixedcull import Occupancy, fixed_cull
            occ = Occupancy.of(model)
            culled = lambda lo, hi: render_field4(model, o[lo:hi], d[lo:hi], num_steps=T, out=buf[: hi - lo], occupancy=occ)
            # alternate the two once more so that neither owes its number to its place in the run
            out["culled_ms"], out["culled_ms_all"] = time_view(culled, n)
            out["dense_ms_again"], _ = time_view(dense, n)
            out["culled_ms_again"], _ = time_view(culled, n)
            nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_infer, model.min_near)

            def share_and_delta(oc, fn):
                occupied, dmax, dsum = 0, 0.0, 0.0
                for lo in range(0, n, CHUNK):
                    hi = min(lo + CHUNK, n)
                    occupied += int(fixed_cull(o[lo:hi], d[lo:hi], nears[lo:hi], fars[lo:hi], model.aabb_infer, T, oc)[2].item())
                    img_d = combine_packed([dense(lo, hi)], nears[lo:hi], fars[lo:hi], (1.0, 0.0))[0]
                    img_c = combine_packed([fn(lo, hi)], nears[lo:hi], fars[lo:hi], (1.0, 0.0))[0]
                    delta = (img_d[..., :3] - img_c[..., :3]).abs()
                    dmax, dsum = max(dmax, float(delta.max())), dsum + float(delta.sum())
                return occupied / (n * T), {"max": dmax, "mean": dsum / (2 * n * 3)}
            out["occupied_share"], out["image_delta"] = share_and_delta(occ, culled)
            out["speedup"] = out["dense_ms"] / out["culled_ms"]
            # The scene's network is untrained: its density has nothing to do with the analytic sphere, so image_delta above measures that
            # mismatch. The same figures with a grid estimated from the network's OWN density (Occupancy.estimate, cell centres) show what
            # the approximation itself costs on this network.
            own = Occupancy.estimate(model, jitter=False)
            culled_own = lambda lo, hi: render_field4(model, o[lo:hi], d[lo:hi], num_steps=T, out=buf[: hi - lo], occupancy=own)
            ms, _ = time_view(culled_own, n)
            share, delta = share_and_delta(own, culled_own)
            out["own_grid"] = {"culled_ms": ms, "occupied_share": share, "image_delta": delta}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
