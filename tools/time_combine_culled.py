"""The combined render of placed, occupancy-culled objects on ONE device, with and without the objects' dense fields, over an
800 x 800 x 512 view in chunks of 16384 rays. The scene is tools/time_placement.py's: the analytic sphere grid in a box of bound 1 (an
untrained network), the scene's box of bound 2, the camera at radius 4. Run on the GPU box; prints one JSON line:

    packed_*      today's path: combine.placed_field_fns (cull -> host read -> emit -> field -> culled pack into a [chunk,512,4] buffer per
                  object), then combine.combine_packed over the K buffers
    culled_*      combine.render_scene_culled: the same up to the pack, then foc_combine_select_composite_culled on the compact lists
    *_1           one object: 37 degrees about (1, 2, 3), translation (0.6, 0.2, -0.4), scale 0.5
    *_3           three: that one, the identity, and translation (-0.9, 0.3, 0.5) at scale 0.75
    *_empty       one object whose occupancy grid is all zero: the floor of a view in which nothing is occupied
    *_ms          milliseconds per view, median of 5 timed views after 1 warm-up view, device events around the whole view (near / far of the
                  view included, both variants); the variants alternate and are walked twice in one process (`*_ms_again`);
                  `*_ms_all`: the five views of the first walk
    share_*       occupied samples / (objects x rays x 512) over the view

`--packed-only` times today's path alone and imports nothing this tool's commit added; `--tree DIR` takes the package (and its built
library) from another checkout: the control is this mode run alternately on this checkout and on a checkout of the parent commit."""
import argparse
import json
import os
import statistics
import sys

import torch

SIDE, T, CHUNK, WARMUP, VIEWS = 800, 512, 16384, 1, 5
SCENE_BOUND, RADIUS = 2.0, 4.0


def time_view(fn):
    """Median milliseconds of VIEWS calls of fn() after WARMUP, each between two device events."""
    times = []
    for rep in range(WARMUP + VIEWS):
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
    ap.add_argument("--packed-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    from focnerf_amd import Placement, combine, synthetic
    from focnerf_amd.field import half_cache_scope
    from focnerf_amd.fixedcull import Occupancy, fixed_cull
    assert torch.cuda.is_available(), "time_combine_culled.py measures on the GPU; there is no CPU fallback"
    assert (bench.VIEW, bench.NUM_STEPS) == (SIDE, T)
    dev = torch.device("cuda", 0)
    model = bench.build_model(1, dev, cuda_ray=True, seed=0).eval()          # the sphere grid is installed by build_model
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    poses = synthetic.rand_poses(1, dev, radius=RADIUS, generator=torch.Generator().manual_seed(0))
    o, d = synthetic.get_rays(poses[:1], synthetic.intrinsics(SIDE, SIDE), SIDE, SIDE)
    o, d = o[0].contiguous(), d[0].contiguous()
    n = o.shape[0]
    occ = Occupancy.of(model)
    nothing = Occupancy(torch.zeros_like(occ.bitfield), occ.cascade, occ.grid_size, occ.bound)
    scene = torch.tensor([-SCENE_BOUND] * 3 + [SCENE_BOUND] * 3, dtype=torch.float32, device=dev)
    general = Placement.rotated((1, 2, 3), 37, translation=(0.6, 0.2, -0.4), scale=0.5)
    scenes = {"1": ([occ], [general]), "3": ([occ] * 3, [general, Placement(), Placement(translation=(-0.9, 0.3, 0.5), scale=0.75)]),
              "empty": ([nothing], [general])}
    bufs = [torch.empty(CHUNK, T, 4, dtype=torch.float32, device=dev) for _ in range(3)]
    out = {"view": [SIDE, SIDE, T], "chunk": CHUNK, "views_timed": VIEWS, "warmup_views": WARMUP, "tree": os.path.abspath(args.tree),
           "scene_bound": SCENE_BOUND, "object_bound": float(model.bound), "camera_radius": RADIUS}

    def packed(occs, places):
        fns, nears, fars = combine.placed_field_fns([model] * len(occs), occs, places, o, d, T, scene)
        image4 = torch.empty(2, n, 4, dtype=torch.float32, device=dev)
        depth = torch.empty(n, dtype=torch.float32, device=dev)
        for lo in range(0, n, CHUNK):
            hi = min(lo + CHUNK, n)
            fields = [fn(lo, hi, buf[: hi - lo]) for fn, buf in zip(fns, bufs)]
            image4[:, lo:hi], depth[lo:hi] = combine.combine_packed(fields, nears[lo:hi], fars[lo:hi], (1.0, 0.0))
        return image4, depth

    def culled(occs, places):
        return combine.render_scene_culled([model] * len(occs), occs, places, o, d, T, scene, (1.0, 0.0), CHUNK)

    variants = {"packed": packed} if args.packed_only else {"packed": packed, "culled": culled}
    with torch.no_grad(), half_cache_scope():
        for suffix in ("_ms", "_ms_again"):
            for sname, (occs, places) in scenes.items():
                for vname, fn in variants.items():
                    key = f"{vname}_{sname}"
                    out[key + suffix], all_ms = time_view(lambda: fn(occs, places))
                    if suffix == "_ms":
                        out[key + "_ms_all"] = all_ms
        for sname, (occs, places) in scenes.items():
            if not args.packed_only:                                     # the two variants render the same view
                a, b = packed(occs, places), culled(occs, places)
                out[f"equal_{sname}"] = bool(torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
            _, nears, fars = combine.placed_field_fns([model] * len(occs), occs, places, o, d, T, scene)
            occupied = 0
            for oc, P in zip(occs, places):
                for lo in range(0, n, CHUNK):
                    hi = min(lo + CHUNK, n)
                    occupied += int(fixed_cull(o[lo:hi], d[lo:hi], nears[lo:hi], fars[lo:hi], scene, T, oc, placement=P, obj_aabb=model.aabb_infer)[2].item())
            out[f"share_{sname}"] = occupied / (len(occs) * n * T)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
