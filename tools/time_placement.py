"""Unplaced against placed occupancy-culled `render_field4` for ONE object over an 800 x 800 x 512 view, in chunks of 16384 rays: what
`placement=` costs a rank of the combined render per object per view. The object is the analytic sphere grid in a box of bound 1
(synthetic.analytic_density_grid installed with set_density_grid); the scene's box has bound 2 and the camera stands at radius 4,
outside both. Run on the GPU box; prints one JSON line:

    unplaced              the object in its own box: render_field4(..., occupancy=occ)                       (samples span the object's box)
    identity_own_box      placement=Placement(), scene_aabb = the object's box: the SAME samples as `unplaced`, through the placed
                          entry points — the transform, the inside test and the gain on an unchanged workload
    identity_scene        placement=Placement(), scene_aabb = the scene's box                                 (samples span the scene's box)
    general_scene         37 degrees about (1, 2, 3), translation (0.6, 0.2, -0.4), scale 0.5, in the scene's box
    *_ms                  milliseconds per view, median of 5 timed views after 1 warm-up view, device events around the whole view;
                          the forms are walked twice in one process (`*_ms_again`) so that none owes its number to its place in the run
    *_share               occupied samples / (rays x 512) over the view

`--unplaced-only` times the unplaced form alone and imports nothing this tool's commit added; `--tree DIR` takes the package (and its
built library) from another checkout. The control for the existing path is this mode run alternately on this checkout and on a
checkout of the parent commit on the same box (the parent's library lacks the placed entry points, so the binding of this checkout
refuses to load it through FOCNERF_LIB_PATH: the parent runs as a whole)."""
import argparse
import json
import os
import statistics
import sys

import torch

SIDE, T, CHUNK, WARMUP, VIEWS = 800, 512, 16384, 1, 5
SCENE_BOUND, RADIUS = 2.0, 4.0


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
    ap.add_argument("--unplaced-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import bench
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.field import half_cache_scope
    from focnerf_amd.fixedcull import Occupancy, fixed_cull
    from focnerf_amd.fixedstep import render_field4
    assert torch.cuda.is_available(), "time_placement.py measures on the GPU; there is no CPU fallback"
    assert (bench.VIEW, bench.NUM_STEPS) == (SIDE, T)
    dev = torch.device("cuda", 0)
    model = bench.build_model(1, dev, cuda_ray=True, seed=0).eval()          # the sphere grid is installed by build_model
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    poses = synthetic.rand_poses(1, dev, radius=RADIUS, generator=torch.Generator().manual_seed(0))
    o, d = synthetic.get_rays(poses[:1], synthetic.intrinsics(SIDE, SIDE), SIDE, SIDE)
    o, d = o[0].contiguous(), d[0].contiguous()
    n = o.shape[0]
    buf = torch.empty(CHUNK, T, 4, dtype=torch.float32, device=dev)
    occ = Occupancy.of(model)
    out = {"view": [SIDE, SIDE, T], "chunk": CHUNK, "views_timed": VIEWS, "warmup_views": WARMUP, "tree": os.path.abspath(args.tree),
           "scene_bound": SCENE_BOUND, "object_bound": float(model.bound), "camera_radius": RADIUS}
    forms = {"unplaced": lambda lo, hi: render_field4(model, o[lo:hi], d[lo:hi], num_steps=T, out=buf[: hi - lo], occupancy=occ)}
    boxes = {"unplaced": (model.aabb_infer, None)}
    if not args.unplaced_only:
        from focnerf_amd import Placement
        scene = torch.tensor([-SCENE_BOUND] * 3 + [SCENE_BOUND] * 3, dtype=torch.float32, device=dev)
        general = Placement.rotated((1, 2, 3), 37, translation=(0.6, 0.2, -0.4), scale=0.5)
        for name, P, box in (("identity_own_box", Placement(), model.aabb_infer), ("identity_scene", Placement(), scene), ("general_scene", general, scene)):
            forms[name] = (lambda lo, hi, P=P, box=box: render_field4(model, o[lo:hi], d[lo:hi], num_steps=T, out=buf[: hi - lo], occupancy=occ,
                                                                      placement=P, scene_aabb=box))
            boxes[name] = (box, P)
    with torch.no_grad(), half_cache_scope():
        for suffix in ("_ms", "_ms_again"):
            for name, fn in forms.items():
                out[name + suffix], all_ms = time_view(fn, n)
                if suffix == "_ms":
                    out[name + "_ms_all"] = all_ms
        for name, (box, P) in boxes.items():
            nears, fars = raymarching.near_far_from_aabb(o, d, box, model.min_near)
            occupied = 0
            for lo in range(0, n, CHUNK):
                hi = min(lo + CHUNK, n)
                rays = (o[lo:hi], d[lo:hi], nears[lo:hi], fars[lo:hi], box, T, occ)
                count = fixed_cull(*rays) if P is None else fixed_cull(*rays, placement=P, obj_aabb=model.aabb_infer)
                occupied += int(count[2].item())
            out[name + "_share"] = occupied / (n * T)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
