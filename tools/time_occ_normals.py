"""Surface normals on the occupancy-grid path (csrc/occrender.hip foc_occ_render_step_normals) against the colour view it rides on and the
fixed-step normal map, on an 800 x 800 view of tools/time_normals.py's scene: bench.py's network (bound 1, its analytic occupancy grid),
embeddings uniform in [-0.5, 0.5], a camera at radius 2. Run on the GPU box; prints one JSON line. Milliseconds are the median of REPS timed
calls after WARMUP (`*_all`: every repeat, the spread), a host clock around work that ends in a device synchronise. Child processes, each
under its own time limit; the parent never opens the GPU and starts nothing after a child that failed or ran out of time.

  colour   (a) run_cuda colour view, dt_gamma 0, max_steps 1024, T_thresh 1e-4 — one child per tree: this one, and with --parent-tree PATH a
           built checkout of the parent commit, alternated A B A B in one session as tools/ab_libs.sh alternates libraries (a whole tree,
           not FOCNERF_LIB_PATH: the binding is read from the header, and the parent's library lacks this commit's entry points).
           Expectation: no difference beyond the spread of the repeats; a difference means the composite's existing instantiations changed.
  normals  (b) normals="only"   (c) normals=True   (d) (a) followed by (b), the alternative to (c)   (e) render_normals, 512 fixed steps
           each twice, alternated (`*_again`); mean_angle_deg: between (b)'s and (e)'s normals over the pixels opaque (weights_sum > 0.5) in both.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 2, 7
SIDE = 800
KW = dict(dt_gamma=0, max_steps=1024, T_thresh=1e-4)
LIMIT = 300                                            # seconds per child


def timed(fn):
    import torch
    times = []
    for rep in range(WARMUP + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def _scene(tree=REPO):
    import torch
    sys.path.insert(0, tree)
    import bench
    from focnerf_amd import synthetic
    dev = torch.device("cuda", 0)
    model = bench.build_model(1, dev, cuda_ray=True, seed=0).eval()
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    poses = synthetic.rand_poses(1, dev, radius=2.0, generator=torch.Generator().manual_seed(0))
    o, d = synthetic.get_rays(poses[:1], synthetic.intrinsics(SIDE, SIDE), SIDE, SIDE)
    return model, o[0].contiguous(), d[0].contiguous()


def leg_colour(tree):
    import torch
    model, o, d = _scene(tree)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ms, every = timed(lambda: model.run_cuda(o, d, bg_color=1.0, **KW))
        image = model.run_cuda(o, d, bg_color=1.0, **KW)["image"]
    return {"colour_ms": ms, "colour_ms_all": every, "image_sum": float(image.double().sum()), "tree": "this" if tree == REPO else "parent"}


def leg_normals():
    import torch
    model, o, d = _scene()
    import focnerf_amd
    out = {"view": [SIDE, SIDE], "reps": REPS, "warmup": WARMUP}

    def colour_then_only():
        model.run_cuda(o, d, bg_color=1.0, **KW)
        model.run_cuda(o, d, normals="only", **KW)

    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        for suffix in ("_ms", "_ms_again"):                             # alternate: no leg owes its number to its place in the run
            out["colour" + suffix], _ = timed(lambda: model.run_cuda(o, d, bg_color=1.0, **KW))
            out["only" + suffix], out["only_all" + suffix] = timed(lambda: model.run_cuda(o, d, normals="only", **KW))
            out["aux" + suffix], out["aux_all" + suffix] = timed(lambda: model.run_cuda(o, d, normals=True, bg_color=1.0, **KW))
            out["colour_then_only" + suffix], out["colour_then_only_all" + suffix] = timed(colour_then_only)
            out["fixed512" + suffix], _ = timed(lambda: focnerf_amd.render_normals(model, o, d, num_steps=512))
        march = model.run_cuda(o, d, normals="only", **KW)
        n_fix, w_fix, _ = focnerf_amd.render_normals(model, o, d, num_steps=512)
    both = (march["weights_sum"] > 0.5) & (w_fix > 0.5)
    cos = (march["normal"][both].double() * n_fix[both].double()).sum(-1).clamp(-1, 1)
    out["opaque_in_both_share"] = float(both.double().mean())
    out["mean_angle_deg"] = float(torch.rad2deg(torch.acos(cos)).mean()) if both.any() else None
    out["aux_faster_than_colour_then_only"] = bool(out["aux_ms"] < out["colour_then_only_ms"] and out["aux_ms_again"] < out["colour_then_only_ms_again"])
    return out


def _child(leg, tree=REPO):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--tree", tree], capture_output=True, text=True, timeout=LIMIT,
                           cwd=tree)
    except subprocess.TimeoutExpired:
        return {"error": f"time limit of {LIMIT} s"}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
    if r.returncode != 0 or not lines:
        return {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
    return json.loads(lines[-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["colour", "normals"], help="(internal) run one leg in this process")
    ap.add_argument("--tree", default=REPO, help="(internal) the tree a colour leg imports")
    ap.add_argument("--parent-tree", help="a built checkout of the parent commit, for leg (a)'s A/B")
    args = ap.parse_args()
    if args.leg:
        import torch
        assert torch.cuda.is_available(), "time_occ_normals.py measures on the GPU; there is no CPU fallback"
        print("LEG " + json.dumps(leg_colour(os.path.abspath(args.tree)) if args.leg == "colour" else leg_normals()))
        return
    out = {"colour": []}
    trees = [REPO, os.path.abspath(args.parent_tree)] * 2 if args.parent_tree else [REPO]
    for tree in trees:
        r = _child("colour", tree)
        out["colour"].append(r)
        if "error" in r:
            print(json.dumps(out))
            return                                                       # nothing more is started on the GPU after a leg that failed or hung
    if args.parent_tree:
        here = [r["colour_ms"] for r in out["colour"][0::2]]
        parent = [r["colour_ms"] for r in out["colour"][1::2]]
        spread = max(max(r["colour_ms_all"]) - min(r["colour_ms_all"]) for r in out["colour"])
        out["colour_ab"] = {"this_ms": here, "parent_ms": parent, "spread_of_repeats_ms": spread,
                            "difference_ms": statistics.mean(here) - statistics.mean(parent),
                            "same_image": len({r["image_sum"] for r in out["colour"]}) == 1}
    out["normals"] = _child("normals")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
