"""The attribute stage of `mesh.extract_scene_mesh` — `query_scene` at the vertices of a scene's surface — for TWO placed objects at
resolution 256, on networks of the trained shape (bench.py's model, embeddings uniform in [-0.5, 0.5]; untrained, so the surface is noise
and has many vertices). Run on the GPU box; prints one JSON line. Milliseconds from a host clock around work that ends in a device
synchronise, the two routes ALTERNATED for REPS repetitions after WARMUP of each; median, min and max:

    query_ms   query_scene(models, placements, vertices): cull -> emit -> foc_field_normals -> foc_surface_frame -> encoder + field
               inference -> foc_scene_select, on the vertices inside each object's box only
    torch_ms   the plain torch route in the same process: EVERY vertex on EVERY object — q = A x + b, `normals.density_gradient`, the unit
               normal, the module's `forward(q, -n)` under fp16 autocast — then the box test and the select with `torch.where`
    agree      how far the two answers are apart (the torch route's colours come from the training-path kernels): the share of vertices with
               the same winner, and [median, 99.9th percentile, max] of the differences of sigma (relative), colour and normal where the
               winner is the same

The geometry stage (scene_volume + marching_cubes) is timed once for scale (`geometry_ms`); tools/time_mesh.py measures it properly."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from focnerf_amd import mesh, Placement, query_scene, density_gradient  # noqa: E402

WARMUP, REPS = 2, 7
SCENE = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_route(models, placements, x):
    """-> (sigma, object_id, rgb, normal) as query_scene defines them, from torch ops and the modules' own entry points."""
    n, dev = x.shape[0], x.device
    sigma = torch.zeros(n, device=dev)
    ids = torch.full((n,), -1, dtype=torch.int32, device=dev)
    rgb, normal = torch.zeros(n, 3, device=dev), torch.zeros(n, 3, device=dev)
    with torch.no_grad():
        for k, (model, P) in enumerate(zip(models, placements)):
            A, b = P.world_to_object64()
            A, b = torch.from_numpy(A.astype(np.float32)).to(dev), torch.from_numpy(b.astype(np.float32)).to(dev)
            q = x @ A.T + b
            box = model.aabb_infer
            inside = ((q >= box[:3]) & (q <= box[3:])).all(-1)
            qc = torch.minimum(torch.maximum(q, box[:3]), box[3:])
            s, grad = density_gradient(model, qc)
            n_obj = mesh.unit_normals(grad)
            none = (n_obj == 0).all(-1, keepdim=True)
            dirs = torch.where(none, torch.tensor([0.0, 0.0, -1.0], device=dev), -n_obj)
            with torch.autocast("cuda", dtype=torch.float16):
                _, c = model(qc, dirs)
            v = s * float(P.sigma_gain)
            win = inside & (v > sigma)
            sigma = torch.where(win, v, sigma)
            ids = torch.where(win, torch.full_like(ids, k), ids)
            rgb = torch.where(win[:, None], c.float(), rgb)
            normal = torch.where(win[:, None], n_obj @ torch.from_numpy(P.rotation.astype(np.float32)).to(dev).T, normal)
    return sigma, ids, rgb, normal


def spread(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "all": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_scene_mesh.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    R = args.resolution
    models = []
    for seed in (0, 1):
        m = bench.build_model(1, dev, cuda_ray=False, seed=seed).eval()
        torch.manual_seed(seed)
        m.encoder.embeddings.data.uniform_(-0.5, 0.5)
        models.append(m)
    # scales near 1: the untrained networks' densities are alike, and the gains 1 / scale must leave both objects a share of the surface
    placements = [Placement.rotated((0, 0, 1), 90, translation=(0.5, -0.2, 0.1), scale=0.9),
                  Placement.rotated((1, 2, 0.5), 33, translation=(-0.5, 0.3, 0.0), scale=1.1)]
    vol = mesh.scene_volume(models, placements, R, SCENE)
    thr = float(vol[vol > 0].median())
    del vol
    geometry_ms, (v, f) = clock(lambda: mesh.extract_scene_geometry(models, placements, SCENE, R, thr))
    out = {"resolution": R, "objects": 2, "threshold": thr, "vertices": v.shape[0], "triangles": f.shape[0], "reps": REPS, "warmup": WARMUP,
           "geometry_ms": geometry_ms}
    routes = {"query_ms": lambda: query_scene(models, placements, v), "torch_ms": lambda: torch_route(models, placements, v)}
    times = {name: [] for name in routes}
    for rep in range(WARMUP + REPS):
        for name, fn in routes.items():                                  # alternated: neither owes its number to its place in the run
            ms, _ = clock(fn)
            if rep >= WARMUP:
                times[name].append(ms)
    for name in routes:
        out[name] = spread(times[name])
    out["torch_over_query"] = out["torch_ms"]["median"] / out["query_ms"]["median"]
    s = query_scene(models, placements, v)
    ts, ti, tc, tn = torch_route(models, placements, v)
    same = (s.object_id == ti)
    covered = same & (ti >= 0)
    out["covered_share"] = float((s.object_id >= 0).float().mean())
    out["object_shares"] = [float((s.object_id == k).float().mean()) for k in range(2)]
    def far(a, b):                                                       # [median, 99.9th percentile, max] of the largest component's difference
        d = (a - b)[covered].abs().reshape(int(covered.sum()), -1).amax(-1).float().sort().values
        return [float(d[len(d) // 2]), float(d[int(len(d) * 0.999)]), float(d[-1])]
    # the torch route maps x with a matmul, the kernels with their own fixed-order q = A x + b: positions an ulp apart, and the untrained field
    # is noise at the fine levels, so single vertices can differ by a whole normal; the percentiles say how rare that is
    out["agree"] = {"same_winner_share": float(same.float().mean()), "sigma_rel": far(s.sigma / ts.clamp_min(1e-30), ts / ts.clamp_min(1e-30)),
                    "rgb_abs": far(s.rgb, tc), "normal_abs": far(s.normal, tn)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
