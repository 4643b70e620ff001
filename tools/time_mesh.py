"""Mesh extraction of ONE object at resolution 256 (the reference's `save_mesh` default) on a network of the trained shape (bench.py's
model, embeddings uniform in [-0.5, 0.5]; untrained: its surface is noise, which is the expensive case for the marching cubes). Run on
the GPU box; prints one JSON line, milliseconds as the median of REPS timed calls after WARMUP, a host clock around work that ends in
a device synchronise (every leg reads a result on the host or is synchronised):

    reference_loop_ms   the reference's `extract_fields` (nerf/utils.py:512-527) on this repository's ops: 128^3 pieces, `.cpu().numpy()`
                        per piece into a host array — what a user has without focnerf_amd.mesh
    dense_ms            mesh.density_volume(model, 256)
    culled_ms           mesh.density_volume(model, 256, occupancy=Occupancy.estimate(model, jitter=False)); occupied_share = the share
                        of lattice points the cull keeps
    marching_cubes_ms   mesh.marching_cubes alone on the dense volume at its median (a non-empty surface), with vertices / triangles
    volume_pass_ms      one read of the volume (`vol.sum()`): the unit "a pass over the volume" for the line above
    sphere_grid         culled_ms / dense_ms / occupied_share with the analytic sphere grid of bench.py's occupancy legs as the occupancy
    sphere_256 / _512   marching_cubes_ms and volume_pass_ms on a smooth surface (a ball of radius 0.4 n in an n^3 volume)
"""
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
from focnerf_amd import mesh  # noqa: E402
from focnerf_amd.fixedcull import Occupancy  # noqa: E402

WARMUP, REPS = 2, 7


def timed(fn):
    times = []
    for rep in range(WARMUP + REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def reference_loop(model, resolution, S=128):
    """`extract_fields` as the reference writes it, with `save_mesh`'s query function."""
    lo, hi = model.aabb_infer[:3].cpu(), model.aabb_infer[3:].cpu()
    dev = model.aabb_infer.device
    X, Y, Z = (torch.linspace(float(lo[k]), float(hi[k]), resolution).split(S) for k in range(3))
    u = np.zeros([resolution] * 3, dtype=np.float32)
    with torch.no_grad():
        for xi, xs in enumerate(X):
            for yi, ys in enumerate(Y):
                for zi, zs in enumerate(Z):
                    xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                    pts = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                    with torch.autocast("cuda", dtype=torch.float16):
                        val = model.density(pts.to(dev))['sigma']
                    u[xi * S: xi * S + len(xs), yi * S: yi * S + len(ys), zi * S: zi * S + len(zs)] = val.reshape(len(xs), len(ys), len(zs)).detach().cpu().numpy()
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    R = args.resolution
    model = bench.build_model(1, dev, cuda_ray=False, seed=0).eval()
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    out = {"resolution": R, "reps": REPS, "warmup": WARMUP}
    out["reference_loop_ms"], out["reference_loop_ms_all"] = timed(lambda: reference_loop(model, R))
    out["dense_ms"], out["dense_ms_all"] = timed(lambda: mesh.density_volume(model, R))
    occ = Occupancy.estimate(model, jitter=False)
    out["culled_ms"], out["culled_ms_all"] = timed(lambda: mesh.density_volume(model, R, occupancy=occ))
    out["dense_ms_again"], _ = timed(lambda: mesh.density_volume(model, R))          # alternate once more: neither owes its number to its place in the run
    out["culled_ms_again"], _ = timed(lambda: mesh.density_volume(model, R, occupancy=occ))
    vol = mesh.density_volume(model, R)
    culled = mesh.density_volume(model, R, occupancy=occ)
    axes = mesh.lattice_axes(model.aabb_infer, R, dev)
    out["occupied_share"] = int(mesh.lattice_cull(axes, 0, R ** 3, occupancy=occ)[2].item()) / R ** 3
    out["dense_equals_reference_loop"] = bool(np.array_equal(vol.cpu().numpy(), reference_loop(model, R)))
    out["culled_equals_dense_where_kept"] = bool(torch.equal(culled[culled > 0], vol[culled > 0]))
    thr = float(vol.median())
    v, f = mesh.marching_cubes(vol, thr)
    out["threshold"], out["vertices"], out["triangles"] = thr, v.shape[0], f.shape[0]
    out["marching_cubes_ms"], out["marching_cubes_ms_all"] = timed(lambda: mesh.marching_cubes(vol, thr))
    out["marching_cubes_normals_ms"], _ = timed(lambda: mesh.marching_cubes(vol, thr, normals=True))
    out["volume_pass_ms"], _ = timed(lambda: vol.sum())
    # an occupancy with empty space: the analytic sphere grid of bench.py's occupancy legs (the network is untrained, so the grid estimated
    # from its own density above keeps every cell)
    grid = Occupancy.of(bench.build_model(1, dev, cuda_ray=True, seed=0))
    out["sphere_grid"] = {"occupied_share": int(mesh.lattice_cull(axes, 0, R ** 3, occupancy=grid)[2].item()) / R ** 3,
                          "culled_ms": timed(lambda: mesh.density_volume(model, R, occupancy=grid))[0],
                          "dense_ms": timed(lambda: mesh.density_volume(model, R))[0]}
    # a smooth surface, at this resolution and at 512 (a volume of 512 MiB: larger than the Infinity Cache)
    for n in (R, 512):
        ax = torch.arange(n, dtype=torch.float32, device=dev) - n / 2
        sphere = 0.4 * n - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
        vs, fs = mesh.marching_cubes(sphere, 0.0)
        out["sphere_%d" % n] = {"vertices": vs.shape[0], "triangles": fs.shape[0], "marching_cubes_ms": timed(lambda: mesh.marching_cubes(sphere, 0.0))[0],
                                "volume_pass_ms": timed(lambda: sphere.sum())[0]}
        del sphere, vs, fs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
