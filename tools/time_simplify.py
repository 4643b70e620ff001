"""Vertex clustering (focnerf_amd.simplify_mesh, csrc/simplify.hip) on the ball of tools/time_mesh.py: radius 0.4 n in an n^3 volume at
n = 256 and n = 512, cells of k = 2 and k = 4 lattice steps, without attributes and with normals, colours and object ids. Run on the GPU
box; prints one JSON line. Milliseconds are the median of REPS timed calls after WARMUP, a host clock around work that ends in a device
synchronise; the legs of one size alternate inside every repetition, and the whole measurement runs in TWO fresh processes one after the
other (`runs`), so that no number owes itself to its place in a run or to one process's allocator state.

    simplify_ms / simplify_attr_ms   simplify_mesh with the grid given (one host read)
    count_ms / emit_ms               the two raw entry points alone (no host read between repetitions, no allocation): what the passes cost;
                                     int64_adds_per_us = the 64-bit atomic adds of the emit (3 per mapped vertex, 9 with normals and
                                     colours) over emit_ms — an upper bound on what the adds cost, the emit also zeroes, reads and writes
    torch_ms / torch_attr_ms         the same result by torch ops written here: torch.unique on the cell keys of the surviving triangles'
                                     corners, index_add_ for the sums, boolean masking for the triangles (float64 sums: close, not the
                                     same bits); checked against the kernel on Vc, Fc and the triangles
    marching_cubes_ms                mesh.marching_cubes (with normals) on the same volume: the pass that feeds the clustering
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARMUP, REPS = 3, 9


def timed_together(legs):
    """{name: fn} -> {name: median ms}; every repetition runs every leg once, in turn."""
    times = {name: [] for name in legs}
    for rep in range(WARMUP + REPS):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARMUP:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: round(statistics.median(ts), 4) for name, ts in times.items()}


def torch_route(v, f, k, dims, normals=None, colors=None, object_id=None):
    """Vertex clustering on the lattice-unit grid (origin 0, cell k) by torch ops. -> (vertices, triangles[, normals, colors, object_id])"""
    inv = torch.tensor(1.0, device=v.device) / float(k)
    t = v * inv
    c = torch.minimum(torch.floor(t).clamp_min(0), torch.tensor([g - 1.0 for g in dims], device=v.device))
    r = (t - c).clamp(0, 1).double()
    key = ((c[:, 0].long() * dims[1] + c[:, 1].long()) * dims[2] + c[:, 2].long())
    tk = key[f.long()]
    survive = (tk[:, 0] != tk[:, 1]) & (tk[:, 1] != tk[:, 2]) & (tk[:, 0] != tk[:, 2])
    kept = torch.unique(tk[survive])
    slot = torch.searchsorted(kept, key).clamp_max(max(kept.numel() - 1, 0))
    mapped = kept[slot] == key
    idx = slot[mapped]
    Vc = kept.numel()
    count = torch.zeros(Vc, dtype=torch.float64, device=v.device).index_add_(0, idx, torch.ones_like(idx, dtype=torch.float64))
    mean = torch.zeros(Vc, 3, dtype=torch.float64, device=v.device).index_add_(0, idx, r[mapped]) / count[:, None]
    cc = torch.zeros(Vc, 3, dtype=torch.float64, device=v.device)
    cc[idx] = c[mapped].double()
    out_v = ((cc + mean) * float(k)).float()
    vmap = torch.where(mapped, slot, torch.full_like(slot, -1))
    tri = vmap[f[survive].long()]
    shift = tri.argmin(dim=1, keepdim=True)
    tri = torch.gather(tri, 1, (shift + torch.arange(3, device=v.device)) % 3).int()
    out = [out_v, tri]
    if normals is not None:
        s = torch.zeros(Vc, 3, dtype=torch.float64, device=v.device).index_add_(0, idx, normals[mapped].double())
        out.append((s / s.norm(dim=1, keepdim=True).clamp_min(1e-300)).float())
    if colors is not None:
        s = torch.zeros(Vc, 3, dtype=torch.float64, device=v.device).index_add_(0, idx, colors[mapped].double().clamp(0, 1))
        out.append((s / count[:, None]).float())
    if object_id is not None:
        first = torch.full((Vc,), v.shape[0], dtype=torch.long, device=v.device).scatter_reduce_(0, idx, torch.nonzero(mapped).view(-1), "amin")
        out.append(object_id[first])
    return out


def raw_legs(v, f, attrs, origin, cell, dims, Vc, Fc):
    """The two entry points on preallocated buffers -> {name: fn}"""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    dev = v.device
    V, F = v.shape[0], f.shape[0]
    org, cel = (ctypes.c_float * 3)(*origin), (ctypes.c_float * 3)(*cell)
    nbytes = lib.foc_simplify_workspace_bytes(V, F, *dims)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    out_v, out_t = torch.empty(Vc, 3, device=dev), torch.empty(Fc, 3, dtype=torch.int32, device=dev)
    vmap, members = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(Vc, dtype=torch.int32, device=dev)
    legs = {}

    def count():
        check(lib.foc_simplify_count(ptr(v), V, ptr(f), F, org, cel, *dims, ptr(ws), nbytes, ptr(counts), stream_of(v)), "simplify_count")
    legs["count_ms"] = count
    for tag, a in (("emit_ms", (None, None, None)), ("emit_attr_ms", attrs)):
        n, c, ids = a
        abytes = lib.foc_simplify_accum_bytes(Vc, int(n is not None), int(c is not None))
        acc = torch.empty(abytes, dtype=torch.uint8, device=dev)
        on, oc = (None if n is None else torch.empty(Vc, 3, device=dev)), (None if c is None else torch.empty(Vc, 3, device=dev))
        oi = None if ids is None else torch.empty(Vc, dtype=torch.int32, device=dev)

        def emit(n=n, c=c, ids=ids, acc=acc, abytes=abytes, on=on, oc=oc, oi=oi):
            check(lib.foc_simplify_emit(ptr(v), V, ptr(f), F, ptr(n), ptr(c), ptr(ids), org, cel, *dims, ptr(ws), ptr(acc), abytes, Vc, Fc, ptr(out_v), ptr(on),
                                        ptr(oc), ptr(oi), ptr(vmap), ptr(members), ptr(out_t), stream_of(v)), "simplify_emit")
        legs[tag] = emit
    return legs


def measure():
    from focnerf_amd import mesh, simplify_mesh
    assert torch.cuda.is_available(), "time_simplify.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    out = {"reps": REPS, "warmup": WARMUP}
    for n in (256, 512):
        ax = torch.arange(n, dtype=torch.float32, device=dev) - n / 2
        ball = 0.4 * n - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
        v, f, nrm = mesh.marching_cubes(ball, 0.0, normals=True)
        g = torch.Generator(device=dev).manual_seed(n)
        col = torch.rand(v.shape[0], 3, device=dev, generator=g)
        ids = (torch.arange(v.shape[0], device=dev) % 3).int()
        row = {"vertices": v.shape[0], "triangles": f.shape[0]}
        row["marching_cubes_ms"] = timed_together({"mc": lambda: mesh.marching_cubes(ball, 0.0, normals=True)})["mc"]
        for k in (2, 4):
            dims = tuple(-(-(n - 1) // k) for _ in range(3))
            origin, cell = (0.0, 0.0, 0.0), (float(k),) * 3
            s = simplify_mesh(v, f, cell=cell, origin=origin, dims=dims)
            sa = simplify_mesh(v, f, cell=cell, origin=origin, dims=dims, normals=nrm, colors=col, object_id=ids)
            tv, tt = torch_route(v, f, k, dims)[:2]
            ta = torch_route(v, f, k, dims, nrm, col, ids)
            Vc, Fc = s.vertices.shape[0], s.triangles.shape[0]
            agree = {"Vc": tv.shape[0] == Vc, "Fc": tt.shape[0] == Fc, "triangles": tt.shape == s.triangles.shape and bool(torch.equal(tt, s.triangles)),
                     "vertices_max_abs_diff": float((tv - s.vertices).abs().max()), "normals_max_abs_diff": float((ta[2] - sa.normals).abs().max()),
                     "colors_max_abs_diff": float((ta[3] - sa.colors).abs().max()), "object_id": bool(torch.equal(ta[4], sa.object_id))}
            assert agree["Vc"] and agree["Fc"] and agree["triangles"] and agree["object_id"], agree
            legs = {"simplify_ms": lambda: simplify_mesh(v, f, cell=cell, origin=origin, dims=dims),
                    "simplify_attr_ms": lambda: simplify_mesh(v, f, cell=cell, origin=origin, dims=dims, normals=nrm, colors=col, object_id=ids),
                    "torch_ms": lambda: torch_route(v, f, k, dims),
                    "torch_attr_ms": lambda: torch_route(v, f, k, dims, nrm, col, ids)}
            legs.update(raw_legs(v, f, (nrm, col, ids), origin, cell, dims, Vc, Fc))
            res = timed_together(legs)
            mapped = int((s.vertex_map >= 0).sum())
            res.update({"Vc": Vc, "Fc": Fc, "members_max": int(s.members.max()), "members_mean": round(mapped / Vc, 2), "agree": agree,
                        "int64_adds_per_us": round(3 * mapped / (res["emit_ms"] * 1e3), 1),
                        "int64_adds_per_us_attr": round(9 * mapped / (res["emit_attr_ms"] * 1e3), 1)})
            row["k%d" % k] = res
        out["ball_%d" % n] = row
        del ball, v, f, nrm, col, ids
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help="measure in this process and print its JSON line")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure()))
        return
    runs = []
    for _ in range(2):                                                   # two fresh processes, one after the other; this one never opens the GPU
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode if p.returncode > 0 else 1)
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"runs": runs}))


if __name__ == "__main__":
    main()
