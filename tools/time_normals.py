"""Surface normals from the density field: the fused kernel (csrc/normals.hip) against the autograd route, on bench.py's network with
embeddings uniform in [-0.5, 0.5]. Run on the GPU box; prints one JSON line. Milliseconds are the median of REPS timed calls after
WARMUP, a host clock around work that ends in a device synchronise. Two child processes, each under its own time limit (the parent
never opens the GPU):

  points   M = 2 097 152 uniform points in the model's box, one process (the gate compares legs of one process):
    autograd_ms       (a) normals.density_gradient with FOC_FUSED_NORMALS=0: GridEncoder's general forward with dy_dx -> FFMLP forward ->
                      FFMLP backward -> grid backward + input backward. Only kernels that exist without csrc/normals.hip: the baseline.
    fused_ms          (b) normals.density_gradient on the fused route (foc_field_normals + three elementwise torch ops)
    kernel_ms         (b') foc_field_normals alone: sigma and normal_rgb (what channels="normal" launches per chunk)
    encode_ms         (c) grid_encode_forward alone on the same points (level-major planes, no dy_dx), for scale
    gate              fused_ms < autograd_ms
  view     an 800 x 800, T = 512 view of tools/time_combine_culled.py's three placed objects through render_scene_culled:
    view_rgb_ms / view_normal_ms      channels="rgb" / "normal", alternated and walked twice (`*_again`)
    decode_ms                         normals.decode_normal_map of the view
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
M_POINTS = 2097152
LIMITS = {"points": 420, "view": 420}                  # seconds per child


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


def _model(cuda_ray):
    import torch
    sys.path.insert(0, REPO)
    import bench
    dev = torch.device("cuda", 0)
    model = bench.build_model(1, dev, cuda_ray=cuda_ray, seed=0).eval()
    model.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return model, dev


def leg_points():
    import torch
    model, dev = _model(False)
    from focnerf_amd import normals
    from focnerf_amd.backend import _gridencoder
    from focnerf_amd.field import field_plan, half_cache_scope
    assert field_plan(model).normals
    x = torch.rand(M_POINTS, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) * 2 - 1
    xn = ((x + 1) / 2).contiguous()
    out = {"points": M_POINTS, "reps": REPS, "warmup": WARMUP}

    def autograd():
        os.environ["FOC_FUSED_NORMALS"] = "0"
        try:
            return normals.density_gradient(model, x)
        finally:
            os.environ["FOC_FUSED_NORMALS"] = "1"

    enc = model.encoder
    grid = enc.spec()
    emb = enc.embeddings.detach().half().contiguous()
    planes = torch.empty(16, M_POINTS, 2, dtype=torch.half, device=dev)
    with torch.no_grad(), half_cache_scope():
        for suffix in ("_ms", "_ms_again"):                             # alternate: no leg owes its number to its place in the run
            out["autograd" + suffix], a_all = timed(autograd)
            out["fused" + suffix], f_all = timed(lambda: normals.density_gradient(model, x))
            out["kernel" + suffix], _ = timed(lambda: normals.field_normals(model, xn))
            out["encode" + suffix], _ = timed(lambda: _gridencoder.grid_encode_forward(xn, emb, enc.offsets, planes, M_POINTS, 3, 2, 16, grid.log2_scale,
                                                                                       grid.base_resolution, None, *grid.tail()))
            if suffix == "_ms":
                out["autograd_ms_all"], out["fused_ms_all"] = a_all, f_all
        s0, g0 = autograd()
        s1, g1 = normals.density_gradient(model, x)
    out["gate_fused_below_autograd"] = bool(out["fused_ms"] < out["autograd_ms"] and out["fused_ms_again"] < out["autograd_ms_again"])
    cos = torch.nn.functional.cosine_similarity(g0.double(), g1.double(), dim=-1)
    out["sigma_equal_share"] = float((s0 == s1).double().mean())
    out["gradient_cosine_median"], out["gradient_cosine_p01"] = float(cos.median()), float(cos.kthvalue(max(1, M_POINTS // 100)).values)
    return out


def leg_view():
    import torch
    model, dev = _model(True)
    sys.path.insert(0, REPO)
    import bench
    from focnerf_amd import Placement, combine, normals, synthetic
    from focnerf_amd.field import half_cache_scope
    from focnerf_amd.fixedcull import Occupancy
    side, T, chunk = bench.VIEW, bench.NUM_STEPS, 16384
    poses = synthetic.rand_poses(1, dev, radius=4.0, generator=torch.Generator().manual_seed(0))
    o, d = synthetic.get_rays(poses[:1], synthetic.intrinsics(side, side), side, side)
    o, d = o[0].contiguous(), d[0].contiguous()
    occ = Occupancy.of(model)
    scene = torch.tensor([-2.0] * 3 + [2.0] * 3, dtype=torch.float32, device=dev)
    places = [Placement.rotated((1, 2, 3), 37, translation=(0.6, 0.2, -0.4), scale=0.5), Placement(), Placement(translation=(-0.9, 0.3, 0.5), scale=0.75)]
    out = {"view": [side, side, T], "chunk": chunk, "objects": len(places)}

    def view(channels):
        return combine.render_scene_culled([model] * 3, [occ] * 3, places, o, d, T, scene, (1.0, 0.0), chunk, channels=channels)

    with torch.no_grad(), half_cache_scope():
        for suffix in ("_ms", "_ms_again"):
            out["view_rgb" + suffix], _ = timed(lambda: view("rgb"))
            out["view_normal" + suffix], _ = timed(lambda: view("normal"))
        img_n, dep_n = view("normal")
        img_c, dep_c = view("rgb")
        out["decode_ms"], _ = timed(lambda: normals.decode_normal_map(img_n))
        normal, opacity = normals.decode_normal_map(img_n)
    out["depth_equal"] = bool(torch.equal(dep_n.view(torch.int32), dep_c.view(torch.int32)))
    hit = opacity > 0.5
    out["rays_hit_share"] = float(hit.double().mean())
    out["unit_normals_share_of_hit"] = float(((normal[hit].norm(dim=-1) - 1).abs() < 1e-5).double().mean()) if hit.any() else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["points", "view"], help="(internal) run one leg in this process")
    args = ap.parse_args()
    if args.leg:
        import torch
        assert torch.cuda.is_available(), "time_normals.py measures on the GPU; there is no CPU fallback"
        print("LEG " + json.dumps(leg_points() if args.leg == "points" else leg_view()))
        return
    out = {}
    for leg, limit in LIMITS.items():
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            out[leg] = {"error": f"time limit of {limit} s"}
            break                                                        # nothing more is started on the GPU after a leg that hung
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not lines:
            out[leg] = {"error": f"exit status {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        out[leg] = json.loads(lines[-1][4:])
    print(json.dumps(out))
    sys.exit(0 if all("error" not in v for v in out.values()) and len(out) == len(LIMITS) else 1)


if __name__ == "__main__":
    main()
