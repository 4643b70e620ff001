"""Connected-component labelling at resolution 256 (the reference's `save_mesh` default): a ball of radius 0.3 n plus a few thousand
random specks, the shape of a trained density with floaters. Run on the GPU box; prints one JSON line, milliseconds as the median of
REPS timed calls after WARMUP, a host clock around work that ends in a device synchronise:

    label_ms             foc_cc_label alone (four launches and the zero fill of the counts; no host read)
    label_components_ms  components.label_components: + the host read of the counts and the dense renumbering in torch
    filter_ms            components.filter_components(keep_largest=1): label, host read, keep order, foc_cc_select
    host_route_ms        what it replaces: device -> host copy, scipy.ndimage.label (3 x 3 x 3 structure), mask of the largest, copy back
    marching_cubes_ms    mesh.marching_cubes on the same volume, as a yardstick
    copy_ms              a plain device copy of the volume (`clone`): the memory floor, 4 bytes read and 4 written per point
    extract_geometry_ms / extract_geometry_keep_largest_ms   on bench.py's model (untrained: its surface is noise)
    filter_vs_host, label_vs_copy, filter_vs_copy            the ratios to report
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
from focnerf_amd import components, mesh  # noqa: E402
from focnerf_amd._lib import lib, ptr, stream_of, check  # noqa: E402

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


def test_volume(n, dev, specks=4000, seed=0):
    ax = torch.arange(n, dtype=torch.float32, device=dev) - n / 2
    vol = (0.3 * n - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)).clamp_min(0.0) * 4.0
    g = torch.Generator(device="cpu").manual_seed(seed)
    at = torch.randint(0, n ** 3, (specks,), generator=g).to(dev)
    vol.view(-1)[at] = 25.0
    return vol.contiguous()


def host_route(vol, thr):
    from scipy import ndimage
    u = vol.cpu().numpy()
    lab, K = ndimage.label(u >= thr, structure=np.ones((3, 3, 3)))
    sizes = np.bincount(lab.reshape(-1), minlength=K + 1)
    sizes[0] = 0
    keep = lab == int(np.argmax(sizes))                                  # argmax: the first of equal sizes, as the keep order's tie rule
    return torch.from_numpy(np.where((lab > 0) & ~keep, np.float32(0), u)).to(vol.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--no-model", action="store_true", help="skip the extract_geometry legs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_components.py measures on the GPU; there is no CPU fallback"
    dev = torch.device("cuda", 0)
    n, thr = args.resolution, 10.0
    vol = test_volume(n, dev)
    out = {"resolution": n, "threshold": thr, "reps": REPS, "warmup": WARMUP}
    c = components.label_components(vol, thr)
    out["components"], out["inside_points"], out["largest"] = c.count, int(c.sizes.sum()), int(c.sizes.max())

    nbytes = lib.foc_cc_workspace_bytes(n, n, n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty(n ** 3, dtype=torch.int32, device=dev)
    sizes = torch.empty(n ** 3, dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int32, device=dev)

    def label_only():
        check(lib.foc_cc_label(ptr(vol), n, n, n, thr, ptr(labels), ptr(sizes), ptr(ws), nbytes, ptr(counts), stream_of(vol)), "cc_label")
    out["label_ms"], out["label_ms_all"] = timed(label_only)
    out["counts4"] = [int(v) & 0xFFFFFFFF for v in counts.tolist()]
    out["label_components_ms"], _ = timed(lambda: components.label_components(vol, thr))
    out["filter_ms"], out["filter_ms_all"] = timed(lambda: components.filter_components(vol, thr, keep_largest=1))
    out["host_route_ms"], out["host_route_ms_all"] = timed(lambda: host_route(vol, thr))
    out["filter_ms_again"], _ = timed(lambda: components.filter_components(vol, thr, keep_largest=1))      # alternate once more
    out["filter_equals_host_route"] = bool(torch.equal(components.filter_components(vol, thr, keep_largest=1), host_route(vol, thr)))
    out["marching_cubes_ms"], _ = timed(lambda: mesh.marching_cubes(vol, thr))
    out["copy_ms"], out["copy_ms_all"] = timed(lambda: vol.clone())
    out["filter_vs_host"] = out["host_route_ms"] / out["filter_ms"]
    out["label_vs_copy"] = out["label_ms"] / out["copy_ms"]
    out["filter_vs_copy"] = out["filter_ms"] / out["copy_ms"]
    if not args.no_model:
        model = bench.build_model(1, dev, cuda_ray=False, seed=0).eval()
        model.encoder.embeddings.data.uniform_(-0.5, 0.5)
        mthr = float(mesh.density_volume(model, n).median())
        out["extract_geometry_ms"], _ = timed(lambda: mesh.extract_geometry(model, n, mthr))
        out["extract_geometry_keep_largest_ms"], _ = timed(lambda: mesh.extract_geometry(model, n, mthr, keep_largest=1))
        out["extract_geometry_ms_again"], _ = timed(lambda: mesh.extract_geometry(model, n, mthr))
        out["model_components"] = components.label_components(mesh.density_volume(model, n), mthr).count
    print(json.dumps(out))


if __name__ == "__main__":
    main()
