"""Generates tests/golden/score.npz from the reference's own scoring of a combined view (COMBINED.py), on the CPU.

    python tests/golden/make_golden_score.py <path of the reference checkout>      (or FOCNERF_REFERENCE=<path>)

Run where the reference lies, with scipy and Pillow installed; no test runs this. COMBINED.py cannot be imported (its methods live in a
class inside its `__main__` block, below imports of ultralytics, lpips, cv2, ...), so `process_images_with_background`, `calculate_psnr`,
`ssim_rgba` and `ssim_channel` are located with `ast`, compiled from the reference file where it lies and run here as methods of a
stand-in object whose `compute_lpips` returns 0 (LPIPS needs AlexNet weights). Nothing of the reference is copied: the fixture holds
data only — the inputs of one 24 x 20 view (float `image4` for a white and a black background, `depth`, `gt`) and what the reference
made of them per background: its two byte images, the depth bytes, PSNR and SSIM.

Each background gets a fresh copy of the ground truth: the reference edits `data['images']` through a numpy view in place, which
carries the white fill over into the black pass only when that tensor already lives on the host (tests/metrics_ref.py, quantize).
"""
import ast
import os
import sys
import textwrap
import types

import numpy as np
import torch

H, W = 24, 20
NAMES = ("process_images_with_background", "calculate_psnr", "ssim_rgba", "ssim_channel")


def draw(seed=0):
    rng = np.random.default_rng(seed)
    N = H * W
    alpha = rng.random(N).astype(np.float32)
    alpha[::7] = 0.5                                   # exactly the threshold: kept
    alpha[1::11] = np.float32(0.5) - np.float32(2.0 ** -25)   # the float32 just below it: masked
    alpha[2::13] = 0.0
    alpha[3::5] = 1.0
    colour = rng.random((N, 3)).astype(np.float32)
    image4 = np.empty((2, N, 4), dtype=np.float32)
    for b, bg in enumerate((1.0, 0.0)):               # a composite over the background, clamped as the combiners clamp
        image4[b, :, :3] = np.clip(colour * alpha[:, None] + np.float32(bg) * (1 - alpha[:, None]), 0, 1)
        image4[b, :, 3] = alpha
    depth = rng.random(N).astype(np.float32)
    depth[::9] = 0.0
    depth[4::9] = 1.0
    gt = np.clip(colour + rng.normal(0, 0.05, (N, 3)), 0, 1).astype(np.float32)
    gt_alpha = np.where(rng.random(N) < 0.3, 0.0, 1.0).astype(np.float32)
    gt_alpha[5::6] = rng.random(gt_alpha[5::6].shape).astype(np.float32)          # in between
    gt_alpha[6::17] = 0.5
    gt = np.concatenate([gt, gt_alpha[:, None]], -1).reshape(H, W, 4)
    pm, gm = alpha < 0.5, gt_alpha < 0.5
    assert (pm & ~gm).any() and (~pm & gm).any() and (pm & gm).any() and (~pm & ~gm).any()          # masked on one side only, on both, on neither
    assert (alpha == 0.5).any() and (gt_alpha == 0).any() and (gt_alpha == 1).any() and ((gt_alpha > 0) & (gt_alpha < 1)).any()
    return image4, depth, gt


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("FOCNERF_REFERENCE")
    if not ref or not os.path.exists(os.path.join(ref, "COMBINED.py")):
        raise SystemExit(__doc__)
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    import torch.nn.functional as F
    src = open(os.path.join(ref, "COMBINED.py")).read()
    wanted = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name in NAMES and node.name not in wanted:
            wanted[node.name] = textwrap.dedent(ast.get_source_segment(src, node))
    assert set(wanted) == set(NAMES), sorted(wanted)
    ns = {"np": np, "torch": torch, "F": F, "Image": Image, "gaussian_filter": gaussian_filter}
    for code in wanted.values():
        exec(compile(code, os.path.join(ref, "COMBINED.py"), "exec"), ns)
    scorer = types.SimpleNamespace(compute_lpips=lambda a, b: 0.0)
    for name in NAMES:
        setattr(scorer, name, types.MethodType(ns[name], scorer))

    image4, depth, gt = draw()
    out = {"H": np.int64(H), "W": np.int64(W), "bgs": np.array([1.0, 0.0]), "image4": image4, "depth": depth, "gt": gt}
    rgba_u8, gt_u8, depth_u8, psnr, ssim = [], [], [], [], []
    for b, name in enumerate(("white", "black")):
        trainer = types.SimpleNamespace(batch_image_depth_generation=lambda data, d, c, bg, b=b: (torch.tensor(image4[b]), torch.tensor(depth)))
        data = {"images": torch.tensor(gt)[None]}
        rgb_img, depth_img, gt_img, p, s, _ = scorer.process_images_with_background(trainer, data, None, None, H, W, name)
        rgba_u8.append(np.asarray(rgb_img)); gt_u8.append(np.asarray(gt_img)); depth_u8.append(np.asarray(depth_img))
        psnr.append(p); ssim.append(s)
    assert np.array_equal(depth_u8[0], depth_u8[1])
    out.update(rgba_u8=np.stack(rgba_u8), gt_u8=np.stack(gt_u8), depth_u8=depth_u8[0], psnr=np.array(psnr, dtype=np.float64), ssim=np.array(ssim, dtype=np.float64))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "score.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", "psnr", psnr, "ssim", ssim)


if __name__ == "__main__":
    main()
