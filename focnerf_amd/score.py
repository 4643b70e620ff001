"""PSNR and SSIM of a combined view against its ground truth, for every background, on the device (csrc/score.hip).

The reference scores each view right after rendering it (COMBINED.py:385-445 compute_metrics_both_backgrounds): per background it copies
the float image to the host, replaces pixels whose alpha is below 0.5 by the background, quantises to 8 bits by truncation, computes
PSNR on the bytes and SSIM from five Gaussian-filtered moments per channel in float64 (scipy.ndimage.gaussian_filter, sigma 1.5: 13
taps — its window_size=11 is read by nothing —, reflected borders), and mixes 0.8 * mean(r, g, b) + 0.2 * alpha. Here the combiners'
`image4 [B,N,4]` and `depth [N]` stay where they are:

    image4, depth = combine_packed(...)                      # or combine_culled, ObjectCombiner.render_view; bgs=(1.0, 0.0)
    s = score_view(image4, depth, gt, H, W)                  # gt [H,W,4] or [N,4] float32 on the same device
    s.psnr, s.ssim                                           # per background, Python floats; s.average_psnr, s.average_ssim
    s.rgba_u8, s.gt_u8, s.depth_u8                           # the byte images on the device, for whoever writes PNGs

Two launches quantise and score; the arithmetic on their [B,4] float64 result is done on the host, and reading it is the function's
only synchronisation. The alpha channel is constant 1 on both sides after quantisation, so its SSIM is taken as exactly 1. LPIPS is
not served: it needs AlexNet weights. Domain: finite values in [0, 1].
"""
import ctypes
import math
from typing import List, NamedTuple

import numpy as np
import torch

from ._lib import lib, ptr, stream_of, check
from .backend import _scratch

MAX_RADIUS = 12
MAX_BACKGROUNDS = 8
MAX_PIXELS = 1 << 30


class ViewScore(NamedTuple):
    psnr: List[float]
    ssim: List[float]
    average_psnr: float
    average_ssim: float
    rgba_u8: torch.Tensor       # [B,H,W,4] uint8
    gt_u8: torch.Tensor         # [B,H,W,4] uint8
    depth_u8: torch.Tensor      # [H,W] uint8


def gaussian_taps(sigma, truncate=4.0):
    """The float64 weights of scipy.ndimage.gaussian_filter(sigma): radius = int(truncate * sigma + 0.5),
    w_k = exp(-0.5 / sigma^2 * k^2) for k = -radius .. radius, divided by their sum."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0 (got {sigma!r})")
    radius = int(truncate * sigma + 0.5)
    if radius > MAX_RADIUS:
        raise ValueError(f"sigma {sigma} gives a filter radius of {radius}; at most {MAX_RADIUS} is supported")
    w = np.exp(-0.5 / (sigma * sigma) * np.arange(-radius, radius + 1) ** 2)        # scipy's own expression, hence its bits
    return (w / w.sum()).tolist()


def _check_inputs(image4, depth, gt, H, W, bgs):
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"H * W must be 1 .. 2^30 pixels (got {H} x {W})")
    N = H * W
    for name, t in (("image4", image4), ("depth", depth), ("gt", gt)):
        if not torch.is_tensor(t):
            raise ValueError(f"score_view: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"score_view: {name} must be float32 (got {t.dtype})")
        if not t.is_cuda:
            raise ValueError(f"score_view: {name} is on {t.device}; these ops have no CPU implementation")
        if t.device != image4.device:
            raise ValueError(f"score_view: {name} is on {t.device}, image4 on {image4.device}")
    if image4.dim() != 3 or image4.shape[1] != N or image4.shape[2] != 4:
        raise ValueError(f"score_view: image4 [B,{N},4] expected for {H} x {W} (got {tuple(image4.shape)})")
    B = image4.shape[0]
    if depth.numel() != N or depth.dim() > 2:
        raise ValueError(f"score_view: depth [{N}] expected (got {tuple(depth.shape)})")
    if tuple(gt.shape) not in ((H, W, 4), (N, 4)):
        raise ValueError(f"score_view: gt [{H},{W},4] or [{N},4] expected (got {tuple(gt.shape)})")
    bgs = [float(v) for v in bgs]
    if len(bgs) != B:
        raise ValueError(f"score_view: {len(bgs)} backgrounds for an image4 of {B}")
    if B < 1 or B > MAX_BACKGROUNDS:
        raise ValueError(f"score_view: 1 .. {MAX_BACKGROUNDS} backgrounds expected (got {B})")
    if not all(math.isfinite(v) for v in bgs):
        raise ValueError(f"score_view: backgrounds must be finite (got {bgs})")
    return H, W, B, bgs


def score_raw(image4, depth, gt, H, W, bgs=(1.0, 0.0), sigma=1.5, k1=0.01, k2=0.03):
    """The two launches of `score_view` without its host read: -> (out float64 [B,4] on the device: the squared byte error summed over
    r, g, b, a, then the mean SSIM of r, g and b; rgba_u8, gt_u8, depth_u8)."""
    taps = gaussian_taps(sigma)
    H, W, B, bgs = _check_inputs(image4, depth, gt, H, W, bgs)
    dev = image4.device
    image4, depth, gt = image4.contiguous(), depth.contiguous(), gt.contiguous()
    pred_u8 = torch.empty(B, H, W, 4, dtype=torch.uint8, device=dev)
    gt_u8 = torch.empty(B, H, W, 4, dtype=torch.uint8, device=dev)
    depth_u8 = torch.empty(H, W, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 4, dtype=torch.float64, device=dev)
    nbytes = lib.foc_score_workspace_bytes(H, W, B)
    ws = _scratch.get("score_view", nbytes, dev)
    st = stream_of(image4)
    check(lib.foc_score_quantize(ptr(image4), ptr(depth), ptr(gt), (ctypes.c_float * B)(*bgs), H, W, B, ptr(pred_u8), ptr(gt_u8), ptr(depth_u8), st),
          "score_quantize")
    check(lib.foc_score_view(ptr(pred_u8), ptr(gt_u8), H, W, B, (ctypes.c_double * len(taps))(*taps), (len(taps) - 1) // 2, float(k1) ** 2, float(k2) ** 2,
                             ptr(out), ptr(ws), nbytes, st), "score_view")
    return out, pred_u8, gt_u8, depth_u8


def psnr_from_sse(sse, n_values):
    """calculate_psnr (COMBINED.py:267-291) on bytes, in float64: the maximum is 255 there, because alpha is 255."""
    if sse == 0:
        return float("inf")
    return 20.0 * math.log10(255.0 / math.sqrt(sse / n_values))


def score_view(image4, depth, gt, H, W, bgs=(1.0, 0.0), sigma=1.5, k1=0.01, k2=0.03) -> ViewScore:
    """Scores of one view for every background of `image4 [B,N,4]` (`bgs` in the same order) against `gt`; see the module docstring."""
    out, pred_u8, gt_u8, depth_u8 = score_raw(image4, depth, gt, H, W, bgs, sigma, k1, k2)
    rows = out.tolist()                                                      # the one synchronisation
    n_values = int(H) * int(W) * 4                                           # alpha's term is 0 but counts in the mean
    psnr = [psnr_from_sse(r[0], n_values) for r in rows]
    ssim = [0.8 * ((r[1] + r[2] + r[3]) / 3.0) + 0.2 * 1.0 for r in rows]
    return ViewScore(psnr, ssim, sum(psnr) / len(psnr), sum(ssim) / len(ssim), pred_u8, gt_u8, depth_u8)
