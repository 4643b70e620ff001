"""Float64 numpy statement of the combined view's scoring (COMBINED.py:267-378): quantise, PSNR and SSIM. No scipy import.

    quantize(image4, depth, gt, H, W, bgs) -> pred_u8 [B,H,W,4], gt_u8 [B,H,W,4], depth_u8 [H,W]
    psnr(pred_u8, gt_u8), ssim_rgba(pred_u8, gt_u8, sigma, k1, k2)     one background each
    score(image4, depth, gt, H, W, bgs, ...) -> dict                   what focnerf_amd.score.score_view returns, as numpy / floats

The filter is scipy.ndimage.gaussian_filter's: taps `gaussian_taps(sigma)` (radius int(4 sigma + 0.5), so 13 taps at sigma 1.5 — the
reference's window_size=11 is read by nothing), borders mode='reflect' (`reflect_index`), rows first and then columns here (scipy runs
the axes the other way round; the two agree to rounding). `ssim_rgba` follows the reference's flow channel by channel INCLUDING alpha,
whose two sides are constant 1: its SSIM is 1 up to rounding, which the kernel path takes as exactly 1.
"""
import numpy as np


def gaussian_taps(sigma, truncate=4.0):
    """scipy.ndimage._filters._gaussian_kernel1d(sigma, 0, radius) with radius = int(truncate * sigma + 0.5), in float64."""
    sigma = float(sigma)
    radius = int(truncate * sigma + 0.5)
    k = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return w / w.sum()


def reflect_index(i, n):
    """scipy's mode='reflect' (d c b a | a b c d): the index inside [0, n) that offset i reads, for any integer i and n >= 1."""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def filter1d(a, taps, axis):
    """Correlation of float64 `a` with the symmetric `taps` along `axis`, reflected borders."""
    radius = (len(taps) - 1) // 2
    n = a.shape[axis]
    out = np.zeros_like(a, dtype=np.float64)
    at = np.arange(n)
    for k in range(-radius, radius + 1):
        out += taps[k + radius] * np.take(a, reflect_index(at + k, n), axis=axis)
    return out


def gaussian_filter(a, sigma):
    taps = gaussian_taps(sigma)
    return filter1d(filter1d(np.asarray(a, dtype=np.float64), taps, 1), taps, 0)


def ssim_channel(ch1, ch2, sigma, k1, k2, L=1.0):
    mu1 = gaussian_filter(ch1, sigma)
    mu2 = gaussian_filter(ch2, sigma)
    sigma1_sq = gaussian_filter(ch1 ** 2, sigma) - mu1 ** 2
    sigma2_sq = gaussian_filter(ch2 ** 2, sigma) - mu2 ** 2
    sigma12 = gaussian_filter(ch1 * ch2, sigma) - mu1 * mu2
    C1 = (k1 * L) ** 2
    C2 = (k2 * L) ** 2
    ssim_map = ((2 * mu1 * mu2 + C1) * (2 * sigma12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (sigma1_sq + sigma2_sq + C2))
    return float(np.mean(ssim_map))


def ssim_channels(pred_u8, gt_u8, sigma=1.5, k1=0.01, k2=0.03):
    """The four per-channel SSIMs (r, g, b, a) of two [H,W,4] byte images."""
    a = pred_u8.astype(np.float64) / 255.0
    b = gt_u8.astype(np.float64) / 255.0
    return [ssim_channel(a[..., c], b[..., c], sigma, k1, k2) for c in range(4)]


def ssim_rgba(pred_u8, gt_u8, sigma=1.5, k1=0.01, k2=0.03):
    s = ssim_channels(pred_u8, gt_u8, sigma, k1, k2)
    return 0.8 * float(np.mean(s[:3])) + 0.2 * s[3]


def sse(pred_u8, gt_u8):
    """Sum over r, g, b, a of the squared byte differences, a Python int."""
    d = pred_u8.astype(np.int64) - gt_u8.astype(np.int64)
    return int((d * d).sum())


def psnr(pred_u8, gt_u8):
    """calculate_psnr on byte images in float64: max_pixel_value is 255 there because alpha is 255."""
    e = sse(pred_u8, gt_u8)
    if e == 0:
        return float("inf")
    return float(20.0 * np.log10(255.0 / np.sqrt(e / pred_u8.size)))


def _to_u8(x):
    return (np.asarray(x, dtype=np.float32) * np.float32(255.0)).astype(np.uint8)          # one float32 multiply, truncation toward zero


def quantize(image4, depth, gt, H, W, bgs=(1.0, 0.0)):
    """process_images_with_background :353-366 for every background, each from the ORIGINAL ground truth."""
    image4 = np.asarray(image4, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.float32).reshape(H, W, 4)
    assert image4.shape == (len(bgs), H * W, 4)
    pred_u8, gt_u8 = [], []
    for b, bg in enumerate(bgs):
        img = image4[b].reshape(H, W, 4).copy()
        g = gt.copy()
        fill = np.array([bg, bg, bg, 1.0], dtype=np.float32)
        img[img[:, :, 3] < np.float32(0.5)] = fill
        g[g[:, :, 3] < np.float32(0.5)] = fill
        img[:, :, 3] = 1.0
        g[:, :, 3] = 1.0
        pred_u8.append(_to_u8(img))
        gt_u8.append(_to_u8(g))
    return np.stack(pred_u8), np.stack(gt_u8), _to_u8(np.asarray(depth, dtype=np.float32).reshape(H, W))


def score(image4, depth, gt, H, W, bgs=(1.0, 0.0), sigma=1.5, k1=0.01, k2=0.03):
    pred_u8, gt_u8, depth_u8 = quantize(image4, depth, gt, H, W, bgs)
    B = len(bgs)
    out = {"rgba_u8": pred_u8, "gt_u8": gt_u8, "depth_u8": depth_u8,
           "sse": [sse(pred_u8[b], gt_u8[b]) for b in range(B)],
           "psnr": [psnr(pred_u8[b], gt_u8[b]) for b in range(B)],
           "ssim_channels": [ssim_channels(pred_u8[b], gt_u8[b], sigma, k1, k2) for b in range(B)]}
    out["ssim"] = [0.8 * float(np.mean(s[:3])) + 0.2 * s[3] for s in out["ssim_channels"]]
    out["average_psnr"] = float(np.mean(out["psnr"]))
    out["average_ssim"] = float(np.mean(out["ssim"]))
    return out
