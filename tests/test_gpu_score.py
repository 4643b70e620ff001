"""GPU: focnerf_amd.score (csrc/score.hip) against the float64 statement tests/metrics_ref.py on the same inputs.

Bounds. The byte images and the squared error are integers: identical. Each SSIM within 1e-9 absolute: float64 unit roundoff is
1.1e-16, the division by sigma1^2 + sigma2^2 + C2 amplifies by up to 1 / C2 = 1.1e3, over a few dozen operations per pixel — two
float64 orders of summation were seen 5e-13 apart. PSNR within 1e-9 dB: both sides compute it in float64 from the same integer.
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (5, 3), (13, 7), (33, 47), (64, 64), (70, 130)]          # below and around the radius, ragged tiles, aligned, wider than tall
SSIM_TOL = 1e-9
PSNR_TOL = 1e-9


def _blur(a):
    return (a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, -1, 0)) / 4


@functools.lru_cache(maxsize=None)
def make_case(H, W, content, B=2):
    """-> (image4 [B,N,4], depth [N], gt [H,W,4], bgs) float32 numpy, read-only."""
    rng = np.random.default_rng(1000 * H + W)
    N = H * W
    bgs = {1: (1.0,), 2: (1.0, 0.0), 3: (1.0, 0.0, 0.5)}[B]
    colour = rng.random((H, W, 3))
    alpha = rng.random((H, W))
    alpha.ravel()[::5] = 0.5
    gt_rgb, gt_alpha = np.clip(_blur(colour) + rng.normal(0, 0.02, (H, W, 3)), 0, 1), np.where(rng.random((H, W)) < 0.25, rng.random((H, W)), 1.0)
    if content == "identical":
        gt_rgb, gt_alpha = colour, alpha
    elif content == "constant":
        colour, gt_rgb, alpha, gt_alpha = np.full((H, W, 3), 0.3), np.full((H, W, 3), 0.6), np.ones((H, W)), np.ones((H, W))
    elif content == "masked":
        alpha, gt_alpha = alpha * 0.49, gt_alpha * 0.49
    elif content == "half":
        alpha, gt_alpha = np.full((H, W), 0.5), np.full((H, W), 0.5)
    else:
        assert content == "noise"
    image4 = np.empty((B, N, 4), dtype=np.float32)
    for b, bg in enumerate(bgs):
        if content == "identical":
            image4[b, :, :3] = colour.reshape(N, 3)                         # the same floats on both sides whatever the background
        else:
            image4[b, :, :3] = np.clip(colour * alpha[..., None] + bg * (1 - alpha[..., None]), 0, 1).reshape(N, 3)
        image4[b, :, 3] = alpha.reshape(N)
    depth = rng.random(N).astype(np.float32)
    gt = np.concatenate([gt_rgb, gt_alpha[..., None]], -1).astype(np.float32)
    for a in (image4, depth, gt):
        a.setflags(write=False)
    return image4, depth, gt, bgs


@functools.lru_cache(maxsize=None)
def reference(H, W, content, B=2, sigma=1.5):
    image4, depth, gt, bgs = make_case(H, W, content, B)
    return metrics_ref.score(image4, depth, gt, H, W, bgs, sigma=sigma)


def run(image4, depth, gt, H, W, bgs, **kw):
    from focnerf_amd import score
    dev = torch.device("cuda:0")
    t = [torch.tensor(np.asarray(a), device=dev) for a in (image4, depth, gt)]
    out, _, _, _ = score.score_raw(*t, H, W, bgs, **kw)
    return score.score_view(*t, H, W, bgs, **kw), out.cpu().numpy()


def compare(s, out, ref, H, W):
    B = len(ref["psnr"])
    assert s.rgba_u8.shape == (B, H, W, 4) and s.rgba_u8.dtype == torch.uint8 and s.depth_u8.shape == (H, W) and s.rgba_u8.is_cuda
    assert np.array_equal(s.rgba_u8.cpu().numpy(), ref["rgba_u8"])
    assert np.array_equal(s.gt_u8.cpu().numpy(), ref["gt_u8"])
    assert np.array_equal(s.depth_u8.cpu().numpy(), ref["depth_u8"])
    assert out.shape == (B, 4) and out.dtype == np.float64
    for b in range(B):
        assert out[b, 0] == float(int(out[b, 0])) and int(out[b, 0]) == ref["sse"][b]
        for c in range(3):
            print(f"{H}x{W} bg {b} channel {c}: ssim {out[b, 1 + c]!r}, statement {ref['ssim_channels'][b][c]!r}, diff {abs(out[b, 1 + c] - ref['ssim_channels'][b][c]):.3e}")
            assert abs(out[b, 1 + c] - ref["ssim_channels"][b][c]) <= SSIM_TOL
        print(f"{H}x{W} bg {b}: ssim {s.ssim[b]!r} vs {ref['ssim'][b]!r}, psnr {s.psnr[b]!r} vs {ref['psnr'][b]!r}")
        assert abs(s.ssim[b] - ref["ssim"][b]) <= SSIM_TOL
        if math.isinf(ref["psnr"][b]):
            assert s.psnr[b] == float("inf")
        else:
            assert abs(s.psnr[b] - ref["psnr"][b]) <= PSNR_TOL
    assert isinstance(s.psnr, list) and isinstance(s.ssim[0], float) and len(s.ssim) == B
    assert s.average_ssim == pytest.approx(ref["average_ssim"], abs=SSIM_TOL)
    if math.isfinite(ref["average_psnr"]):
        assert s.average_psnr == pytest.approx(ref["average_psnr"], abs=PSNR_TOL)
    else:
        assert s.average_psnr == float("inf")


@pytest.mark.parametrize("H,W", SIZES)
def test_noise_against_a_blurred_copy(H, W):
    image4, depth, gt, bgs = make_case(H, W, "noise")
    s, out = run(image4, depth, gt, H, W, bgs)
    compare(s, out, reference(H, W, "noise"), H, W)


@pytest.mark.parametrize("H,W", SIZES)
def test_identical_images(H, W):
    image4, depth, gt, bgs = make_case(H, W, "identical")
    s, out = run(image4, depth, gt, H, W, bgs)
    compare(s, out, reference(H, W, "identical"), H, W)
    for b in range(2):
        assert s.psnr[b] == float("inf") and out[b, 0] == 0 and abs(s.ssim[b] - 1.0) <= 1e-12


@pytest.mark.parametrize("content", ["constant", "masked", "half"])
@pytest.mark.parametrize("H,W", [(5, 3), (33, 47)])
def test_constant_masked_and_threshold_alpha(H, W, content):
    image4, depth, gt, bgs = make_case(H, W, content)
    s, out = run(image4, depth, gt, H, W, bgs)
    ref = reference(H, W, content)
    compare(s, out, ref, H, W)
    if content == "masked":                                                     # every pixel is the background on both sides
        assert (s.rgba_u8[0] == 255).all() and (s.rgba_u8[1, ..., :3] == 0).all() and s.psnr == [float("inf")] * 2
    if content == "half":                                                       # exactly 0.5 is kept
        assert (s.rgba_u8[0, ..., :3] != 255).any() and (s.rgba_u8[1, ..., :3] != 0).any() and (s.gt_u8[1, ..., :3] != 0).any()


@pytest.mark.parametrize("B", [1, 3])
def test_one_and_three_backgrounds(B):
    H, W = 33, 47
    image4, depth, gt, bgs = make_case(H, W, "noise", B)
    s, out = run(image4, depth, gt, H, W, bgs)
    compare(s, out, reference(H, W, "noise", B), H, W)
    if B == 3:
        masked = torch.tensor(np.asarray(gt[..., 3] < 0.5))
        assert masked.any() and (s.gt_u8[2].cpu()[masked][:, :3] == 127).all()  # uint8(trunc(0.5 * 255))


def test_sigma_0_8():
    H, W = 13, 7
    image4, depth, gt, bgs = make_case(H, W, "noise")
    s, out = run(image4, depth, gt, H, W, bgs, sigma=0.8)
    compare(s, out, reference(H, W, "noise", 2, 0.8), H, W)
    assert abs(s.ssim[0] - reference(H, W, "noise")["ssim"][0]) > 1e-6          # another filter, another score


def test_custom_constants_and_flat_gt_layout():
    H, W = 13, 7
    image4, depth, gt, bgs = make_case(H, W, "noise")
    from focnerf_amd import score
    dev = torch.device("cuda:0")
    s = score.score_view(torch.tensor(image4, device=dev), torch.tensor(depth, device=dev), torch.tensor(gt, device=dev).view(H * W, 4), H, W, k1=0.02, k2=0.05)
    ref = metrics_ref.score(image4, depth, gt, H, W, bgs, k1=0.02, k2=0.05)
    for b in range(2):
        assert abs(s.ssim[b] - ref["ssim"][b]) <= SSIM_TOL and abs(s.psnr[b] - ref["psnr"][b]) <= PSNR_TOL


def test_reference_fixture_end_to_end():
    z = np.load(os.path.join(REPO, "tests", "golden", "score.npz"))
    H, W = int(z["H"]), int(z["W"])
    s, out = run(z["image4"], z["depth"], z["gt"], H, W, tuple(z["bgs"]))
    assert np.array_equal(s.rgba_u8.cpu().numpy(), z["rgba_u8"]) and np.array_equal(s.gt_u8.cpu().numpy(), z["gt_u8"])
    assert np.array_equal(s.depth_u8.cpu().numpy(), z["depth_u8"])
    for b in range(2):
        print(f"fixture bg {b}: ssim {s.ssim[b]!r} vs {float(z['ssim'][b])!r}, psnr {s.psnr[b]!r} vs {float(z['psnr'][b])!r}")
        assert abs(s.ssim[b] - float(z["ssim"][b])) <= SSIM_TOL
        assert abs(s.psnr[b] - float(z["psnr"][b])) <= 1e-3                    # the reference's float32 mean (tests/test_score_ref.py)
    compare(s, out, metrics_ref.score(z["image4"], z["depth"], z["gt"], H, W, tuple(z["bgs"])), H, W)


def test_same_bits_on_every_run_in_both_deterministic_modes():
    import focnerf_amd
    from focnerf_amd import score
    H, W = 70, 130
    image4, depth, gt, bgs = make_case(H, W, "noise")
    dev = torch.device("cuda:0")
    t = [torch.tensor(a, device=dev) for a in (image4, depth, gt)]
    outs = []
    for flag in (False, True):
        with focnerf_amd.deterministic(flag):
            for _ in range(2):
                outs.append(score.score_raw(*t, H, W, bgs)[0].cpu().numpy().view(np.uint64))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])


def test_scores_what_combine_packed_returns():
    from focnerf_amd import combine, score
    H = W = 8
    N, T = H * W, 16
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    fields = []
    for k in range(2):
        dens = torch.rand(N, T, generator=g) * 8.0 * (torch.rand(N, 1, generator=g) < 0.7)         # some rays stay empty: alpha below 0.5
        fields.append(combine.pack_field4(dens.to(dev), torch.rand(N, T, 3, generator=g).to(dev)))
    nears, fars = torch.full((N,), 0.2, device=dev), torch.full((N,), 1.7, device=dev)
    image4, depth = combine.combine_packed(fields, nears, fars)
    assert image4.shape == (2, N, 4) and depth.shape == (N,)
    gt = torch.rand(H, W, 4, generator=g).to(dev)
    s = score.score_view(image4, depth, gt, H, W)
    out = score.score_raw(image4, depth, gt, H, W)[0].cpu().numpy()
    a = image4[1, :, 3]                      # the composite adds the background to alpha too: white is opaque everywhere, black keeps the ray's weight
    assert (a < 0.5).any() and (a >= 0.5).any() and (image4[0, :, 3] >= 0.5).all()
    compare(s, out, metrics_ref.score(image4.cpu().numpy(), depth.cpu().numpy(), gt.cpu().numpy(), H, W), H, W)
