"""CPU: the float64 statement of the combined view's scoring (tests/metrics_ref.py) against the reference's recorded results
(tests/golden/score.npz, made by tests/golden/make_golden_score.py), the tap table, the reflect rule, and the host-side refusals of
the scoring entry points and of focnerf_amd.score — none of it needs a GPU."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "score.npz")

# scipy.ndimage's weights for sigma 1.5 (radius 6): exp(-0.5 / 2.25 * k^2) / sum, float64
TAPS_SIGMA_1_5 = [8.922106863539231e-05, 0.001028196578138909, 0.007597402196596929, 0.03599434807370883, 0.1093411749545305,
                  0.212967528547854, 0.2659642571610709, 0.212967528547854, 0.1093411749545305, 0.03599434807370883,
                  0.007597402196596929, 0.001028196578138909, 8.922106863539231e-05]


def test_statement_reproduces_the_reference_fixture():
    z = np.load(GOLDEN)
    H, W = int(z["H"]), int(z["W"])
    assert (H, W) == (24, 20) and z["image4"].shape == (2, H * W, 4) and z["image4"].dtype == np.float32
    alpha, gt_alpha = z["image4"][0, :, 3], z["gt"].reshape(-1, 4)[:, 3]
    assert (alpha < 0.5).any() and (alpha == 0.5).any() and (alpha > 0.5).any()                      # the cases the fixture must hold
    assert (gt_alpha == 0).any() and (gt_alpha == 1).any() and ((gt_alpha > 0) & (gt_alpha < 1)).any()
    assert ((alpha < 0.5) != (gt_alpha < 0.5)).any()
    r = metrics_ref.score(z["image4"], z["depth"], z["gt"], H, W, tuple(z["bgs"]))
    assert np.array_equal(r["rgba_u8"], z["rgba_u8"]) and np.array_equal(r["gt_u8"], z["gt_u8"]) and np.array_equal(r["depth_u8"], z["depth_u8"])
    assert (z["rgba_u8"][..., 3] == 255).all() and (z["gt_u8"][..., 3] == 255).all()
    for b in range(2):
        print(f"bg {b}: ssim {r['ssim'][b]!r} vs {float(z['ssim'][b])!r}, psnr {r['psnr'][b]!r} vs {float(z['psnr'][b])!r}")
        assert abs(r["ssim"][b] - float(z["ssim"][b])) <= 1e-9
        # the reference's mean is a float32 sum of 1920 terms: n * eps = 1.1e-4 relative in the worst case, times 10 / ln 10 dB
        assert abs(r["psnr"][b] - float(z["psnr"][b])) <= 1e-3
    assert abs(r["average_psnr"] - float(z["psnr"].mean())) <= 1e-3 and abs(r["average_ssim"] - float(z["ssim"].mean())) <= 1e-9


def test_tap_table():
    from focnerf_amd import score
    for taps in (metrics_ref.gaussian_taps(1.5), score.gaussian_taps(1.5)):
        assert len(taps) == 13 and list(taps) == TAPS_SIGMA_1_5                 # 13 taps: the reference's window_size=11 is read by nothing
    assert abs(sum(TAPS_SIGMA_1_5) - 1.0) < 1e-15
    assert len(score.gaussian_taps(0.8)) == 7 and list(metrics_ref.gaussian_taps(0.8)) == score.gaussian_taps(0.8)
    assert len(score.gaussian_taps(3.1)) == 25                                   # radius 12, the largest served
    with pytest.raises(ValueError):
        score.gaussian_taps(3.2)                                                 # radius 13
    with pytest.raises(ValueError):
        score.gaussian_taps(0.0)


def test_reflect_index_rule():
    i = np.arange(-13, 14)
    assert metrics_ref.reflect_index(i, 1).tolist() == [0] * 27
    assert metrics_ref.reflect_index(i, 3).tolist() == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert metrics_ref.reflect_index(i, 7).tolist() == [1, 2, 3, 4, 5, 6, 6, 5, 4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 5, 6, 6, 5, 4, 3, 2, 1, 0]
    for n in (1, 3, 7):                                                          # numpy's name for d c b a | a b c d is 'symmetric'
        assert np.array_equal(np.pad(np.arange(n), 13, mode="symmetric"), metrics_ref.reflect_index(i[0] + np.arange(n + 26), n))
    a = np.random.default_rng(0).random((5, 3))
    const = np.full((5, 3), 0.37)
    assert np.abs(metrics_ref.gaussian_filter(const, 1.5) - 0.37).max() < 1e-15  # a reflected constant stays constant
    assert abs(metrics_ref.gaussian_filter(a, 1.5).mean() - a.mean()) < 0.2


def test_statement_quantises_by_truncation_and_masks_by_alpha():
    image4 = np.array([[[0.999, 0.5, 1.0, 0.5], [0.2, 0.4, 0.6, 0.49999997], [0.0, 1.0 / 255.0, 0.9999, 1.0]]], dtype=np.float32)
    gt = np.array([[0.3, 0.3, 0.3, 0.0], [0.3, 0.3, 0.3, 0.75], [0.3, 0.3, 0.3, 0.5]], dtype=np.float32)
    p, g, d = metrics_ref.quantize(image4, np.array([0.0, 0.5, 1.0], np.float32), gt, 1, 3, (0.5,))
    assert p[0, 0].tolist() == [[254, 127, 255, 255], [127, 127, 127, 255], [0, 1, 254, 255]]
    assert g[0, 0].tolist() == [[127, 127, 127, 255], [76, 76, 76, 255], [76, 76, 76, 255]]
    assert d[0].tolist() == [0, 127, 255]
    assert metrics_ref.psnr(p[0], p[0]) == float("inf") and metrics_ref.sse(p[0], g[0]) == sum((a - b) ** 2 for a, b in zip(p.ravel().tolist(), g.ravel().tolist()))


def test_library_refuses_bad_arguments_without_a_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib
    assert lib.foc_abi_version() == 2
    assert lib.foc_score_workspace_bytes(800, 800, 2) == 2 * 50 * 50 * 32 and lib.foc_score_workspace_bytes(1, 1, 1) == 32
    assert lib.foc_score_workspace_bytes(17, 33, 3) == 3 * 2 * 3 * 32
    assert lib.foc_score_workspace_bytes(0, 4, 1) == 0 and lib.foc_score_workspace_bytes(1 << 16, (1 << 14) + 1, 1) == 0 and lib.foc_score_workspace_bytes(4, 4, 9) == 0
    one = ctypes.c_void_p(256)                                     # never dereferenced: every refusal comes before any launch
    bgs = (ctypes.c_float * 2)(1.0, 0.0)
    taps = (ctypes.c_double * 13)(*TAPS_SIGMA_1_5)

    def quantize(image4=one, depth=one, gt=one, bgs=bgs, H=4, W=4, B=2, pred=one, gtu=one, du=one):
        return lib.foc_score_quantize(image4, depth, gt, bgs, H, W, B, pred, gtu, du, None)
    assert quantize(image4=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert quantize(gtu=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert quantize(bgs=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert quantize(du=None) == 1 and b"come together" in lib.foc_last_error()
    assert quantize(H=0) == 1 and b"2^30" in lib.foc_last_error()
    assert quantize(H=1 << 16, W=1 << 16) == 1 and b"2^30" in lib.foc_last_error()       # H * W = 2^32 wraps to 0 in 32 bits
    assert quantize(B=0) == 1 and b"backgrounds" in lib.foc_last_error()
    assert quantize(bgs=(ctypes.c_float * 2)(1.0, float("nan"))) == 1 and b"not finite" in lib.foc_last_error()
    assert quantize(image4=ctypes.c_void_p(260)) == 1 and b"aligned" in lib.foc_last_error()

    def view(pred=one, gtu=one, H=4, W=4, B=2, taps=taps, radius=6, C1=1e-4, C2=9e-4, out=one, ws=one, nbytes=64):
        return lib.foc_score_view(pred, gtu, H, W, B, taps, radius, C1, C2, out, ws, nbytes, None)
    assert view(pred=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert view(taps=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert view(out=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert view(ws=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert view(H=1 << 16, W=1 << 16) == 1 and b"2^30" in lib.foc_last_error()
    assert view(B=9) == 1 and b"backgrounds" in lib.foc_last_error()
    assert view(taps=(ctypes.c_double * 27)(*([1 / 27] * 27)), radius=13) == 1 and b"radius must not exceed 12" in lib.foc_last_error()
    skew = list(TAPS_SIGMA_1_5)
    skew[0] *= 2
    assert view(taps=(ctypes.c_double * 13)(*skew)) == 1 and b"symmetric" in lib.foc_last_error()
    assert view(C2=float("nan")) == 1 and b"C1 and C2" in lib.foc_last_error()
    assert view(nbytes=63) == 1 and b"workspace of 63 bytes" in lib.foc_last_error()
    assert view(H=17, W=17, nbytes=255) == 1 and b"asks for 256" in lib.foc_last_error()
    assert view(ws=ctypes.c_void_p(260)) == 1 and b"aligned" in lib.foc_last_error()


def test_python_interface_refuses_bad_arguments_without_a_gpu():
    import torch
    import focnerf_amd
    from focnerf_amd import score
    assert focnerf_amd.score_view is score.score_view and focnerf_amd.ViewScore is score.ViewScore
    assert "score_view" in focnerf_amd.__all__ and "ViewScore" in focnerf_amd.__all__
    assert score.ViewScore._fields == ("psnr", "ssim", "average_psnr", "average_ssim", "rgba_u8", "gt_u8", "depth_u8")
    H, W = 4, 5
    image4, depth, gt = torch.zeros(2, H * W, 4), torch.zeros(H * W), torch.zeros(H, W, 4)
    with pytest.raises((ValueError, RuntimeError)):
        score.score_view(image4, depth, gt, H, W)                                # host tensors: these ops have no CPU implementation
    with pytest.raises(ValueError):
        score.score_view(image4, depth, gt, H, W, sigma=4.0)                     # radius 16 > 12, refused before anything else

    class OnDevice:                                                              # what the checks read of a tensor, without a device
        def __init__(self, *shape, dtype=torch.float32, device="cuda:0"):
            self.shape, self.dtype, self.device, self.is_cuda = torch.Size(shape), dtype, torch.device(device), True

        def dim(self):
            return len(self.shape)

        def numel(self):
            return math.prod(self.shape)

    real_is_tensor = torch.is_tensor
    torch.is_tensor = lambda t: isinstance(t, OnDevice) or real_is_tensor(t)
    try:
        ok = (OnDevice(2, H * W, 4), OnDevice(H * W), OnDevice(H, W, 4))
        assert score._check_inputs(*ok, H, W, (1.0, 0.0)) == (H, W, 2, [1.0, 0.0])
        assert score._check_inputs(ok[0], ok[1], OnDevice(H * W, 4), H, W, (1.0, 0.0))[2] == 2
        bad = [((OnDevice(2, H * W, 3), ok[1], ok[2]), (1.0, 0.0)),             # not RGBA
               ((OnDevice(2, H * W + 1, 4), ok[1], ok[2]), (1.0, 0.0)),         # N != H * W
               ((OnDevice(H * W, 4), ok[1], ok[2]), (1.0, 0.0)),                # no background dimension
               ((ok[0], OnDevice(H * W - 1), ok[2]), (1.0, 0.0)),               # depth of another view
               ((ok[0], ok[1], OnDevice(W, H, 4)), (1.0, 0.0)),                 # gt transposed
               ((ok[0], ok[1], OnDevice(H, W, 4, dtype=torch.float16)), (1.0, 0.0)),
               ((OnDevice(2, H * W, 4, dtype=torch.float64), ok[1], ok[2]), (1.0, 0.0)),
               ((ok[0], ok[1], OnDevice(H, W, 4, device="cuda:1")), (1.0, 0.0)),
               (ok, (1.0,)), (ok, (1.0, 0.0, 0.5)),                              # len(bgs) != B
               (ok, (1.0, float("inf"))),
               ((OnDevice(9, H * W, 4), ok[1], ok[2]), (0.0,) * 9)]
        for tensors, bgs in bad:
            with pytest.raises(ValueError):
                score._check_inputs(*tensors, H, W, bgs)
        with pytest.raises(ValueError):
            score._check_inputs(*ok, 0, W, (1.0, 0.0))
        with pytest.raises(ValueError):
            score._check_inputs(*ok, 1 << 16, 1 << 16, (1.0, 0.0))
    finally:
        torch.is_tensor = real_is_tensor
    assert score.psnr_from_sse(0, 16) == float("inf")
    assert score.psnr_from_sse(16 * 255 * 255, 16) == 0.0 and abs(score.psnr_from_sse(16, 16) - 20 * math.log10(255.0)) < 1e-12
    assert "LPIPS" in score.__doc__ and "window_size=11" in score.__doc__
