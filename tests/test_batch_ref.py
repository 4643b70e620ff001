"""CPU: the reference statements of focnerf_amd.batch (tests/batch_ref.py) against known answers, the repository's torch statement of
get_rays, the torch lines of the reference's train_step, torch.nn.MSELoss / HuberLoss with autograd and torch's gather / scatter; mutants
that the bounds must reject; the host-side refusals of the three entry points; DeviceDataset's refusals without a device."""
import ctypes

import numpy as np
import pytest
import torch

import batch_ref
from batch_ref import U

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


# ---------------------------------------------------------------- random numbers
@pytest.mark.parametrize("ctr,key,out", KNOWN)
def test_philox_known_answers(ctr, key, out):
    assert tuple(batch_ref.philox(ctr, key)) == out
    from focnerf_amd import _lib                                   # the kernels' own function, compiled for the host
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    assert _lib.lib.foc_philox4x32_10(c, k, o) == 0
    assert tuple(o) == out


def test_the_vector_form_is_the_integer_form():
    seed, step = 0x0123456789abcdef, (7 << 32) + 5
    q = batch_ref.philox_rays(seed, step, 70, 1)
    for r in (0, 1, 63, 69):
        assert tuple(int(v) for v in q[r]) == tuple(batch_ref.philox((r, step & 0xffffffff, step >> 32, 1), (seed & 0xffffffff, seed >> 32)))
    u = batch_ref.uniform(q)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert batch_ref.uniform(0xffffffff) == np.float32(1.0 - U) and batch_ref.uniform(0xff) == 0.0


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("step", [0, 1])
def test_pixels_are_in_range_and_uniform(seed, step):
    H, W, n = 5, 7, 4096
    inds = batch_ref.pixel_inds(seed, step, n, H, W)
    assert inds.dtype == np.int64 and (inds >= 0).all() and (inds < H * W).all()
    counts = np.bincount(inds, minlength=H * W)
    chi2 = float(((counts - n / (H * W)) ** 2 / (n / (H * W))).sum())
    print(f"chi-square seed {seed} step {step}: {chi2:.1f}")
    assert chi2 < 65.2                                             # the 99.9 % point for 34 degrees of freedom
    assert (batch_ref.pixel_inds(seed, step, 64, 800, 800) < 640000).all()
    assert (batch_ref.pixel_inds(seed, step, 64, 1, 1) == 0).all()


def test_steps_seeds_and_streams_differ():
    a = batch_ref.pixel_inds(0, 0, 256, 800, 800)
    assert not np.array_equal(a, batch_ref.pixel_inds(0, 1, 256, 800, 800))
    assert not np.array_equal(a, batch_ref.pixel_inds(1, 0, 256, 800, 800))
    assert not np.array_equal(a, batch_ref.pixel_inds(0, 1 << 32, 256, 800, 800))
    assert not np.array_equal(batch_ref.philox_rays(0, 0, 8, 0), batch_ref.philox_rays(0, 0, 8, 1))


@pytest.mark.parametrize("H,W", [(5, 7), (800, 800), (130, 257)])
def test_the_error_map_route_stays_inside_its_cell(H, W):
    rng = np.random.default_rng(0)
    c = rng.permutation(16384)[:4096]
    c[:4] = [0, 127, 16383 - 127, 16383]
    rows, cols = batch_ref.coarse_pixels(3, 9, c, H, W)
    assert (rows >= 0).all() and (rows < H).all() and (cols >= 0).all() and (cols < W).all()
    # the cell of a pixel in float64, with one fp32 rounding of slack at the cell's edges (the reference computes in fp32 too)
    lo_r, hi_r = np.floor((c // 128) * (H / 128) * (1 - 4 * U)), np.minimum(np.floor((c // 128 + 1) * (H / 128) * (1 + 4 * U)), H - 1)
    lo_c, hi_c = np.floor((c % 128) * (W / 128) * (1 - 4 * U)), np.minimum(np.floor((c % 128 + 1) * (W / 128) * (1 + 4 * U)), W - 1)
    assert (rows >= lo_r).all() and (rows <= hi_r).all() and (cols >= lo_c).all() and (cols <= hi_c).all()
    # the torch lines (nerf/utils.py:104-107) on the same uniforms
    q = batch_ref.philox_rays(3, 9, 4096, 0)
    u1, u2 = torch.from_numpy(batch_ref.uniform(q[:, 1])), torch.from_numpy(batch_ref.uniform(q[:, 2]))
    ic = torch.from_numpy(c)
    ix, iy = ic // 128, ic % 128
    sx, sy = H / 128, W / 128
    ix = (ix * sx + u1 * sx).long().clamp(max=H - 1)
    iy = (iy * sy + u2 * sy).long().clamp(max=W - 1)
    assert np.array_equal(ix.numpy(), rows) and np.array_equal(iy.numpy(), cols)


# ---------------------------------------------------------------- rays
def _poses(n, seed=0):
    from focnerf_amd import synthetic
    return synthetic.rand_poses(n, "cpu", radius=2.0, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("H,W", [(5, 7), (800, 800)])
def test_rays_against_the_torch_statement(H, W):
    from focnerf_amd import synthetic
    poses, intr = _poses(3), synthetic.intrinsics(H, W)
    inds = batch_ref.pixel_inds(0, 0, 256, H, W)
    for v in range(3):
        ro, rd = synthetic.get_rays(poses[v:v + 1], intr, H, W, torch.from_numpy(inds)[None])
        o64, d64 = batch_ref.rays64(poses[v].numpy(), intr, inds // W, inds % W)
        assert np.array_equal(ro[0].numpy(), o64.astype(np.float32))
        err = np.abs(rd[0].numpy().astype(np.float64) - d64).max()
        print(f"{H}x{W} view {v}: torch fp32 vs float64 {err / U:.2f} U (bound 16 U)")
        assert err <= batch_ref.RAY_BOUND


@pytest.mark.parametrize("mutant", [dict(half=0.0), dict(swap=True), dict(transpose=True)])
def test_ray_mutants_fall_outside_the_bound(mutant):
    from focnerf_amd import synthetic
    H, W = 5, 7
    poses, intr = _poses(1, seed=1), synthetic.intrinsics(H, W)
    inds = np.arange(H * W)
    _, good = batch_ref.rays64(poses[0].numpy(), intr, inds // W, inds % W)
    _, bad = batch_ref.rays64(poses[0].numpy(), intr, inds // W, inds % W, **mutant)
    assert np.abs(good - bad).max() > 1000 * batch_ref.RAY_BOUND


# ---------------------------------------------------------------- pixels, colour space, blend
def test_pixel_values_and_the_linear_conversion():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(batch_ref.pixel_values(v), (torch.arange(256, dtype=torch.float32) / 255).numpy())
    h = np.linspace(0, 1, 33).astype(np.float16)
    assert np.array_equal(batch_ref.pixel_values(h), torch.from_numpy(h).float().numpy())
    x = torch.linspace(0, 1, 1001, dtype=torch.float64)
    ref = torch.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)             # nerf/utils.py:52-53
    np.testing.assert_allclose(batch_ref.srgb_to_linear64(x.numpy()), ref.numpy(), rtol=1e-14, atol=0)


def test_blend_against_the_torch_lines():
    rng = np.random.default_rng(2)
    images = torch.from_numpy(rng.random((1, 300, 4)).astype(np.float32))
    images[0, :5, 3] = torch.tensor([0.0, 1.0, 0.5, 1.0, 0.0])
    bg = torch.from_numpy(rng.random((1, 300, 3)).astype(np.float32))
    for bg_color in (bg, 1):
        gt = images[..., :3] * images[..., 3:] + bg_color * (1 - images[..., 3:])       # nerf/utils.py:856
        b = bg[0].numpy() if torch.is_tensor(bg_color) else np.float32(1)
        mine = batch_ref.blend32(images[0, :, :3].numpy(), images[0, :, 3:].numpy(), b)
        assert mine.dtype == np.float32 and np.array_equal(mine, gt[0].numpy())
        ref64 = batch_ref.blend64(images[0, :, :3].numpy(), images[0, :, 3:].numpy(), b)
        assert np.abs(mine - ref64).max() <= 4 * U
        mutant = batch_ref.blend64(images[0, :, :3].numpy(), images[0, :, 3:].numpy(), b, drop_one_minus=True)
        assert np.abs(mutant - ref64).max() > 1e-2


# ---------------------------------------------------------------- loss
def _pred_gt(n, seed=3):
    rng = np.random.default_rng(seed)
    p, g = rng.random((n, 3)), rng.random((n, 3))
    p[: n // 4] = g[: n // 4] + rng.uniform(-0.1, 0.1, (n // 4, 3))                      # both sides of Huber's delta = 0.1
    return p.astype(np.float32), g.astype(np.float32)


@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_and_gradient_against_torch(kind):
    p32, g32 = _pred_gt(257)
    delta = float(np.float32(0.1))
    tp = torch.tensor(p32, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(g32, dtype=torch.float64)
    crit = torch.nn.MSELoss(reduction="none") if kind == "mse" else torch.nn.HuberLoss(reduction="none", delta=delta)
    ray = crit(tp, tg).mean(-1)                                                          # nerf/utils.py:867
    loss = ray.mean()                                                                    # :899
    loss.backward()
    ray64, grad64, loss64 = batch_ref.loss64(p32, g32, kind, 0.1)
    np.testing.assert_allclose(ray64, ray.detach().numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(grad64, tp.grad.numpy(), rtol=1e-12, atol=1e-300)
    assert abs(loss64 - loss.item()) <= 1e-12 * loss.item()
    # the fp32 statement lies inside the bounds
    ray32, grad32 = batch_ref.loss32(p32, g32, kind, 0.1)
    assert ray32.dtype == np.float32 and grad32.dtype == np.float32
    assert abs(float(ray32.astype(np.float64).mean()) - loss64) <= batch_ref.loss_bound(loss64, kind)
    assert (np.abs(grad32 - grad64) <= batch_ref.grad_bound(grad64, p32, g32, kind)).all()
    # the mean over 2 of the 3 channels falls outside
    ray_m, grad_m, loss_m = batch_ref.loss64(p32, g32, kind, 0.1, channels=2)
    assert abs(loss_m - loss64) > 1000 * batch_ref.loss_bound(loss64, kind)
    assert (np.abs(grad_m - grad64) > batch_ref.grad_bound(grad64, p32, g32, kind)).mean() > 0.9


def test_fp16_predictions_are_widened_exactly():
    p32, g32 = _pred_gt(64)
    p16 = p32.astype(np.float16)
    a = batch_ref.loss32(p16, g32)
    b = batch_ref.loss32(p16.astype(np.float32), g32)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_ema_against_gather_and_scatter():
    rng = np.random.default_rng(4)
    emap = torch.from_numpy(rng.random((3, 16384)).astype(np.float32))
    inds = torch.from_numpy(rng.permutation(16384)[:300])[None]
    error = torch.from_numpy(rng.random((1, 300)).astype(np.float32))
    index = [1]
    row = emap[index].clone()                                                            # nerf/utils.py:887-897
    ema = 0.1 * row.gather(1, inds) + 0.9 * error
    row.scatter_(1, inds, ema)
    want = emap.clone()
    want[index] = row
    mine = batch_ref.error_map_update32(emap.numpy(), 1, inds.numpy(), error[0].numpy())
    assert np.array_equal(mine, want.numpy())
    old = emap[1, inds[0]].numpy()
    assert np.abs(batch_ref.ema32(old, error[0].numpy()) - batch_ref.ema64(old, error[0].numpy())).max() <= 4 * U
    assert np.abs(batch_ref.ema64(old, error[0].numpy(), swapped=True) - batch_ref.ema64(old, error[0].numpy())).max() > 1e-2


def test_a_whole_reference_batch_holds_together():
    rng = np.random.default_rng(5)
    images = rng.integers(0, 256, (3, 5, 7, 4), dtype=np.uint8)
    poses = _poses(3).numpy()
    intr = (6.0, 6.5, 3.5, 2.5)
    b0 = batch_ref.sample(images, poses, intr, [2, 0, 1], 0, 0, 63, clamp=False)
    b4 = batch_ref.sample(images, poses, intr, [2, 0, 1], 0, 4, 63, clamp=False)
    assert b0["view"] == 2 and b4["view"] == 0 and b0["gt"].dtype == np.float32 and b0["gt"].shape == (63, 3)
    assert not np.array_equal(b0["inds"], b4["inds"]) and not np.array_equal(b0["bg"], b4["bg"])
    assert batch_ref.sample(images, poses, intr, [2, 0, 1], 0, 0, 1000)["inds"].shape == (35,)      # N is clamped to H * W
    lin = batch_ref.sample(images, poses, intr, [2, 0, 1], 0, 0, 63, linear=True, clamp=False)
    assert np.array_equal(lin["inds"], b0["inds"]) and (lin["gt64"] <= b0["gt"] + 1e-6).all() and (lin["gt_bound"] < 8 * U).all()
    white = batch_ref.sample(images[..., :3], poses, intr, [2, 0, 1], 0, 0, 63, clamp=False)
    assert (white["bg"] == 1).all() and np.array_equal(white["gt"], batch_ref.pixel_values(images[2].reshape(35, 4)[b0["inds"], :3]))


# ---------------------------------------------------------------- the C ABI: refusals on the host, before any launch
def test_host_side_refusals_of_the_three_entry_points():
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)                                       # never dereferenced: validation fails first
    bw, lw = lib.foc_batch_workspace_bytes(), lib.foc_photo_loss_workspace_bytes()
    assert bw >= 4 and lw >= 8 * 256

    def sample(images=one, dtype=_lib.FOC_U8, V=3, H=5, W=7, C=4, N=63, ws=one, ws_bytes=bw, wgs=0, fx=6.0):
        return lib.foc_batch_sample(images, dtype, V, H, W, C, one, fx, 6.0, 3.5, 2.5, one, one, 0, N, None, 1, 0, one, one, one, one, one, one, ws, ws_bytes,
                                    wgs, None)
    assert sample(images=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert sample(ws=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert sample(C=2) == 1 and b"C must be 3 or 4" in lib.foc_last_error()
    assert sample(C=5) == 1 and b"C must be 3 or 4" in lib.foc_last_error()
    assert sample(dtype=3) == 2 and b"dtype" in lib.foc_last_error()
    assert sample(N=0) == 1 and b"N must be" in lib.foc_last_error()
    assert sample(H=32768, W=32769) == 1 and b"2^30" in lib.foc_last_error()
    assert sample(H=0) == 1 and b"2^30" in lib.foc_last_error()
    assert sample(V=0) == 1 and b"V must be" in lib.foc_last_error()
    assert sample(fx=0.0) == 1 and b"intrinsics" in lib.foc_last_error()
    assert sample(ws_bytes=bw - 1) == 1 and b"workspace of" in lib.foc_last_error()
    assert sample(wgs=1025) == 1 and b"workgroups" in lib.foc_last_error()

    assert lib.foc_view_rays(None, 6.0, 6.0, 3.5, 2.5, 5, 7, one, one, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_view_rays(one, 6.0, 6.0, 3.5, 2.5, 5, 7, one, None, None) == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_view_rays(one, 6.0, 6.0, 3.5, 2.5, 65536, 16385, one, one, None) == 1 and b"2^30" in lib.foc_last_error()
    assert lib.foc_view_rays(one, 6.0, float("nan"), 3.5, 2.5, 5, 7, one, one, None) == 1 and b"intrinsics" in lib.foc_last_error()

    def loss(pred=one, dtype=_lib.FOC_F32, N=63, kind=0, delta=0.1, emap=None, V=0, view=None, coarse=None, ws=one, ws_bytes=lw):
        return lib.foc_photo_loss(pred, dtype, one, N, kind, delta, emap, V, view, coarse, one, one, one, ws, ws_bytes, None)
    assert loss(pred=None) == 1 and b"null pointer" in lib.foc_last_error()
    assert loss(dtype=_lib.FOC_U8) == 2 and b"dtype" in lib.foc_last_error()
    assert loss(kind=2) == 1 and b"kind" in lib.foc_last_error()
    assert loss(kind=1, delta=0.0) == 1 and b"delta" in lib.foc_last_error()
    assert loss(N=0) == 1 and b"N must be" in lib.foc_last_error()
    assert loss(emap=one, V=3) == 1 and b"null pointer" in lib.foc_last_error()
    assert loss(emap=one, V=0, view=one, coarse=one) == 1 and b"V must be" in lib.foc_last_error()
    assert loss(ws_bytes=lw - 8) == 1 and b"workspace of" in lib.foc_last_error()
    assert loss(ws=ctypes.c_void_p(4)) == 1 and b"workspace of" in lib.foc_last_error()


# ---------------------------------------------------------------- the Python layer without a device
def test_exports():
    import focnerf_amd
    from focnerf_amd import batch
    assert focnerf_amd.DeviceDataset is batch.DeviceDataset and focnerf_amd.RaySampler is batch.RaySampler and focnerf_amd.photo_loss is batch.photo_loss
    for name in ("batch", "DeviceDataset", "RaySampler", "photo_loss"):
        assert name in focnerf_amd.__all__


def test_device_dataset_refuses_cpu_tensors_and_wrong_shapes():
    from focnerf_amd import DeviceDataset, RaySampler, photo_loss
    images, poses, intr = torch.zeros(3, 5, 7, 4, dtype=torch.uint8), torch.eye(4).repeat(3, 1, 1), (6.0, 6.0, 3.5, 2.5)
    with pytest.raises(ValueError, match="no CPU implementation"):
        DeviceDataset(images, poses, intr)
    with pytest.raises(ValueError, match="must be a tensor"):
        DeviceDataset(images.numpy(), poses, intr)
    with pytest.raises(ValueError, match="must be a DeviceDataset"):
        RaySampler(images)
    with pytest.raises(ValueError, match="no CPU implementation"):
        photo_loss(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="kind must be"):
        photo_loss(torch.zeros(4, 3), torch.zeros(4, 3), kind="l1")


@pytest.mark.parametrize("what,message", [("dtype", "uint8, float16 or float32"), ("dims", r"\[V,H,W,3\] or \[V,H,W,4\]"), ("channels", r"\[V,H,W,3\] or \[V,H,W,4\]"),
                                          ("poses_shape", r"poses \[3,4,4\]"), ("poses_dtype", "poses must be float32"), ("intrinsics", "four numbers"),
                                          ("fx", "fx and fy not zero"), ("color_space", "'srgb' or 'linear'"), ("good", "no CPU implementation")])
def test_device_dataset_shape_checks(what, message):
    """Shapes, dtypes, intrinsics and the colour space are checked before the devices, so a CPU-only host reaches every one of them;
    the good case then fails on the device check alone."""
    from focnerf_amd import DeviceDataset
    images, poses, intr, cs = torch.zeros(3, 5, 7, 4, dtype=torch.uint8), torch.eye(4).repeat(3, 1, 1), (6.0, 6.0, 3.5, 2.5), "srgb"
    if what == "dtype":
        images = images.to(torch.int32)
    elif what == "dims":
        images = images[0]
    elif what == "channels":
        images = images[..., :2]
    elif what == "poses_shape":
        poses = poses[:2]
    elif what == "poses_dtype":
        poses = poses.double()
    elif what == "intrinsics":
        intr = (6.0, 6.0, 3.5)
    elif what == "fx":
        intr = (0.0, 6.0, 3.5, 2.5)
    elif what == "color_space":
        cs = "rgb"
    with pytest.raises(ValueError, match=message):
        DeviceDataset(images, poses, intr, cs)
