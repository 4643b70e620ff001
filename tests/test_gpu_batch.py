"""GPU: focnerf_amd.batch (csrc/batch.hip) against tests/batch_ref.py — the sampler bit for bit where the arithmetic is exact or stated
operation by operation, within counted bounds where it is not; the loss likewise; a captured graph that draws batch t, t + 1, t + 2 by
itself; and the whole step on the real training path, eager against replayed. The bounds and their derivation are in batch_ref.py."""
import contextlib

import numpy as np
import pytest
import torch

import batch_ref
from batch_ref import U

pytestmark = pytest.mark.gpu

ORDER = [2, 0, 1]
NS = [1, 63, 255, 256, 257]                     # both sides of a wave and of a workgroup
LOSS_NS = NS + [256 * 256 + 257]                # and more rays than the capped grid (256 workgroups) covers in one pass


@contextlib.contextmanager
def no_sync():
    """Any host synchronisation inside the block is an error (where torch has the switch)."""
    has = hasattr(torch.cuda, "set_sync_debug_mode")
    if has:
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        if has:
            torch.cuda.set_sync_debug_mode("default")


_DATA = {}


def _data(H, W, C, dtype, V=3):
    """Images (numpy, in the dtype the device gets), poses (numpy fp32) and intrinsics; made once per shape and never changed."""
    key = (H, W, C, dtype, V)
    if key not in _DATA:
        from focnerf_amd import synthetic
        rng = np.random.default_rng(H * 1000 + W * 10 + C)
        u8 = rng.integers(0, 256, (V, H, W, C), dtype=np.uint8)
        u8.reshape(-1, C)[:4] = [[0] * C, [255] * C, [10] * C, [11] * C]            # both ends, and both sides of the linear conversion's knee
        if C == 4:
            u8[0, 0, :3, 3] = [0, 255, 128]
        images = u8 if dtype == "uint8" else (u8.astype(np.float32) / np.float32(255)).astype(dtype)
        poses = synthetic.rand_poses(V, "cpu", radius=2.0, generator=torch.Generator().manual_seed(H)).numpy()
        _DATA[key] = (images, poses, tuple(float(np.float32(v)) for v in synthetic.intrinsics(H, W)))
    return _DATA[key]


def _sampler(H, W, C, dtype, N, color_space="srgb", seed=7, **kw):
    from focnerf_amd import DeviceDataset, RaySampler
    images, poses, intr = _data(H, W, C, dtype)
    ds = DeviceDataset(torch.from_numpy(images).cuda(), torch.from_numpy(poses).cuda(), intr, color_space)
    s = RaySampler(ds, num_rays=N, seed=seed, **kw)
    s.order.copy_(torch.tensor(ORDER, dtype=torch.int32))
    return s


def _np(t):
    return t.detach().cpu().numpy()


def _check_batch(b, ref, linear, what):
    n = ref["inds"].shape[0]
    assert np.array_equal(_np(b.inds), ref["inds"][None]), what
    assert int(b.view) == ref["view"], what
    assert b.rays_o.shape == (1, n, 3) and b.rays_d.shape == (1, n, 3) and b.gt_rgb.shape == (1, n, 3) and b.inds.dtype == torch.int64
    assert np.array_equal(_np(b.rays_o)[0], ref["rays_o"].astype(np.float32)), what
    err = np.abs(_np(b.rays_d)[0].astype(np.float64) - ref["rays_d"]).max()
    print(f"{what}: rays_d {err / U:.2f} U (bound 16 U)")
    assert err <= batch_ref.RAY_BOUND, what
    if not linear:
        assert np.array_equal(_np(b.gt_rgb)[0].view(np.uint32), ref["gt"].view(np.uint32)), what
    else:
        d = np.abs(_np(b.gt_rgb)[0].astype(np.float64) - ref["gt64"])
        print(f"{what}: linear gt max {np.max(d / np.maximum(ref['gt_bound'], 1e-300)):.3f} of its bound")
        assert (d <= ref["gt_bound"]).all(), what


# ---------------------------------------------------------------- the sampler
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("dtype", ["uint8", "float16", "float32"])
def test_batches_follow_the_reference(dtype, C, N):
    """A 5 x 7 image, three views in the order 2, 0, 1, four steps (so `step mod V` wraps), both colour spaces: inds, view, bg_color and
    gt_rgb ('srgb') bit-equal, 'linear' within one ulp through the blend, rays within 16 U, rays_o exact; the step advances by one per
    call and the ticket word is zero after each; another launch size gives the same bits. (N above the 35 pixels: clamp=False.)"""
    H, W = 5, 7
    images, poses, intr = _data(H, W, C, dtype)
    for cs in ("srgb", "linear"):
        s = _sampler(H, W, C, dtype, N, cs, clamp=False)
        assert s.num_rays == N
        kept = []
        for step in range(4):
            with no_sync():
                b = s.next()
            assert int(s.step) == step + 1 and int(s._ws[0]) == 0
            ref = batch_ref.sample(images, poses, intr, ORDER, 7, step, N, linear=cs == "linear", clamp=False)
            _check_batch(b, ref, cs == "linear", f"{dtype} C={C} N={N} {cs} step {step}")
            if C == 4:
                assert torch.is_tensor(b.bg_color) and np.array_equal(_np(b.bg_color)[0].view(np.uint32), ref["bg"].view(np.uint32))
            else:
                assert b.bg_color == 1.0 and (s._bg == 1).all()
            assert b.inds_coarse is None
            kept.append([t.clone() for t in (b.inds, b.rays_o, b.rays_d, b.gt_rgb, s._bg, b.view)])
        assert N == 1 or not torch.equal(kept[0][0], kept[3][0]), "steps 0 and 3 share a view and must still differ"
        # the same tensors every time, and the same bits from another launch size
        again = s.next()
        assert again.rays_d.data_ptr() == b.rays_d.data_ptr() and again.inds.data_ptr() == b.inds.data_ptr()
        for step in (0, 3):
            s.step.fill_(step)
            b = s.next(workgroups=3)
            assert int(s.step) == step + 1 and int(s._ws[0]) == 0
            for got, want in zip((b.inds, b.rays_o, b.rays_d, b.gt_rgb, s._bg, b.view), kept[step]):
                assert torch.equal(got.view(torch.int32) if got.dtype == torch.float32 else got, want.view(torch.int32) if want.dtype == torch.float32 else want)


def test_a_fixed_white_background_and_the_clamp():
    """random_bg=False: the blend runs against 1 and bg_color is the float 1; num_rays is clamped to H * W as the reference does."""
    images, poses, intr = _data(5, 7, 4, "uint8")
    s = _sampler(5, 7, 4, "uint8", 4096, random_bg=False)
    assert s.num_rays == 35
    b = s.next()
    ref = batch_ref.sample(images, poses, intr, ORDER, 7, 0, 4096, random_bg=False)
    _check_batch(b, ref, False, "white")
    assert b.bg_color == 1.0 and (ref["bg"] == 1).all()


def test_the_index_range_of_an_800_by_800_view():
    images, poses, intr = _data(800, 800, 4, "uint8")
    s = _sampler(800, 800, 4, "uint8", 4096)
    for step in range(2):
        with no_sync():
            b = s.next()
        ref = batch_ref.sample(images, poses, intr, ORDER, 7, step, 4096)
        _check_batch(b, ref, False, f"800x800 step {step}")
        assert np.array_equal(_np(b.bg_color)[0].view(np.uint32), ref["bg"].view(np.uint32))
    assert ref["inds"].max() > 600000 and ref["view"] == 0


@pytest.mark.parametrize("H,W,N,clamp", [(5, 7, 35, True), (5, 7, 257, False), (800, 800, 4096, True)])
def test_the_error_map_route(H, W, N, clamp):
    """inds_coarse is torch's draw (distinct cells of the view's row); given it, the pixels are the reference's bit for bit, inside
    their cell and the image; the loss then updates exactly those cells of exactly that row."""
    from focnerf_amd import photo_loss
    images, poses, intr = _data(H, W, 4, "uint8")
    s = _sampler(H, W, 4, "uint8", N, error_map=True, clamp=clamp)
    s.error_map.copy_(torch.rand(3, 16384, generator=torch.Generator().manual_seed(1)) + 0.01)
    for step in range(2):
        before = _np(s.error_map).copy()
        with no_sync():
            b = s.next()
        coarse = _np(b.inds_coarse)[0]
        assert b.inds_coarse.shape == (1, N) and len(set(coarse.tolist())) == N and coarse.min() >= 0 and coarse.max() < 16384
        ref = batch_ref.sample(images, poses, intr, ORDER, 7, step, N, inds_coarse=coarse, clamp=clamp)
        _check_batch(b, ref, False, f"error map {H}x{W} step {step}")
        assert (ref["rows"] < H).all() and (ref["cols"] < W).all()
        assert (np.abs(ref["rows"] + 0.5 - (coarse // 128 + 0.5) * (H / 128)) <= 0.5 * H / 128 + 0.5 + 1e-3).all()      # the pixel's centre within half a
        assert (np.abs(ref["cols"] + 0.5 - (coarse % 128 + 0.5) * (W / 128)) <= 0.5 * W / 128 + 0.5 + 1e-3).all()       # cell (+ half a pixel) of the cell's
        pred = torch.rand(1, N, 3, generator=torch.Generator().manual_seed(step)).cuda()
        with no_sync():
            loss, ray_loss = photo_loss(pred, b.gt_rgb, error_map=(s.error_map, b.view, b.inds_coarse))
        rl, _ = batch_ref.loss32(_np(pred)[0], _np(b.gt_rgb)[0])
        want = batch_ref.error_map_update32(before, ref["view"], coarse, rl)
        assert np.array_equal(_np(s.error_map).view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(want[ref["view"]], before[ref["view"]])


def test_view_rays_are_the_sampled_rays():
    """All rays of a view, row-major: within the bound of the float64 statement, and bit for bit the sampler's rays at its pixels."""
    for H, W in ((5, 7), (800, 800)):
        images, poses, intr = _data(H, W, 3, "uint8")
        s = _sampler(H, W, 3, "uint8", 256, clamp=False)
        b = s.next()
        v = int(b.view)
        with no_sync():
            ro, rd = s.view_rays(v)
        assert ro.shape == (1, H * W, 3) and rd.shape == (1, H * W, 3)
        pix = np.arange(H * W)
        o64, d64 = batch_ref.rays64(poses[v], intr, pix // W, pix % W)
        assert np.array_equal(_np(ro)[0], o64.astype(np.float32))
        assert np.abs(_np(rd)[0].astype(np.float64) - d64).max() <= batch_ref.RAY_BOUND
        assert torch.equal(rd[0][b.inds[0]].view(torch.int32), b.rays_d[0].view(torch.int32))
        assert torch.equal(ro[0][b.inds[0]].view(torch.int32), b.rays_o[0].view(torch.int32))
    with pytest.raises(ValueError, match="view 3 of 3"):
        s.view_rays(3)


def test_shuffle_and_the_state_dict():
    s = _sampler(5, 7, 4, "uint8", 33, error_map=True)
    s.shuffle(torch.Generator().manual_seed(0))
    assert sorted(s.order.tolist()) == [0, 1, 2]
    s.next()
    s.next()
    s.error_map[1, 5] = 0.25
    state = s.state_dict()
    assert set(state) == {"seed", "step", "order", "error_map"} and state["step"] == 2 and state["seed"] == 7 and not state["order"].is_cuda
    t = _sampler(5, 7, 4, "uint8", 33, seed=0, error_map=True)
    t.load_state_dict(state)
    assert int(t.step) == 2 and t.seed == 7 and torch.equal(t.order, s.order) and torch.equal(t.error_map, s.error_map)
    # a resumed run continues the sequence (the error-map draw is torch's: hand both the same cells)
    plain, resumed = _sampler(5, 7, 4, "uint8", 33), _sampler(5, 7, 4, "uint8", 33, seed=0)
    plain.next()
    plain.next()
    st = plain.state_dict()
    assert st["error_map"] is None
    resumed.load_state_dict(st)
    a, b = plain.next(), resumed.next()
    assert torch.equal(a.inds, b.inds) and torch.equal(a.gt_rgb, b.gt_rgb) and torch.equal(a.view, b.view)
    with pytest.raises(ValueError, match="permutation"):
        resumed.load_state_dict(dict(st, order=torch.tensor([0, 0, 1])))
    with pytest.raises(ValueError, match="error map"):
        resumed.load_state_dict(state)


# ---------------------------------------------------------------- the loss
def _pred_gt(n, seed):
    rng = np.random.default_rng(seed)
    p, g = rng.random((n, 3)), rng.random((n, 3))
    q = max(n // 4, 1)
    p[:q] = g[:q] + rng.uniform(-0.1, 0.1, (q, 3))                                   # both sides of Huber's delta = 0.1
    return p.astype(np.float32), g.astype(np.float32)


@pytest.mark.parametrize("N", LOSS_NS)
@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_loss_gradient_and_mean(kind, N):
    """ray_loss and grad bit-equal to the fp32 statement; loss within its bound of float64; two runs the same bits; fp16 predictions as
    their widened values; backward under LossScaler at scale 1024 exactly grad * 1024 — all without a host synchronisation."""
    from focnerf_amd import LossScaler, photo_loss
    p32, g32 = _pred_gt(N, N)
    ray_ref, grad_ref = batch_ref.loss32(p32, g32, kind, 0.1)
    _, grad64, loss64 = batch_ref.loss64(p32, g32, kind, 0.1)
    pred = torch.from_numpy(p32).cuda()[None].requires_grad_(True)
    gt = torch.from_numpy(g32).cuda()[None]
    scaler = LossScaler(init_scale=1024.0)
    scaler._on(pred.device)
    photo_loss(pred.detach(), gt, kind)                                              # the workspace exists from here on
    with no_sync():
        loss, ray_loss = photo_loss(pred, gt, kind, delta=0.1)
        loss2, ray_loss2 = photo_loss(pred.detach(), gt, kind, delta=0.1)
        scaler.scale(loss).backward()
    assert loss.shape == () and loss.dtype == torch.float32 and ray_loss.shape == (1, N) and not ray_loss.requires_grad
    assert np.array_equal(_np(ray_loss)[0].view(np.uint32), ray_ref.view(np.uint32))
    assert np.array_equal(_np(pred.grad)[0].view(np.uint32), (grad_ref * np.float32(1024)).view(np.uint32))
    assert (np.abs(grad_ref.astype(np.float64) - grad64) <= batch_ref.grad_bound(grad64, p32, g32, kind)).all()
    err = abs(float(loss.detach()) - loss64)
    print(f"{kind} N={N}: loss {float(loss.detach()):.8f}, {err / (U * loss64):.2f} U of {batch_ref.LOSS_BOUND[kind] / U:.0f} U")
    assert err <= batch_ref.loss_bound(loss64, kind)
    assert torch.equal(loss.detach().view(torch.int32), loss2.view(torch.int32)) and torch.equal(ray_loss, ray_loss2)
    # fp16 predictions
    p16 = torch.from_numpy(p32.astype(np.float16)).cuda()[None].requires_grad_(True)
    with no_sync():
        l16, r16 = photo_loss(p16, gt, kind)
        l16w, r16w = photo_loss(p16.detach().float(), gt, kind)
        l16.backward()
    assert torch.equal(l16.detach().view(torch.int32), l16w.view(torch.int32)) and torch.equal(r16, r16w) and p16.grad.dtype == torch.float16
    r16_ref, g16_ref = batch_ref.loss32(p32.astype(np.float16), g32, kind, 0.1)
    assert np.array_equal(_np(r16)[0].view(np.uint32), r16_ref.view(np.uint32))
    assert np.array_equal(_np(p16.grad)[0], g16_ref.astype(np.float16))


def test_loss_refusals():
    from focnerf_amd import photo_loss
    p, g = torch.zeros(4, 3, device="cuda"), torch.zeros(4, 3, device="cuda")
    for bad in (lambda: photo_loss(p.double(), g), lambda: photo_loss(p, g.half()), lambda: photo_loss(p[:, :2], g[:, :2]), lambda: photo_loss(p, g[:3]),
                lambda: photo_loss(p, g, kind="huber", delta=0.0),
                lambda: photo_loss(p, g, error_map=(torch.ones(3, 100, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")))):
        with pytest.raises(ValueError, match="photo_loss"):
            bad()


# ---------------------------------------------------------------- graphs
def test_a_replayed_graph_draws_the_next_batch_by_itself():
    """next() + photo_loss captured once with a stand-in prediction computed from the rays; three replays, read after each: batches t,
    t + 1, t + 2 of the reference, all different; the capture itself advances nothing."""
    from focnerf_amd import photo_loss
    N = 257
    images, poses, intr = _data(5, 7, 4, "uint8")
    s = _sampler(5, 7, 4, "uint8", N, clamp=False)

    def step():
        b = s.next()
        pred = b.rays_d * 0.5 + 0.5
        loss, ray_loss = photo_loss(pred, b.gt_rgb)
        return b, pred, loss, ray_loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                                       # step 0 eagerly: the loss's workspace exists
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            b, pred, loss, ray_loss = step()
        torch.cuda.synchronize()
        assert int(s.step) == 1 and int(s._ws[0]) == 0, "a capture executes nothing"
        seen = []
        for t in (1, 2, 3):
            graph.replay()
            torch.cuda.synchronize()
            assert int(s.step) == t + 1 and int(s._ws[0]) == 0
            ref = batch_ref.sample(images, poses, intr, ORDER, 7, t, N, clamp=False)
            _check_batch(b, ref, False, f"replay {t}")
            assert np.array_equal(_np(b.bg_color)[0].view(np.uint32), ref["bg"].view(np.uint32))
            rl, _ = batch_ref.loss32(_np(pred)[0], _np(b.gt_rgb)[0])
            assert np.array_equal(_np(ray_loss)[0].view(np.uint32), rl.view(np.uint32))
            l64 = batch_ref.loss64(_np(pred)[0], _np(b.gt_rgb)[0])[2]
            assert abs(float(loss) - l64) <= batch_ref.loss_bound(l64)
            seen.append((_np(b.inds).copy(), float(loss)))
        assert not np.array_equal(seen[0][0], seen[1][0]) and not np.array_equal(seen[1][0], seen[2][0]) and len({v for _, v in seen}) == 3
    torch.cuda.current_stream().wait_stream(side)


def test_the_whole_step_on_the_real_training_path():
    """NeRFNetwork(bound=1).run(fused=True), 64 rays of an 8 x 8 dataset, 64 steps per ray, fp16 autocast, deterministic mode,
    perturb=False. The step: sampler.next(), run(bg_color=b.bg_color), photo_loss, LossScaler, FusedAdam.step(scaler=..., zero_grads=True).
    Both runs start from the same seed, take one warm-up step (it sizes the scratch buffers and creates the optimizer state, which a capture
    may not do) and put parameters, moments, counters, scale and the sampler's step back; then three steps eagerly against one captured
    graph replayed three times: losses and parameters bit-equal, and the parameters did move.
    Not asserted: a falling loss. The targets are noise images of three different views and a run is three steps, so "step 3 below step
    1" says nothing robust at this size; it is left out rather than loosened."""
    import focnerf_amd
    from focnerf_amd import DeviceDataset, FusedAdam, LossScaler, RaySampler, photo_loss, synthetic
    from focnerf_amd.network import NeRFNetwork

    def run(graphed):
        torch.manual_seed(5)
        gen = torch.Generator().manual_seed(5)
        m = NeRFNetwork(bound=1).cuda().train()
        poses = synthetic.rand_poses(3, "cuda", radius=2.0, generator=gen)
        images = torch.rand(3, 8, 8, 4, generator=gen).cuda()
        sampler = RaySampler(DeviceDataset(images, poses, synthetic.intrinsics(8, 8)), num_rays=64, seed=5)
        opt = FusedAdam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
        scaler = LossScaler(init_scale=1024.0)

        def step():
            b = sampler.next()
            with torch.autocast("cuda", dtype=torch.float16):
                out = m.run(b.rays_o, b.rays_d, None, fused=True, num_steps=64, upsample_steps=0, bg_color=b.bg_color, perturb=False)
            loss, _ = photo_loss(out["image"], b.gt_rgb)
            scaler.scale(loss).backward()
            opt.step(scaler=scaler, zero_grads=True)
            return loss.detach()

        params = [p for g in opt.param_groups for p in g["params"]]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        losses = []
        with focnerf_amd.deterministic(), torch.cuda.stream(side):
            start = [p.detach().clone() for p in params]
            step()                                                                   # the warm-up step, then everything back to the start
            torch.cuda.synchronize()
            with torch.no_grad():
                for p, p0 in zip(params, start):
                    p.copy_(p0)
                    if p in opt.state:
                        for k in ("step", "exp_avg", "exp_avg_sq"):
                            opt.state[p][k].zero_()
                scaler._scale.fill_(1024.0)
                scaler._growth_tracker.zero_()
                sampler.step.zero_()
            torch.cuda.synchronize()
            if graphed:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    out = step()
                torch.cuda.synchronize()
                assert int(sampler.step) == 0 and all(torch.equal(p.detach(), p0) for p, p0 in zip(params, start)), "a capture executes nothing"
            for _ in range(3):
                if graphed:
                    graph.replay()
                else:
                    out = step()
                torch.cuda.synchronize()
                losses.append(out.clone())
            assert int(sampler.step) == 3
        torch.cuda.current_stream().wait_stream(side)
        return losses, [p.detach().clone() for p in params], start

    le, pe, start = run(False)
    lg, pg, _ = run(True)
    assert all(torch.isfinite(v) for v in le) and len({float(v) for v in le}) == 3
    assert sum(not torch.equal(p, p0) for p, p0 in zip(pe, start)) >= 3, "the steps did update the parameters"
    for a, b in zip(le, lg):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (le, lg)
    for p, q in zip(pe, pg):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32))
