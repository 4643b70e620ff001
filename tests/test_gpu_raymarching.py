"""GPU parity: raymarching ops (through the Python operator API -> C ABI -> HIP kernels) vs the CPU oracle.
Integer / index / control-flow results are bit-exact; compositing (uses __expf, wave-parallel sums) is
within 1e-4 absolute — the tolerance north_star states for RGB/sigma."""
import numpy as np
import pytest
import torch

import march_ref
import oracle
from util import scene, to_np

pytestmark = pytest.mark.gpu

RGB_TOL = 1e-4


@pytest.fixture(scope="module")
def rm():
    from focnerf_amd import raymarching
    return raymarching


@pytest.mark.parametrize("N", [1, 63, 257, 4096, 100003])
def test_near_far_from_aabb_bit_exact(rm, N):
    s = scene(2, 4096, seed=1)
    g = torch.Generator().manual_seed(N)
    o = (torch.rand(N, 3, generator=g) - 0.5) * 6
    d = torch.randn(N, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    if N > 8:
        d[3] = torch.tensor([0.0, 0.0, 1.0])      # axis-aligned: 1/0 = inf paths
        d[5] = torch.tensor([-0.0, 1.0, 0.0])
    n_ref, f_ref = oracle.near_far_from_aabb(o.numpy(), d.numpy(), s["aabb"].numpy(), 0.2)
    n, f = rm.near_far_from_aabb(o.cuda(), d.cuda(), s["aabb"].cuda(), 0.2)
    assert np.array_equal(to_np(n).view(np.uint32), n_ref.view(np.uint32))
    assert np.array_equal(to_np(f).view(np.uint32), f_ref.view(np.uint32))


def test_near_far_empty(rm):
    n, f = rm.near_far_from_aabb(torch.zeros(0, 3).cuda(), torch.zeros(0, 3).cuda(), torch.tensor([-1., -1, -1, 1, 1, 1]).cuda(), 0.2)
    assert n.shape == (0,) and f.shape == (0,)


def test_sph_from_ray(rm):
    g = torch.Generator().manual_seed(0)
    o = (torch.rand(1000, 3, generator=g) - 0.5)
    d = torch.randn(1000, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    ref = oracle.sph_from_ray(o.numpy(), d.numpy(), 3.0)
    got = to_np(rm.sph_from_ray(o.cuda(), d.cuda(), 3.0))
    np.testing.assert_allclose(got, ref, atol=2e-6)     # atan2/sqrt: libm vs ocml


def test_morton_bit_exact_and_round_trip(rm):
    g = torch.Generator().manual_seed(0)
    c = torch.randint(0, 128, (128 ** 3 // 8 + 5, 3), generator=g, dtype=torch.int32)
    idx = rm.morton3D(c.cuda())
    assert np.array_equal(to_np(idx), oracle.morton3D(c.numpy()))
    back = rm.morton3D_invert(idx)
    assert np.array_equal(to_np(back), c.numpy())
    # the full 128^3 lattice is a permutation of [0, 128^3)
    ar = torch.arange(128, dtype=torch.int32)
    full = torch.stack(torch.meshgrid(ar, ar, ar, indexing="ij"), -1).reshape(-1, 3).cuda()
    m = rm.morton3D(full).long()
    assert torch.equal(torch.sort(m).values, torch.arange(128 ** 3, device="cuda"))


@pytest.mark.parametrize("n_bytes", [1, 3, 4, 1021, 128 ** 3 * 2 // 8])
def test_packbits_bit_exact(rm, n_bytes):
    g = torch.Generator().manual_seed(n_bytes)
    grid = torch.rand(1, n_bytes * 8, generator=g)
    grid[0, :8] = torch.tensor([0.5, 0.49999, 0.50001, -1.0, float("nan"), float("inf"), 0.0, 1.0])[: min(8, n_bytes * 8)]
    ref = oracle.packbits(grid.numpy(), 0.5)
    got = to_np(rm.packbits(grid.cuda(), 0.5))
    assert np.array_equal(got, ref)


def _march_case(bound, N, dt_gamma, perturb, seed, max_steps=1024):
    s = scene(bound, N, seed=seed)
    n_ref, f_ref = oracle.near_far_from_aabb(s["rays_o"].numpy(), s["rays_d"].numpy(), s["aabb"].numpy(), 0.2)
    g = torch.Generator().manual_seed(seed + 7)
    noises = torch.rand(N, generator=g) if perturb else torch.zeros(N)
    return s, n_ref, f_ref, noises


@pytest.mark.parametrize("bound,dt_gamma,perturb,repeat", [(1, 0.0, False, 1), (2, 1 / 128, False, 1), (2, 1 / 128, True, 1), (4, 1 / 64, True, 1),
                                                           (2, 1 / 128, True, 9),
                                                           # dt_gamma that is no power of two (t + t * dt_gamma rounds twice: the recurrence's
                                                           # mul + add form), and large ones whose rays cross all three step regimes in a round or two
                                                           (2, 0.013, True, 1), (4, 0.05, False, 1), (1, 0.3, True, 1), (4, 0.25, True, 1)])
def test_march_rays_train_bit_exact(rm, bound, dt_gamma, perturb, repeat):
    """`repeat` > 1: more than 16384 rays, which the library marches with one ray per lane instead of one per wave."""
    from focnerf_amd.backend import _raymarching as be
    N, max_steps = 2048, 1024
    s, n_ref, f_ref, noises = _march_case(bound, N, dt_gamma, perturb, seed=3)
    if repeat > 1:
        s["rays_o"], s["rays_d"] = s["rays_o"].repeat(repeat, 1), s["rays_d"].repeat(repeat, 1)
        n_ref, f_ref = np.tile(n_ref, repeat), np.tile(f_ref, repeat)
        N *= repeat
        noises = torch.rand(N, generator=torch.Generator().manual_seed(21))
    C, H = s["cascade"], 128
    # sizing pass on the oracle, then a tight M and a too-small M (dropped rays)
    _, _, _, rays0, cnt0 = oracle.march_rays_train(s["rays_o"].numpy(), s["rays_d"].numpy(), s["bits"].numpy(), s["bound"], dt_gamma, max_steps,
                                                   C, H, N * max_steps // 8, n_ref, f_ref, noises.numpy())
    total = int(cnt0[0])
    assert total > 10 * N // 10, "scene should produce samples"
    for M in [total + 128, max(total // 2, 1)]:
        xr, dr, lr, rr, cr = oracle.march_rays_train(s["rays_o"].numpy(), s["rays_d"].numpy(), s["bits"].numpy(), s["bound"], dt_gamma, max_steps,
                                                     C, H, M, n_ref, f_ref, noises.numpy())
        dev = "cuda"
        xyzs = torch.zeros(M, 3, device=dev); dirs = torch.zeros(M, 3, device=dev); deltas = torch.zeros(M, 2, device=dev)
        rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
        counter = torch.zeros(2, dtype=torch.int32, device=dev)
        be.march_rays_train(s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda(), s["bound"], dt_gamma, max_steps, N, C, H, M,
                            torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda(), xyzs, dirs, deltas, rays, counter, noises.cuda())
        assert np.array_equal(to_np(counter), cr)
        assert np.array_equal(to_np(rays), rr), "per-ray (id, offset, count) must be bit-exact"
        for got, ref, nm in [(xyzs, xr, "xyzs"), (dirs, dr, "dirs"), (deltas, lr, "deltas")]:
            assert np.array_equal(to_np(got).view(np.uint32), ref.view(np.uint32)), f"{nm} differ (M={M})"
        # size-independent structure: offsets are the exclusive prefix sum of the counts (ray order)
        r = to_np(rays)
        assert np.array_equal(r[:, 0], np.arange(N)) and np.array_equal(r[:, 1], np.concatenate([[0], np.cumsum(r[:-1, 2])]))


@pytest.mark.parametrize("bound,dt_gamma,max_steps,fill", [(1, 0.0, 1024, 0.5), (2, 1 / 128, 100, 0.5), (2, 1 / 256, 64, 0.9), (4, 1 / 32, 333, 0.1),
                                                            (1, 0.0, 7, 1.0)])
def test_march_rays_train_random_occupancy_bit_exact(rm, bound, dt_gamma, max_steps, fill):
    """The wave-per-ray marcher replays the serial loop's control flow on bit masks: a random occupancy grid (cells flip every step or
    two), the step cap reached inside a block of 64 lattice points, axis-parallel rays (1/d = inf) and rays that miss the box."""
    from focnerf_amd.backend import _raymarching as be
    N = 1024
    s, n_ref, f_ref, noises = _march_case(bound, N, dt_gamma, True, seed=11)
    C, H = s["cascade"], 128
    g = torch.Generator().manual_seed(5)
    bits = (torch.rand(C * H ** 3 // 8, 8, generator=g) < fill).to(torch.uint8)
    bits = (bits << torch.arange(8, dtype=torch.uint8)).sum(dim=1).to(torch.uint8)
    rays_o, rays_d = s["rays_o"].clone(), s["rays_d"].clone()
    rays_d[:8] = torch.tensor([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.6, -0.8]]).repeat(2, 1)   # zero components
    rays_o[:8] = torch.tensor([[0.1, -0.2, 0.9 * bound], [0.3, -0.9 * bound, 0.1], [0.9 * bound, 0.2, -0.1], [0.0, -0.5 * bound, 0.6 * bound]]).repeat(2, 1)
    rays_o[8:12] += 10 * bound                                                                                       # miss the box
    n_ref, f_ref = oracle.near_far_from_aabb(rays_o.numpy(), rays_d.numpy(), s["aabb"].numpy(), 0.2)
    M = N * max_steps
    xr, dr, lr, rr, cr = oracle.march_rays_train(rays_o.numpy(), rays_d.numpy(), bits.numpy(), s["bound"], dt_gamma, max_steps, C, H, M, n_ref, f_ref,
                                                 noises.numpy())
    assert rr[:, 2].max() == max_steps or fill < 0.9, "some ray should run into the step cap"
    dev = "cuda"
    xyzs = torch.zeros(M, 3, device=dev); dirs = torch.zeros(M, 3, device=dev); deltas = torch.zeros(M, 2, device=dev)
    rays = torch.empty(N, 3, dtype=torch.int32, device=dev)
    counter = torch.zeros(2, dtype=torch.int32, device=dev)
    be.march_rays_train(rays_o.cuda(), rays_d.cuda(), bits.cuda(), s["bound"], dt_gamma, max_steps, N, C, H, M, torch.from_numpy(n_ref).cuda(),
                        torch.from_numpy(f_ref).cuda(), xyzs, dirs, deltas, rays, counter, noises.cuda())
    assert np.array_equal(to_np(counter), cr)
    assert np.array_equal(to_np(rays), rr)
    for got, ref, nm in [(xyzs, xr, "xyzs"), (dirs, dr, "dirs"), (deltas, lr, "deltas")]:
        assert np.array_equal(to_np(got).view(np.uint32), ref.view(np.uint32)), f"{nm} differ"


@pytest.mark.parametrize("N", [1, 3, 4, 5, 255, 1025, 4095, 16384, 16385])
def test_slot_reservation_in_the_emit_pass_equals_the_one_workgroup_scan(rm, N):
    """Round 5: batches of the wave form (<= 16 384 rays) reserve their sample slots inside the emit pass (every workgroup adds up the counts of the
    rays before its own) instead of k_march_scan. Ray counts that 4 does not divide, a single ray, both sides of the switch, a counter that does NOT
    start at zero (its entry values reach the emit pass through a snapshot the count pass takes) — against the oracle and against the forced
    one-ray-per-lane form, which keeps the scan kernel: `rays`, `counter` and every sample bit for bit."""
    from focnerf_amd import _lib
    from focnerf_amd.backend import _raymarching as be
    max_steps, dt_gamma = 256, 1 / 128
    s, n_ref, f_ref, _ = _march_case(2, 2048, dt_gamma, True, seed=7)
    rep = (N + 2047) // 2048
    ro, rd = s["rays_o"].repeat(rep, 1)[:N].contiguous(), s["rays_d"].repeat(rep, 1)[:N].contiguous()
    nr, fr = np.tile(n_ref, rep)[:N].copy(), np.tile(f_ref, rep)[:N].copy()
    noises = torch.rand(N, generator=torch.Generator().manual_seed(N))
    C, H = s["cascade"], 128
    M = N * 64 + 128
    xr, dr, lr, rr, cr = oracle.march_rays_train(ro.numpy(), rd.numpy(), s["bits"].numpy(), s["bound"], dt_gamma, max_steps, C, H, M, nr, fr, noises.numpy())
    assert int(cr[0]) > 0 or N < 8

    def run(base):
        xyzs = torch.zeros(M + base, 3, device="cuda"); dirs = torch.zeros(M + base, 3, device="cuda"); deltas = torch.zeros(M + base, 2, device="cuda")
        rays = torch.full((N, 3), -7, dtype=torch.int32, device="cuda")
        counter = torch.tensor([base, 0], dtype=torch.int32, device="cuda")
        be.march_rays_train(ro.cuda(), rd.cuda(), s["bits"].cuda(), s["bound"], dt_gamma, max_steps, N, C, H, M + base, torch.from_numpy(nr).cuda(),
                            torch.from_numpy(fr).cuda(), xyzs, dirs, deltas, rays, counter, noises.cuda())
        return to_np(xyzs), to_np(dirs), to_np(deltas), to_np(rays), to_np(counter)
    for base in (0, 37):
        got = run(base)
        with _lib.option("FOC_MARCH_SERIAL", 1):               # one ray per lane + k_march_scan
            ser = run(base)
        for a, b, nm in zip(got, ser, ("xyzs", "dirs", "deltas", "rays", "counter")):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{nm}: emit-pass reservation differs from the scan kernel (N={N}, base={base})"
        x, d, l, r, c = got
        assert np.array_equal(c, [cr[0] + base, N])
        assert np.array_equal(r[:, 0], rr[:, 0]) and np.array_equal(r[:, 2], rr[:, 2]) and np.array_equal(r[:, 1], rr[:, 1] + base)
        total = int(cr[0])
        assert np.array_equal(x[base:base + total].view(np.uint32), xr[:total].view(np.uint32))
        assert np.array_equal(l[base:base + total].view(np.uint32), lr[:total].view(np.uint32))
        assert not x[:base].any() and not x[base + total:].any()                       # nothing written outside the reserved range


def test_march_rays_train_wrapper_semantics(rm):
    """mean_count / align / force_all_rays sizing rules of raymarching.py:196-229."""
    N = 1024
    s, n_ref, f_ref, _ = _march_case(2, N, 1 / 128, False, seed=5)
    o, d, bits = s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = rm.near_far_from_aabb(o, d, s["aabb"].cuda(), 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    xyzs, dirs, deltas, rays = rm.march_rays_train(o, d, s["bound"], bits, s["cascade"], 128, nears, fars, counter, -1, False, 128, False, 1 / 128, 1024)
    m = int(counter[0].item())
    assert xyzs.shape[0] == m + 128 - m % 128 and int(counter[1].item()) == N
    assert torch.all(xyzs[m:] == 0)
    # estimated mean_count: M = mean_count rounded up by align (a full extra `align` when already aligned)
    counter.zero_()
    x2, _, _, rays2 = rm.march_rays_train(o, d, s["bound"], bits, s["cascade"], 128, nears, fars, counter, 256, False, 128, False, 1 / 128, 1024)
    assert x2.shape[0] == 384
    # idempotent / deterministic
    counter.zero_()
    x3, _, _, rays3 = rm.march_rays_train(o, d, s["bound"], bits, s["cascade"], 128, nears, fars, counter, -1, False, 128, False, 1 / 128, 1024)
    assert torch.equal(x3, xyzs) and torch.equal(rays3, rays)


def _random_segments(N, seed, max_len=300):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_len, N)
    counts[::7] = 0                      # empty rays
    counts[1] = 1
    counts[2] = 64; counts[3] = 65; counts[4] = 128; counts[5] = 1000
    offsets = np.concatenate([[0], np.cumsum(counts[:-1])])
    M = int(counts.sum())
    order = rng.permutation(N)           # rays rows in arbitrary order, ids are a permutation
    rays = np.stack([order, offsets, counts], -1).astype(np.int32)
    sig = (rng.random(M) ** 3 * 60).astype(np.float32)
    sig[rng.random(M) < 0.3] = 0
    rgb = rng.random((M, 3)).astype(np.float32)
    deltas = np.stack([rng.random(M) * 0.02 + 0.003, rng.random(M) * 0.05 + 0.003], -1).astype(np.float32)
    return rays, sig, rgb, deltas, M


@pytest.mark.parametrize("T_thresh", [1e-4, 0.0, 1e-2])
def test_composite_rays_train_forward_backward(rm, T_thresh):
    from focnerf_amd.backend import _raymarching as be
    N = 1500
    rays, sig, rgb, deltas, M = _random_segments(N, 11)
    rays[10, 1] = M - 3; rays[10, 2] = 50       # segment overflowing M: treated as dropped (zeros)
    ws_r, dp_r, im_r = oracle.composite_rays_train_forward(sig, rgb, deltas, rays, N, T_thresh)
    t = lambda a: torch.from_numpy(a).cuda()
    ws = torch.empty(N, device="cuda"); dp = torch.empty(N, device="cuda"); im = torch.empty(N, 3, device="cuda")
    be.composite_rays_train_forward(t(sig), t(rgb), t(deltas), t(rays), M, N, T_thresh, ws, dp, im)
    np.testing.assert_allclose(to_np(ws), ws_r, atol=RGB_TOL, rtol=0)
    np.testing.assert_allclose(to_np(im), im_r, atol=RGB_TOL, rtol=0)
    np.testing.assert_allclose(to_np(dp), dp_r, atol=3e-4, rtol=1e-4)      # depth sums w * t with t up to ~50
    assert to_np(ws)[rays[10, 0]] == 0 and np.all(to_np(im)[rays[10, 0]] == 0)
    # backward
    rng = np.random.default_rng(5)
    gws = rng.standard_normal(N).astype(np.float32)
    gim = rng.standard_normal((N, 3)).astype(np.float32)
    gs_r, gc_r = oracle.composite_rays_train_backward(gws, gim, sig, rgb, deltas, rays, ws_r, im_r, T_thresh)
    gs = torch.zeros(M, device="cuda"); gc = torch.zeros(M, 3, device="cuda")
    be.composite_rays_train_backward(t(gws), t(gim), t(sig), t(rgb), t(deltas), t(rays), ws, im, M, N, T_thresh, gs, gc)
    np.testing.assert_allclose(to_np(gc), gc_r, atol=RGB_TOL * 4, rtol=1e-4)
    np.testing.assert_allclose(to_np(gs), gs_r, atol=2e-4, rtol=2e-3)


def test_composite_autograd_matches_torch_reference(rm):
    """The autograd Function against a plain torch fp32 implementation of the same recurrence."""
    N = 200
    rays, sig, rgb, deltas, M = _random_segments(N, 21, max_len=80)
    sig_t = torch.from_numpy(sig).cuda().requires_grad_(True)
    rgb_t = torch.from_numpy(rgb).cuda().requires_grad_(True)
    ws, dp, im = rm.composite_rays_train(sig_t, rgb_t, torch.from_numpy(deltas).cuda(), torch.from_numpy(rays).cuda(), 0.0)
    gw = torch.randn(N, device="cuda"); gi = torch.randn(N, 3, device="cuda")
    (ws * gw).sum().add((im * gi).sum()).backward()
    s2 = torch.from_numpy(sig).double().requires_grad_(True)
    c2 = torch.from_numpy(rgb).double().requires_grad_(True)
    loss = 0
    for n in range(N):
        idx, off, cnt = rays[n]
        if cnt == 0:
            continue
        a = 1 - torch.exp(-s2[off:off + cnt] * torch.from_numpy(deltas[off:off + cnt, 0]).double())
        T = torch.cumprod(torch.cat([torch.ones(1, dtype=torch.double), 1 - a]), 0)[:-1]
        w = a * T
        loss = loss + w.sum() * gw[idx].item() + ((w[:, None] * c2[off:off + cnt]).sum(0) * gi[idx].double().cpu()).sum()
    loss.backward()
    np.testing.assert_allclose(to_np(sig_t.grad), s2.grad.numpy(), atol=2e-4, rtol=2e-3)
    np.testing.assert_allclose(to_np(rgb_t.grad), c2.grad.numpy(), atol=2e-4, rtol=1e-3)


@pytest.mark.parametrize("use", ["image", "weights_sum", "depth"])
def test_composite_autograd_with_unused_outputs(rm, use):
    """A loss that reads one output only: the others' gradients reach the node as None (no zero tensors are materialised) and the result
    equals the one obtained with explicit zero gradients; depth has no derivative (raymarching.py:275)."""
    N = 100
    rays, sig, rgb, deltas, M = _random_segments(N, 5, max_len=70)
    args = (torch.from_numpy(deltas).cuda(), torch.from_numpy(rays).cuda(), 1e-4)
    grads = {}
    for explicit in (False, True):
        sig_t = torch.from_numpy(sig).cuda().requires_grad_(True)
        rgb_t = torch.from_numpy(rgb).cuda().requires_grad_(True)
        ws, dp, im = rm.composite_rays_train(sig_t, rgb_t, *args)
        picked = {"image": im.sum(), "weights_sum": ws.sum(), "depth": dp.sum()}[use]
        loss = picked + (0.0 * ws.sum() + 0.0 * im.sum() if explicit else 0.0)
        loss.backward()
        grads[explicit] = (to_np(sig_t.grad), to_np(rgb_t.grad))
    assert np.array_equal(grads[False][0], grads[True][0]) and np.array_equal(grads[False][1], grads[True][1])
    if use == "depth":
        assert not grads[False][0].any() and not grads[False][1].any()
    else:
        assert grads[False][0].any()


def _analytic_field(x, d):
    sig = 30 * np.exp(-(x ** 2).sum(-1) / 0.3).astype(np.float32)
    rgb = (0.5 + 0.5 * np.sin(3 * x + d)).astype(np.float32)
    return sig, rgb


def _set_march_form(lib_option, form):
    """R9's two forms behind foc_march_rays: 16 lanes per ray (k_march_rays_row) and the plain one-lookup-at-a-time loop (k_march_rays)."""
    lib_option("FOC_MARCH_RAYS_ROW_MAX", 1000000000 if form == "row" else 0)


@pytest.mark.parametrize("form", ["row", "serial"])
@pytest.mark.parametrize("perturb", [False, True])
def test_inference_loop_final_image_without_resync(rm, form, perturb, lib_option):
    """The whole inference loop of legacy/nerf/renderer.py:323-372 run TWICE, independently: on the oracle and on the GPU, each on its own
    state from the first iteration to the last (device-side compaction, no per-iteration re-synchronisation) — an error that builds up in
    composite_rays or march_rays over the iterations would show in the final image. Tolerated: the counted rays whose transmittance crosses
    T_thresh one sample earlier or later (__expf vs expf at the boundary), each of which moves a pixel by <= ~T_thresh. All forms of R9."""
    _set_march_form(lib_option, form)
    N = 4000                                           # scene() draws from a 64 x 64 view: at most 4096 rays
    s, n_ref, f_ref, noises = _march_case(2, N, 1 / 128, perturb, seed=13)
    assert s["rays_o"].shape[0] == N
    C, H, max_steps, T_thresh = s["cascade"], 128, 1024, 1e-4
    o_np, d_np, bits_np = s["rays_o"].numpy(), s["rays_d"].numpy(), s["bits"].numpy()
    # ---- oracle loop, its own state
    ws = np.zeros(N, np.float32); dp = np.zeros(N, np.float32); im = np.zeros((N, 3), np.float32)
    alive = np.arange(N, dtype=np.int32); rt = n_ref.copy()
    step, its = 0, 0
    killed_at = np.full(N, -1)
    while step < max_steps and alive.shape[0] > 0:
        n_alive = alive.shape[0]
        n_step = max(min(N // n_alive, 8), 1)
        M = n_alive * n_step
        M += 128 - M % 128
        nz = noises.numpy()[:n_alive] if (perturb and step == 0) else np.zeros(n_alive, np.float32)
        x, dd, dl = oracle.march_rays(n_alive, n_step, alive, rt, o_np, d_np, s["bound"], 1 / 128, max_steps, C, H, bits_np, n_ref, f_ref, nz, M=M)
        sig, rgb = _analytic_field(x, dd)
        before = alive.copy()
        alive, rt, ws, dp, im = oracle.composite_rays(n_alive, n_step, T_thresh, alive, rt, sig, rgb, dl, ws, dp, im)
        killed_at[before[alive < 0]] = its
        alive = alive[alive >= 0]
        step += n_step
        its += 1
    # ---- GPU loop, its own state
    dev = "cuda"
    o, d, bits = s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda()
    gws = torch.zeros(N, device=dev); gdp = torch.zeros(N, device=dev); gim = torch.zeros(N, 3, device=dev)
    galive = torch.arange(N, dtype=torch.int32, device=dev); grt = nears.clone()
    gstep, gits = 0, 0
    while gstep < max_steps and galive.shape[0] > 0:
        n_alive = galive.shape[0]
        n_step = max(min(N // n_alive, 8), 1)
        # the wrapper draws torch.rand when perturb is set; the oracle's noise is handed over through the backend instead
        M = n_alive * n_step
        M += 128 - M % 128
        gx = torch.zeros(M, 3, device=dev); gd = torch.zeros(M, 3, device=dev); gl = torch.zeros(M, 2, device=dev)
        nz = noises[:n_alive].cuda() if (perturb and gstep == 0) else torch.zeros(n_alive, device=dev)
        from focnerf_amd.backend import _raymarching
        _raymarching.march_rays(n_alive, n_step, galive, grt, o, d, s["bound"], 1 / 128, max_steps, C, H, bits, nears, fars, gx, gd, gl, nz)
        sig, rgb = _analytic_field(to_np(gx), to_np(gd))
        rm.composite_rays(n_alive, n_step, galive, grt, torch.from_numpy(sig).cuda(), torch.from_numpy(rgb).cuda(), gl, gws, gdp, gim, T_thresh)
        comp, n_out = rm.compact_alive(galive)
        galive = comp[: int(n_out.item())].contiguous()
        gstep += n_step
        gits += 1
    assert its > 3 and ws.max() > 0.9 and abs(gits - its) <= 1
    d_ws, d_im = np.abs(to_np(gws) - ws), np.abs(to_np(gim) - im).max(-1)
    # every pixel within the threshold's reach; all but the counted flips within the kernel tolerance
    assert d_ws.max() <= 4 * T_thresh and d_im.max() <= 4 * T_thresh, (d_ws.max(), d_im.max())
    flips = (d_ws > RGB_TOL) | (d_im > RGB_TOL)
    assert flips.mean() < 2e-3, f"{flips.sum()} of {N} rays differ by more than {RGB_TOL}"
    np.testing.assert_allclose(to_np(gdp)[~flips], dp[~flips], atol=2e-4, rtol=1e-5)


@pytest.mark.parametrize("form", ["row", "serial"])
def test_inference_march_and_composite_loop(rm, form, lib_option):
    """legacy/nerf/renderer.py:323-372 loop, oracle vs GPU, with an analytic field standing in for the network. Per iteration: sample
    positions / directions / deltas bit for bit (all forms of R9), composite state within RGB_TOL; the
    state is re-synchronised to the oracle's after each iteration so that every iteration's inputs are identical (the un-synchronised
    end-to-end comparison is test_inference_loop_final_image_without_resync)."""
    _set_march_form(lib_option, form)
    N = 3000
    s, n_ref, f_ref, _ = _march_case(2, N, 1 / 128, False, seed=9)
    C, H, max_steps, T_thresh = s["cascade"], 128, 1024, 1e-4
    o_np, d_np, bits_np = s["rays_o"].numpy(), s["rays_d"].numpy(), s["bits"].numpy()

    field_np = _analytic_field

    # oracle loop
    ws = np.zeros(N, np.float32); dp = np.zeros(N, np.float32); im = np.zeros((N, 3), np.float32)
    alive = np.arange(N, dtype=np.int32); rt = n_ref.copy()
    # GPU loop state
    dev = "cuda"
    o, d, bits = s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda()
    gws = torch.zeros(N, device=dev); gdp = torch.zeros(N, device=dev); gim = torch.zeros(N, 3, device=dev)
    galive = torch.arange(N, dtype=torch.int32, device=dev); grt = nears.clone()
    step = 0
    it = 0
    while step < max_steps:
        n_alive = alive.shape[0]
        assert galive.shape[0] == n_alive
        if n_alive <= 0:
            break
        n_step = max(min(N // n_alive, 8), 1)
        M = n_alive * n_step
        M += 128 - M % 128
        x, dd, dl = oracle.march_rays(n_alive, n_step, alive, rt, o_np, d_np, s["bound"], 1 / 128, max_steps, C, H, bits_np, n_ref, f_ref,
                                      np.zeros(n_alive, np.float32), M=M)
        gx, gd, gl = rm.march_rays(n_alive, n_step, galive, grt, o, d, s["bound"], bits, C, H, nears, fars, 128, False, 1 / 128, max_steps)
        assert np.array_equal(to_np(gx).view(np.uint32), x.view(np.uint32)), f"march_rays xyzs differ at iteration {it}"
        assert np.array_equal(to_np(gl).view(np.uint32), dl.view(np.uint32))
        assert np.array_equal(to_np(gd).view(np.uint32), dd.view(np.uint32))
        sig, rgb = field_np(x, dd)
        alive, rt, ws, dp, im = oracle.composite_rays(n_alive, n_step, T_thresh, alive, rt, sig, rgb, dl, ws, dp, im)
        rm.composite_rays(n_alive, n_step, galive, grt, torch.from_numpy(sig).cuda(), torch.from_numpy(rgb).cuda(), gl, gws, gdp, gim, T_thresh)
        # __expf vs expf can move T across the threshold for a ray exactly at the boundary; the kill decision
        # is compared on the oracle's state and the GPU state is re-synchronised to keep the loop comparable
        ga = to_np(galive)
        mism = (ga >= 0) != (alive >= 0)
        assert mism.mean() < 2e-3, "ray termination decisions diverge"
        np.testing.assert_allclose(to_np(gws), ws, atol=RGB_TOL)
        np.testing.assert_allclose(to_np(gim), im, atol=RGB_TOL)
        galive = torch.from_numpy(alive).cuda(); grt = torch.from_numpy(rt).cuda()
        gws = torch.from_numpy(ws).cuda(); gdp = torch.from_numpy(dp).cuda(); gim = torch.from_numpy(im).cuda()
        # device-side ordered compaction == boolean mask
        comp, n_out = rm.compact_alive(galive)
        alive = alive[alive >= 0]
        assert int(n_out.item()) == alive.shape[0] and np.array_equal(to_np(comp)[: alive.shape[0]], alive)
        galive = comp[: alive.shape[0]].contiguous()
        step += n_step
        it += 1
    assert it > 3 and ws.max() > 0.9


def test_full_view_march_properties(rm):
    """BASELINE size: one 800x800 view (640 000 rays). Checked through size-independent structure."""
    from focnerf_amd import synthetic
    H = W = 800
    bound = 2
    s = scene(bound, 10, seed=0)
    o, d = synthetic.make_view_rays(H, W, bound, 1, seed=4, device="cuda")
    o, d = o[0], d[0]
    N = o.shape[0]
    nears, fars = rm.near_far_from_aabb(o, d, s["aabb"].cuda(), 0.2)
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    M_est = 640000 * 64
    xyzs, dirs, deltas, rays = rm.march_rays_train(o, d, float(bound), s["bits"].cuda(), s["cascade"], 128, nears, fars, counter, M_est, False, 128,
                                                   False, 1 / 128, 1024)
    total = int(counter[0].item())
    assert int(counter[1].item()) == N and 0 < total <= xyzs.shape[0]
    r = rays.long()
    assert torch.equal(r[:, 0], torch.arange(N, device="cuda"))
    assert torch.equal(r[:, 1], torch.cumsum(r[:, 2], 0) - r[:, 2])          # exclusive prefix sum
    assert int(r[:, 2].sum().item()) == total and int(r[:, 2].max().item()) <= 1024
    assert torch.all(xyzs[:total].abs() <= bound) and torch.all(deltas[:total, 0] > 0)
    assert torch.all(xyzs[total:] == 0)
    # every emitted sample sits in an occupied cell of its cascade-0/1 grid region: re-derive occupancy for a subset
    # (tests/march_ref.py's float64 lookup; a sample within rounding of a cell face or of a level's threshold is left out)
    sub = torch.randperm(total, device="cuda")[:20000]
    occ, clear = march_ref.soundness(dict(bound=float(bound), C=s["cascade"], H=128, bits=s["bits"].numpy()), to_np(xyzs[sub]), to_np(deltas[sub, 0]))
    assert clear.mean() > 0.99 and occ[clear].all(), f"{(clear & ~occ).sum()} of 20000 samples lie in clearly empty cells"
    # composite of a constant field over the full view: closed form 1 - exp(-sigma * sum dt) per ray
    sig = torch.full((xyzs.shape[0],), 0.5, device="cuda")
    rgb = torch.full((xyzs.shape[0], 3), 0.25, device="cuda")
    ws, dp, im = rm.composite_rays_train(sig, rgb, deltas, rays, 0.0)
    seg = torch.zeros(N, device="cuda", dtype=torch.float64)
    ids = torch.repeat_interleave(torch.arange(N, device="cuda"), r[:, 2])
    seg.index_add_(0, ids, deltas[:total, 0].double())
    want = 1 - torch.exp(-0.5 * seg)
    assert torch.allclose(ws.double(), want, atol=2e-5)
    assert torch.allclose(im[:, 0].double(), 0.25 * want, atol=2e-5)


@pytest.mark.parametrize("form", ["row", "serial"])
def test_dead_list_entries_are_skipped(rm, form, lib_option):
    """A ray list with -1 entries (what composite_rays leaves behind, and what `compact_alive(pad=True)` puts behind the count): march_rays
    writes nothing for them (their slots stay zero = "terminated"), composite_rays leaves them and every per-ray accumulator alone — the
    live entries get exactly what the compacted list gets. This is what lets the render loop hand on a list whose true length it has not
    read back yet."""
    _set_march_form(lib_option, form)
    N, n_step = 1500, 4
    s, n_ref, f_ref, _ = _march_case(2, N, 1 / 128, False, seed=9)
    C, H = s["cascade"], 128
    o, d, bits = s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda()
    g = torch.Generator().manual_seed(3)
    keep = torch.rand(N, generator=g) > 0.4
    holes = torch.where(keep, torch.arange(N), torch.full((N,), -1)).to(torch.int32).cuda()
    dense = torch.arange(N, dtype=torch.int32)[keep].cuda()
    kept, count = rm.compact_alive(holes, pad=True)
    assert int(count.item()) == dense.shape[0] and torch.equal(kept[: dense.shape[0]], dense) and bool((kept[dense.shape[0]:] == -1).all())
    out = {}
    for name, lst in (("holes", holes), ("padded", kept), ("dense", dense)):
        t_now = nears.clone()
        ws = torch.zeros(N, device="cuda"); dp = torch.zeros(N, device="cuda"); im = torch.zeros(N, 3, device="cuda")
        x, dd, dl = rm.march_rays(lst.shape[0], n_step, lst, t_now, o, d, s["bound"], bits, C, H, nears, fars, 128, False, 1 / 128, 1024)
        sig, rgb = _analytic_field(to_np(x), to_np(dd))
        lst2 = lst.clone()
        rm.composite_rays(lst.shape[0], n_step, lst2, t_now, torch.from_numpy(sig).cuda(), torch.from_numpy(rgb).cuda(), dl, ws, dp, im, 1e-4)
        out[name] = (x, dl, lst2, ws, dp, im, t_now)
    n_live = dense.shape[0]
    for name in ("holes", "padded"):
        x, dl, lst2, ws, dp, im, t_now = out[name]
        sel = (holes >= 0) if name == "holes" else (torch.arange(N, device="cuda") < n_live)
        xs, dls = x[: N * n_step].view(N, n_step, 3), dl[: N * n_step].view(N, n_step, 2)
        assert torch.equal(xs[sel], out["dense"][0][: n_live * n_step].view(n_live, n_step, 3))
        assert torch.equal(dls[sel], out["dense"][1][: n_live * n_step].view(n_live, n_step, 2))
        assert not xs[~sel].any() and not dls[~sel].any(), "dead entries must leave their slots zero"
        assert bool((lst2[~sel] == -1).all())
        for k in (3, 4, 5, 6):
            assert torch.equal(out[name][k], out["dense"][k]), (name, k)
    assert out["dense"][3].max() > 0


@pytest.mark.parametrize("n_step", [1, 4, 8, 16])
@pytest.mark.parametrize("row_max,form", [("1000000000", "two"), ("0", "two"), ("0", "row"), ("0", "lane"), ("0", "staged"), ("0", "")])
def test_two_phase_march_and_composite_compact_equal_the_single_calls(rm, n_step, row_max, form, lib_option):
    """foc_march_rays_two_phase == foc_march_rays bit for bit in each of its forms — the two phases (first visits per lane, walkers compacted
    and marched again, 16 lanes per ray / one ray per lane), the 16-lanes-per-ray kernel that stages a ray's samples in LDS and writes every
    slot itself (buffers handed over full of NaN), one ray per lane, and the form it picks by burst length; its normalised output ==
    (x + bound) * (1 / (2 bound)); foc_composite_compact (register-resident bursts of 4, 8, 16) == composite_rays + compact_alive (list, count,
    every accumulator)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    lib_option("FOC_MARCH_RAYS_ROW_MAX", row_max)
    lib_option("FOC_OCC_MARCH_FORM", form or "")
    N = 3000
    s, n_ref, f_ref, _ = _march_case(2, N, 1 / 128, False, seed=9)
    C, H = s["cascade"], 128
    o, d, bits = s["rays_o"].cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda()
    g = torch.Generator().manual_seed(5)
    lst = torch.where(torch.rand(N, generator=g) > 0.2, torch.arange(N), torch.full((N,), -1)).to(torch.int32).cuda()      # with dead entries
    t_now = nears.clone()
    noises = torch.zeros(N, device="cuda")
    M = N * n_step
    lib_option("FOC_MARCH_RAYS_ROW_MAX", 0)                       # reference call: the plain serial kernel
    x0, d0, l0 = rm.march_rays(N, n_step, lst, t_now, o, d, s["bound"], bits, C, H, nears, fars, -1, False, 1 / 128, 1024)
    lib_option("FOC_MARCH_RAYS_ROW_MAX", row_max)
    st = stream_of(o)
    for normalised in (0, 1):
        fills = bool(lib.foc_march_rays_two_phase_fills(n_step, normalised))
        assert fills == (form in ("row", "staged") or (form == "" and n_step > 2))
        x1, d1, l1 = (torch.full((M, k), float("nan") if fills else 0.0, device="cuda") for k in (3, 3, 2))
        scratch = torch.zeros(N + 4, dtype=torch.int32, device="cuda")
        check(lib.foc_march_rays_two_phase(N, n_step, ptr(lst), ptr(t_now), ptr(o), ptr(d), float(s["bound"]), 1 / 128, 1024, C, H, ptr(bits), ptr(nears), ptr(fars),
                                           ptr(x1), ptr(d1), ptr(l1), ptr(noises), ptr(scratch), normalised, st), "two_phase")
        want = x0 if not normalised else torch.where(l0[:, :1] != 0, (x0 + s["bound"]) * (1.0 / (2.0 * s["bound"])), torch.zeros_like(x0))
        assert torch.equal(x1, want) and torch.equal(d1, d0) and torch.equal(l1, l0)
        if form == "two" or (form == "" and n_step <= 2):
            assert int(scratch[0]) > 0, "some rays must have been walkers"
    # composite + compaction in one call vs the two calls
    sig, rgb = _analytic_field(to_np(x0), to_np(d0))
    sig, rgb = torch.from_numpy(sig).cuda(), torch.from_numpy(rgb).cuda()
    a_list, a_t = lst.clone(), t_now.clone()
    a_ws, a_dp, a_im = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, 3, device="cuda")
    rm.composite_rays(N, n_step, a_list, a_t, sig, rgb, l0, a_ws, a_dp, a_im, 1e-4)
    kept, count = rm.compact_alive(a_list, pad=True)
    b_list, b_t = lst.clone(), t_now.clone()
    b_ws, b_dp, b_im = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, 3, device="cuda")
    out = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    n_out = torch.zeros(1, dtype=torch.int32, device="cuda")
    blocks = torch.zeros(N // 1024 + 2, dtype=torch.int32, device="cuda")
    check(lib.foc_composite_compact(N, n_step, 1e-4, ptr(b_list), ptr(b_t), ptr(sig), ptr(rgb), ptr(l0), ptr(b_ws), ptr(b_dp), ptr(b_im), ptr(out), ptr(n_out),
                                    ptr(blocks), None, 0, 1, 0, st), "composite_compact")
    assert int(n_out) == int(count) and torch.equal(out, kept) and torch.equal(b_list, a_list)
    for a, b in ((a_t, b_t), (a_ws, b_ws), (a_dp, b_dp), (a_im, b_im)):
        assert torch.equal(a, b)
    # sample-major arrays ([n_step][N] instead of [N][n_step]): the staged kernel writes them (flag bit 2), foc_composite_compact reads them
    if lib.foc_march_rays_two_phase_sample_major(N, n_step, 4):
        xs, ds_, ls = (torch.full((M, k), float("nan"), device="cuda") for k in (3, 3, 2))
        scratch = torch.zeros(N + 4, dtype=torch.int32, device="cuda")
        check(lib.foc_march_rays_two_phase(N, n_step, ptr(lst), ptr(t_now), ptr(o), ptr(d), float(s["bound"]), 1 / 128, 1024, C, H, ptr(bits), ptr(nears), ptr(fars),
                                           ptr(xs), ptr(ds_), ptr(ls), ptr(noises), ptr(scratch), 4, st), "two_phase (sample-major)")
        for got, want in ((xs, x0), (ds_, d0), (ls, l0)):
            assert torch.equal(got.view(n_step, N, -1).transpose(0, 1), want[:M].view(N, n_step, -1))
        sig_sm = sig[:M].view(N, n_step).t().contiguous()
        rgb_sm = rgb[:M].view(N, n_step, 3).transpose(0, 1).contiguous()
        c_list, c_t = lst.clone(), t_now.clone()
        c_ws, c_dp, c_im = torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, 3, device="cuda")
        out.fill_(-1); n_out.zero_(); blocks.zero_()
        deaths = torch.zeros(n_step + 1, 64, dtype=torch.int32, device="cuda")
        check(lib.foc_composite_compact(N, n_step, 1e-4, ptr(c_list), ptr(c_t), ptr(sig_sm), ptr(rgb_sm), ptr(ls), ptr(c_ws), ptr(c_dp), ptr(c_im), ptr(out), ptr(n_out),
                                        ptr(blocks), ptr(deaths), 0, n_step + 1, 1, st), "composite_compact (sample-major)")
        assert int(n_out) == int(count) and torch.equal(out, kept) and torch.equal(c_list, a_list)
        for a, b in ((a_t, c_t), (a_ws, c_ws), (a_dp, c_dp), (a_im, c_im)):
            assert torch.equal(a, b)
        # the death histogram: every listed ray that did not survive, at the slot where it ended
        assert int(deaths.sum()) == int((lst >= 0).sum()) - int(count)


@pytest.mark.parametrize("form", ["staged", "lane", ""])
@pytest.mark.parametrize("max_steps", [37, 1024])
def test_rederived_burst_equals_single_sample_calls(rm, form, max_steps, lib_option):
    """foc_march_rays_two_phase with flag bit 1: a burst of k samples == k calls of the reference kernel with n_step = 1, each continued from
    rays_t + deltas[:,1] the way composite_rays hands t to the next call (raymarching.cu:871, 899) — bit for bit, also where a skip over
    empty space more than doubles t and t - last_t is rounded (max_steps 37: steps of dt_max; rays starting inside the box at t = 0.2)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    lib_option("FOC_OCC_MARCH_FORM", form or "")
    N, k = 4000, 8
    s, n_ref, f_ref, _ = _march_case(2, N, 1 / 128, False, seed=11, max_steps=max_steps)
    C, H = s["cascade"], 128
    # half of the rays start INSIDE the box (near = min_near = 0.2): the first occupied cell is then several times t away
    o = s["rays_o"].clone()
    o[::2] *= 0.15
    o = o.contiguous()
    n_ref, f_ref = oracle.near_far_from_aabb(o.numpy(), s["rays_d"].numpy(), s["aabb"].numpy(), 0.2)
    o, d, bits = o.cuda(), s["rays_d"].cuda(), s["bits"].cuda()
    nears, fars = torch.from_numpy(n_ref).cuda(), torch.from_numpy(f_ref).cuda()
    lst = torch.arange(N, dtype=torch.int32, device="cuda")
    # reference: k single-sample calls, t handed on as composite_rays does (fp32 add of deltas[:,1]); a ray that returned no sample is finished
    lib_option("FOC_MARCH_RAYS_ROW_MAX", 0)
    t_now = nears.clone()
    alive = torch.ones(N, dtype=torch.bool, device="cuda")
    want_x, want_l = torch.zeros(N, k, 3, device="cuda"), torch.zeros(N, k, 2, device="cuda")
    for j in range(k):
        x, _, dl = rm.march_rays(N, 1, lst, t_now, o, d, s["bound"], bits, C, H, nears, fars, -1, False, 1 / 128, max_steps)
        got = (dl[:N, 0] > 0) & alive
        want_x[:, j][got] = x[:N][got]
        want_l[:, j][got] = dl[:N][got]
        t_now = torch.where(got, t_now + dl[:N, 1], t_now)
        alive = got
    assert alive.float().mean() > 0.3, "most rays should still be marching after k samples"
    st = stream_of(o)
    noises = torch.zeros(N, device="cuda")
    outs = {}
    for flags in (2, 0):
        x1, d1, l1 = (torch.zeros(N * k, c, device="cuda") for c in (3, 3, 2))
        scratch = torch.zeros(N + 4, dtype=torch.int32, device="cuda")
        check(lib.foc_march_rays_two_phase(N, k, ptr(lst), ptr(nears), ptr(o), ptr(d), float(s["bound"]), 1 / 128, max_steps, C, H, ptr(bits), ptr(nears), ptr(fars),
                                           ptr(x1), ptr(d1), ptr(l1), ptr(noises), ptr(scratch), flags, st), "two_phase")
        outs[flags] = (x1.view(N, k, 3), l1.view(N, k, 2))
    assert torch.equal(outs[2][0], want_x) and torch.equal(outs[2][1], want_l)
    # without the bit the burst keeps the march's own t: last_t + fl(t - last_t) rounds back to t except in tie cases, so on ordinary scenes the
    # two forms agree (they do here) — the bit turns "practically always" into "always"
    same = torch.equal(outs[0][1], want_l)
    print("burst without re-derivation equals the single-sample calls:", same)


@pytest.mark.parametrize("n_step", [1, 3, 4, 8, 16])
def test_composite_rays_every_burst_length(rm, n_step):
    """R10 on synthetic bursts: the register-resident kernels (bursts of 4, 8, 16 on 16-byte aligned arrays) and the pointer-walking one (any
    other burst, or unaligned arrays) give the same bits, and both are the oracle's result up to __expf against expf (1e-5; a ray whose
    transmittance sits on the threshold may end one sample apart) — rays that end on an empty slot, rays that end on the transmittance test
    (opaque samples), rays that survive, accumulators that start non-zero."""
    g = torch.Generator().manual_seed(100 + n_step)
    N = 3001
    M = N * n_step
    sig = (torch.rand(M, generator=g) * 3.0)
    sig[torch.rand(M, generator=g) < 0.02] = 400.0                                  # opaque: the transmittance test fires
    rgb = torch.rand(M, 3, generator=g)
    dl = torch.rand(M, 2, generator=g) * 0.05 + 0.005
    filled = torch.randint(0, n_step + 1, (N,), generator=g)
    filled[torch.rand(N, generator=g) < 0.5] = n_step                                # half of the rays fill their burst
    dl.view(N, n_step, 2)[torch.arange(n_step)[None, :] >= filled[:, None]] = 0.0
    alive = torch.randperm(N, generator=g).to(torch.int32)            # (no dead entries: the reference kernel, and so the oracle, does not expect any)
    rt = torch.rand(N, generator=g) + 0.2
    ws0, dp0, im0 = torch.rand(N, generator=g) * 0.3, torch.rand(N, generator=g), torch.rand(N, 3, generator=g) * 0.3
    want = oracle.composite_rays(N, n_step, 1e-4, alive.numpy(), rt.numpy(), sig.numpy(), rgb.numpy(), dl.numpy(), ws0.numpy(), dp0.numpy(), im0.numpy())

    def dev(t, pad):                       # pad = 1: the array starts 4 bytes into a 16-byte aligned allocation (the pointer-walking kernel)
        buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
        view = buf[pad: pad + t.numel()].view(t.shape)
        view.copy_(t)
        return view
    got = {}
    for pad in (0, 1):
        ga, gt = alive.cuda(), rt.cuda()
        gws, gdp, gim = ws0.cuda(), dp0.cuda(), im0.cuda()
        rm.composite_rays(N, n_step, ga, gt, dev(sig, pad), dev(rgb, pad), dev(dl, 2 * pad), gws, gdp, gim, 1e-4)
        got[pad] = (ga, gt, gws, gdp, gim)
    for a, b in zip(got[0], got[1]):
        assert torch.equal(a, b)
    ga, gt, gws, gdp, gim = got[0]
    same = (to_np(ga) >= 0) == (want[0] >= 0)
    assert same.mean() > 1 - 2e-3, "ray termination decisions diverge"
    for g_, w_, name in ((gt, want[1], "rays_t"), (gws, want[2], "weights_sum"), (gdp, want[3], "depth"), (gim, want[4], "image")):
        np.testing.assert_allclose(to_np(g_)[same], w_[same], atol=1e-5, rtol=1e-5, err_msg=name)
    assert (want[0] >= 0).sum() > 0 and (want[0] < 0).sum() > N // 10
