"""CPU: pin the float64 reference of the fixed-step tail (tests/fixed_tail_ref.py) that the GPU tail tests measure the kernels against —
against the reference's own run() (the run_foc*.npz fixtures), against the C oracle's composite, against autograd's numerical
gradient, and its error bound against an fp32 evaluation of the same expressions."""
import os

import numpy as np
import pytest
import torch

import oracle
from fixed_tail_ref import U, clear_of_half_midpoints, magnitudes, tail, tail_backward

# the bound c * 2^-24 * (T + k) * mag (fixed_tail_ref.py): c = 2 ulps for exp, every other operation correctly rounded (1/2 ulp, inside
# the |result| each rounding adds to mag); k = 16 leaves room for the second-order terms the first-order magnitudes drop.
C, K = 2.0, 16


def ratio(got, want, mag, T, extra=0.0):
    """Worst |got - want| / (2^-24 (T + K) mag) over the elements where want is finite (got must be finite exactly there)."""
    got, want, mag = (np.asarray(a, np.float64) for a in (got, want, mag))
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "non-finite values at other places"
    err = np.maximum(np.abs(got - want)[fin] - extra, 0.0)
    scale = U * (T + K) * mag[fin]
    if err.size == 0:
        return 0.0
    assert not (err[scale == 0] > 0).any(), "an exact value differs"
    return float((err[scale > 0] / scale[scale > 0]).max(initial=0.0))


def linspace_z(near, far, T, noise=None):
    """run()'s z_vals and deltas in fp32 as torch's CPU kernels form them."""
    near, far = torch.as_tensor(near, dtype=torch.float32), torch.as_tensor(far, dtype=torch.float32)
    z = near[:, None] + (far - near)[:, None] * torch.linspace(0.0, 1.0, T).unsqueeze(0)
    sd = (far - near) / T
    if noise is not None:
        z = z + (torch.as_tensor(noise, dtype=torch.float32) - 0.5) * sd[:, None]
    delta = torch.cat([z[:, 1:] - z[:, :-1], sd[:, None]], -1)
    return z, delta


@pytest.mark.parametrize("name", ["run_foc.npz", "run_foc_b2.npz"])
def test_reference_forward_matches_the_run_fixtures(golden_dir, name):
    """The reference's image, depth and weights_sum against nerf.renderer.NeRFRenderer.run (fp32 torch) on the fixture's sigma / rgb:
    within the bound C * 2^-24 * (T + K) * mag that the GPU tests hold the kernels to. The fixture's rgbs are already masked by the
    reference's w > 1e-10; the float64 weights make the same decision except where fp32 loses alpha = 1 - exp(-delta * sigma) to
    rounding (delta * sigma < 2^-22: fp32 gives 0 or 2^-24 where float64 has 1e-10 .. 2e-7, tests/test_gpu_fixtures.py), and such a
    sample carries at most 2e-7 of the image either way."""
    g = np.load(os.path.join(golden_dir, name))
    N, T = g["sigmas"].shape
    z, delta = linspace_z(g["nears"], g["fars"], T)
    kept = (g["rgbs"] != 0).any(-1)
    ref = tail(z, delta, g["nears"], g["fars"], np.ones((N, 3)), 1.0, kept, sigma=g["sigmas"], rgb=g["rgbs"])
    w = ref["weights"].detach().numpy()
    step = (g["fars"] - g["nears"])[:, None] / (T - 1)
    differ = (w > 1e-10) != kept
    assert np.all((step * g["sigmas"])[differ] < 2.0 ** -22)
    m = magnitudes(ref)
    hit = g["nears"] < 1e30
    assert hit.sum() > 0.7 * N and (~hit).sum() > 0
    r_img = ratio(g["image"], ref["image"].detach().numpy(), m["image"], T)
    r_ws = ratio(g["weights_sum"], ref["weights_sum"].detach().numpy(), m["weights_sum"], T)
    r_dp = ratio(g["depth"][hit], ref["depth"].detach().numpy()[hit], m["depth"][hit], T)
    assert max(r_img, r_ws, r_dp) <= C, (r_img, r_ws, r_dp)
    np.testing.assert_allclose(ref["image"].detach().numpy(), g["image"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(ref["weights_sum"].detach().numpy(), g["weights_sum"], rtol=0, atol=2e-6)
    assert np.isnan(ref["depth"].detach().numpy()[~hit]).all() and np.isnan(g["depth"][~hit]).all()


def test_reference_agrees_with_the_oracle_composite():
    """oracle.composite_fixed_steps (fp32 C, no jitter, density_scale 1, a scalar background, no mask) on random fields, a ray that
    misses the box and opaque rays included: image, depth and weights within the bound."""
    rng = np.random.default_rng(11)
    N, T = 37, 200
    sig = np.exp(rng.standard_normal((N, T)) * 2.5).astype(np.float32)
    sig[5:9, 40:] = 3e4                                                   # opaque within a sample
    rgb = rng.random((N, T, 3)).astype(np.float32)
    near = (rng.random(N) * 0.5 + 0.2).astype(np.float32)
    far = (near + 1 + rng.random(N)).astype(np.float32)
    near[3] = far[3] = np.finfo(np.float32).max
    z, delta = linspace_z(near, far, T)
    ref = tail(z, delta, near, far, np.full((N, 3), 0.7), 1.0, np.ones((N, T), bool), sigma=sig, rgb=rgb)
    i4, dp, w = oracle.composite_fixed_steps(sig, rgb, near, far, bg=0.7, clamp01=False, want_weights=True)
    m = magnitudes(ref)
    hit = near < 1e30
    r = [ratio(i4[:, :3], ref["image"].detach().numpy(), m["image"], T), ratio(w, ref["weights"].detach().numpy(), m["weights"], T),
         ratio(dp[hit], ref["depth"].detach().numpy()[hit], m["depth"][hit], T)]
    assert max(r) <= C, r
    assert np.isnan(dp[~hit]).all() and np.isnan(ref["depth"].detach().numpy()[~hit]).all()
    assert (w[5:9, 42:] == 0).any() and (w[5:9, 42:] > 0).any()          # the oracle's transmittance runs through subnormals to 0


def _small_case(seed, N=3, T=6):
    rng = np.random.default_rng(seed)
    h0 = rng.uniform(-3, 3, (N, T))
    c = rng.standard_normal((N, T, 3))
    near = rng.uniform(0.2, 0.5, N).astype(np.float32)
    far = (near + 1 + rng.random(N)).astype(np.float32)
    z, delta = linspace_z(near, far, T, rng.random((N, T)))
    mask = rng.random((N, T)) > 0.3
    return h0, c, z, delta, near, far, rng.random((N, 3)), mask, rng


def test_reference_gradcheck():
    """Autograd's backward through the reference against finite differences (float64, small shapes, |h0| < 15 so trunc_exp is exp,
    sigmoid without the fp16 rounding, whose derivative is zero almost everywhere), all four incoming gradient terms; tail_backward()
    is autograd's gradient of that loss."""
    h0, c, z, delta, near, far, bg, mask, rng = _small_case(0)
    gi, gws, gdp, gsq = (torch.tensor(rng.standard_normal(s)) for s in ((3, 3), 3, 3, 3))

    def loss(h0_, c_):
        o = tail(z, delta, near, far, bg, 3.0, mask, h0=h0_, c=c_, half_rgb=False)
        return (gi * o["image"]).sum() + (gws * o["weights_sum"]).sum() + (gdp * o["depth"]).sum() + (gsq * o["sumsq"]).sum()

    h0t, ct = torch.tensor(h0, requires_grad=True), torch.tensor(c, requires_grad=True)
    assert torch.autograd.gradcheck(loss, (h0t, ct), eps=1e-6, atol=1e-7, rtol=1e-6)
    got = tail_backward(tail(z, delta, near, far, bg, 3.0, mask, h0=h0, c=c, half_rgb=False), gi, gws, gdp, gsq)
    want_h0, want_c = torch.autograd.grad(loss(h0t, ct), (h0t, ct))
    torch.testing.assert_close(got["grad_h0"], want_h0, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(got["grad_c"], want_c, rtol=1e-12, atol=1e-14)


def test_reference_rules_of_the_operation():
    """The pieces of the reference that are rules rather than arithmetic: trunc_exp's clamped backward, the fp16 y of the sigmoid's
    backward (at +7 the rounding moves 1 - y by ~7 %, at +12 y is exactly 1), no depth term on a ray whose grad_depth is 0 (finite rows
    on a ray that misses the box), and midpoint clearance of the colour logits."""
    h0, c, z, delta, near, far, bg, mask, rng = _small_case(1, N=2, T=4)
    h0[0, :] = [16.5, -15.0078125, 3.0, 15.0]
    c[0, :, 0] = [7.0, 12.0, -12.0, 0.0]
    mask[:] = True
    near[1] = far[1] = np.finfo(np.float32).max
    z, delta = linspace_z(near, far, 4)
    ref = tail(z, delta, near, far, bg, 1.0, mask, h0=h0, c=c)
    gi = np.ones((2, 3))
    g = tail_backward(ref, gi, grad_depth=np.zeros(2))
    w = ref["weights"].detach().numpy()
    y = (1 / (1 + np.exp(-c[0, :, 0]))).astype(np.float16).astype(np.float64)
    np.testing.assert_allclose(g["grad_c"][0, :, 0].numpy(), w[0] * y * (1 - y), rtol=1e-14)
    assert y[1] == 1.0 and g["grad_c"][0, 1, 0] == 0
    y64 = 1 / (1 + np.exp(-7.0))
    assert abs((1 - y[0]) / (1 - y64) - 1) > 0.05
    gs = tail_backward(ref, np.zeros((2, 3)), grad_sumsq=np.ones(2))["grad_h0"].numpy()
    sig = np.exp(h0[0])
    np.testing.assert_allclose(gs[0], 2 * sig * np.exp(np.clip(h0[0], -15, 15)), rtol=1e-14)
    assert np.isfinite(g["grad_h0"].numpy()).all() and (g["grad_h0"][1] == 0).all()
    assert np.isnan(ref["depth"].detach().numpy()[1])
    assert np.isnan(tail_backward(ref, gi, grad_depth=np.ones(2))["grad_h0"].numpy()[1]).all()
    cc = clear_of_half_midpoints(rng.standard_normal(20000).astype(np.float16) * 4)
    y = 1 / (1 + np.exp(-cc.astype(np.float64)))
    assert np.array_equal(y.astype(np.float32).astype(np.float16), y.astype(np.float16))


@pytest.mark.parametrize("T", [2, 65, 512])
def test_fp32_evaluation_stays_within_the_bound(T):
    """The bound's own check: the reference's expressions evaluated in fp32 (torch's CPU kernels, their own association orders) stay
    within C * 2^-24 * (T + K) * mag of the float64 values — forward outputs and the gradients of all four terms — on transparent,
    typical, opaque and box-missing rays with density_scale 3 and jittered depths."""
    rng = np.random.default_rng(T)
    N = 24
    h0 = (rng.standard_normal((N, T)) * 2).astype(np.float16).astype(np.float64)
    h0[0:4] = rng.uniform(-16, -8, (4, T)).astype(np.float16)
    h0[4:8, T // 3:] = rng.uniform(4, 16.5, (4, T - T // 3)).astype(np.float16)
    h0[8, :] = np.resize([14.5, -14.5, 15, -15, 15.0078125, -15.0078125], T)
    c = clear_of_half_midpoints((rng.standard_normal((N, T, 3)) * 3).astype(np.float16)).astype(np.float64)
    c[9, :, 0] = np.resize([7.0, 12.0, -12.0], T)
    near = rng.uniform(0.2, 0.5, N).astype(np.float32)
    far = (near + 1 + rng.random(N)).astype(np.float32)
    near[10] = far[10] = np.finfo(np.float32).max
    noise = rng.random((N, T)).astype(np.float32)
    noise[:, 0], noise[:, -1] = 0.0, np.float32(0.99999994)
    z, delta = linspace_z(near, far, T, noise)
    bg = rng.random((N, 3))
    mask = np.ones((N, T), bool)
    grads = dict(grad_image=rng.standard_normal((N, 3)), grad_ws=rng.standard_normal(N) * 0.05, grad_depth=rng.standard_normal(N) * 0.1,
                 grad_sumsq=rng.standard_normal(N) * 1e-9)
    grads["grad_depth"][10] = 0.0
    r64 = tail(z, delta, near, far, bg, 3.0, mask, h0=h0, c=c)
    mask = r64["weights"].detach().numpy() > 1e-10
    r64 = tail(z, delta, near, far, bg, 3.0, mask, h0=h0, c=c)
    r32 = tail(z, delta, near, far, bg, 3.0, mask, h0=h0, c=c, dtype=torch.float32)
    m = magnitudes(r64, **grads)
    g64, g32 = tail_backward(r64, **grads), tail_backward(r32, **grads)
    worst = {}
    for k in ("sigma", "trans", "weights", "weights_sum", "image", "sumsq"):
        worst[k] = ratio(r32[k].detach().numpy(), r64[k].detach().numpy(), m[k], T)
    hit = near < 1e30
    worst["depth"] = ratio(r32["depth"].detach().numpy()[hit], r64["depth"].detach().numpy()[hit], m["depth"][hit], T)
    for k in ("grad_h0", "grad_c", "grad_w"):
        worst[k] = ratio(g32[k].numpy(), g64[k].numpy(), m[k], T)
    assert max(worst.values()) <= C, worst
