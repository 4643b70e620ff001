"""CPU: pin the float64 reference of the per-ray distortion (tests/distortion_ref.py) that test_gpu_distortion.py measures the tail kernels
against — against the O(T^2) definition, against autograd, against the reference's eff_distloss (tests/golden/eff_distloss.npz, made by
tests/golden/make_golden_distortion.py) — `focnerf_amd.loss.ray_distortion` against it, and the bound C * 2^-24 * (T + K) * mag, C = 2, K = 16,
against an fp32 CPU evaluation of every case the GPU file runs (the bound is attainable before a GPU sees it). The host-side refusals of the
four entry points need no GPU and are here too.

Worst ratios |fp32 - float64| / (2^-24 (T + K) mag) of the fp32 CPU evaluation over all cases (asserted <= C = 2):
    fixed-step: ray_dist 0.020, ray_wm 0.024, grad_h0 0.029          ragged: ray_dist 0.029, ray_wm 0.029, grad_h0 0.018
With the distortion's gradient left out of the fp32 evaluation the same comparison gives 59 .. 222 (ragged) and 102 (fixed-step): the bound
notices the term it was extended for.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import distortion_ref as D
import ragged_ref as R
from distortion_ref import C
from fixed_tail_ref import tail
from test_fixed_tail_ref import linspace_z

CASES = R.train_cases()
IDS = [d["name"] for d in CASES]
FIXED_T, FIXED_N = D.FIXED_T, D.FIXED_N
WORST = {}


def _rand(seed, N=5, T=70):
    rng = np.random.default_rng(seed)
    delta = torch.tensor(rng.uniform(1e-3, 5e-2, (N, T)))
    m = torch.cumsum(delta, -1) - 0.5 * delta + 0.3
    alpha = torch.tensor(rng.uniform(0, 0.3, (N, T)) * (rng.random((N, T)) < 0.8))
    w = alpha * torch.cumprod(torch.cat([torch.ones(N, 1, dtype=torch.float64), 1 - alpha[:, :-1]], -1), -1)
    return w, m, delta


def test_reference_is_the_double_sum():
    w, m, delta = _rand(0)
    dist, wm = D.distortion(w, m, delta)
    torch.testing.assert_close(dist, D.pairwise(w, m, delta), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(wm, (w * m).sum(-1), rtol=1e-14, atol=0)


def test_weight_gradient_is_autograd():
    w, m, delta = _rand(1)
    w.requires_grad_(True)
    g, = torch.autograd.grad(D.distortion(w, m, delta)[0].sum(), w)
    torch.testing.assert_close(D.weight_gradient(w.detach(), m, delta), g, rtol=1e-11, atol=1e-14)
    gp, = torch.autograd.grad(D.pairwise(w, m, delta).sum(), w)
    torch.testing.assert_close(g, gp, rtol=1e-10, atol=1e-13)
    # sum_i G_i w_i = 2 dist: the loss is homogeneous of degree 2 in w (the ragged backward takes its total from the forward's output)
    torch.testing.assert_close((D.weight_gradient(w.detach(), m, delta) * w.detach()).sum(-1), 2 * D.distortion(w.detach(), m, delta)[0], rtol=1e-12, atol=0)


def test_reference_and_fallback_match_eff_distloss(golden_dir):
    """The reference's loss (a mean over rays) and gradient, times the ray count, against distortion_ref and focnerf_amd.loss.ray_distortion."""
    from focnerf_amd.loss import ray_distortion
    g = np.load(os.path.join(golden_dir, "eff_distloss.npz"))
    assert int(g["n_cases"]) >= 5
    forms = set()
    for k in range(int(g["n_cases"])):
        w, m = torch.tensor(g[f"w{k}"]), torch.tensor(g[f"m{k}"])
        iv = g[f"interval{k}"]
        forms.add(iv.ndim)
        B = w.shape[0]
        delta = torch.tensor(iv) if iv.ndim else torch.full_like(w, float(iv))
        dist = D.distortion(w, m, delta)[0]
        np.testing.assert_allclose(dist.sum().item(), float(g[f"loss{k}"]) * B, rtol=1e-12)
        np.testing.assert_allclose(D.weight_gradient(w, m, delta).numpy(), g[f"grad{k}"] * B, rtol=1e-10, atol=1e-15)
        wl = w.clone().requires_grad_(True)
        got = ray_distortion(wl, m, delta if iv.ndim else float(iv))
        torch.testing.assert_close(got, dist, rtol=1e-12, atol=1e-16)
        gl, = torch.autograd.grad(got.sum(), wl)
        np.testing.assert_allclose(gl.numpy(), g[f"grad{k}"] * B, rtol=1e-10, atol=1e-15)
    assert forms == {0, 2}, "tensor and scalar intervals"


def test_fallback_detaches_m_and_interval():
    from focnerf_amd.loss import ray_distortion
    w, m, delta = _rand(2, N=2, T=9)
    w.requires_grad_(True); m.requires_grad_(True); delta.requires_grad_(True)
    ray_distortion(w, m, delta).sum().backward()
    assert w.grad is not None and m.grad is None and delta.grad is None


def _record(tag, k, r):
    WORST[f"{tag}.{k}"] = max(WORST.get(f"{tag}.{k}", 0.0), float(np.max(r, initial=0.0)))


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("T", FIXED_T)
def test_fp32_evaluation_of_the_fixed_step_cases_stays_within_the_bound(T, cfg):
    for N in FIXED_N:
        d, g, gd, o = D.fixed_case(N, T, cfg)
        z, delta = linspace_z(d["near"], d["far"], T, d["noise"] if o["noise"] else None)
        bg = d["bg"] if o["bg_ray"] else np.full((N, 3), 0.7, np.float32)
        mask = tail(z, delta, d["near"], d["far"], bg, o["ds"], np.ones((N, T), bool), h0=d["h0"], c=d["c"])["weights"].detach().numpy() > o["thresh"]
        r64 = tail(z, delta, d["near"], d["far"], bg, o["ds"], mask, h0=d["h0"], c=d["c"])
        r32 = tail(z, delta, d["near"], d["far"], bg, o["ds"], mask, h0=d["h0"], c=d["c"], dtype=torch.float32)
        d64, d32 = D.fixed(r64), D.fixed(r32)
        mags = D.fixed_magnitudes(r64, d64, gd, **g)
        b64, b32 = D.fixed_backward(r64, d64, gd, **g), D.fixed_backward(r32, d32, gd, **g)
        assert (d64["dist"][d["missed"]] == 0).all() and (d64["wm"][d["missed"]] == 0).all()
        for k, got, want in (("ray_dist", d32["dist"], d64["dist"]), ("ray_wm", d32["wm"], d64["wm"]), ("grad_h0", b32["grad_h0"], b64["grad_h0"])):
            mk = mags[{"ray_dist": "dist", "ray_wm": "wm"}.get(k, k)].numpy()
            keep = ~d["missed"] if k == "grad_h0" else slice(None)         # a missed ray's rows are NaN with a depth gradient: the family's own test
            r = R.ratios(got.detach().numpy()[keep], want.detach().numpy()[keep], mk[keep], T)
            _record("fixed", k, r)
            assert r.max(initial=0.0) <= C, (N, T, cfg, k, r.max())


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_fp32_evaluation_of_the_ragged_cases_stays_within_the_bound(d):
    gd = D.grad_dist_of(d)
    vals, mags, fwd = R.evaluate(d, "tail", None, mags=True)
    cands, L = R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]
    n = sum(len(c) > 1 for c in cands)
    assert n <= 0.02 * d["N"] and ("stops" not in d or n == 0)
    got = D.ragged_evaluate(d, None, on=R.TERMS, grad_dist=gd, dtype=torch.float32)[0]
    best, _, per = R.match(cands, lambda stops: D.ragged_evaluate(d, stops, on=R.TERMS, grad_dist=gd, mags=True)[:2], got, L, half=())
    for k, v in per.items():
        _record("ragged", k, v)
    assert best.max() <= C, per
    out = ~L["fits"]
    assert not got["ray_dist"][out].any() and not got["ray_wm"][out].any()


ONE = ctypes.c_void_p(64)


def test_entry_points_refuse_null_outputs():
    """Before any launch: the forwards without ray_dist / ray_wm, the backwards whose grad_dist comes without the forward's totals, a c_width
    other than 4 or 16 (the plain entry points' checks, under the new names)."""
    from focnerf_amd._lib import lib
    err = lib.foc_last_error
    fx = (ONE, ONE, ONE, ONE, None, None, 1.0, 4, 8, 1.0, 1e-4, ONE, ONE, ONE, ONE, ONE, ONE, 4, None)
    for rd, wm in ((None, ONE), (ONE, None), (None, None)):
        assert lib.foc_fixed_tail_forward_dist(*fx, rd, wm, None) != 0 and b"fixed_tail_forward_dist: null ray_dist / ray_wm" in err()
    assert lib.foc_fixed_tail_forward_dist(*fx[:17], 8, None, ONE, ONE, None) != 0 and b"fixed_tail_forward_dist: c_width" in err()
    fb = (ONE, None, None, ONE, ONE, ONE, ONE, None, ONE, ONE, None, None, 1.0, 4, 8, 1.0, 1e-4, ONE, ONE, 4, None)
    assert lib.foc_fixed_tail_backward_dist(*fb, ONE, None, ONE, None) != 0 and b"fixed_tail_backward_dist: grad_dist needs weights_sum and ray_wm" in err()
    assert lib.foc_fixed_tail_backward_dist(*fb[:7], ONE, *fb[8:], None, None, ONE, None) != 0 and b"grad_dist needs weights_sum and ray_wm" in err()
    assert lib.foc_fixed_tail_backward_dist(*fb[:7], ONE, *fb[8:14], 1, *fb[15:], ONE, None, ONE, None) != 0 and b"fixed_tail_backward_dist: T must be >= 2" in err()
    of = (ONE, ONE, 4, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, ONE, ONE, ONE, ONE, None)
    for rd, wm in ((None, ONE), (ONE, None)):
        assert lib.foc_occ_tail_forward_dist(*of, rd, wm, None) != 0 and b"occ_tail_forward_dist: null ray_dist / ray_wm" in err()
    assert lib.foc_occ_tail_forward_dist(*of[:2], 8, *of[3:], ONE, ONE, None) != 0 and b"occ_tail_forward_dist: c_width" in err()
    ob = (ONE, None, ONE, ONE, 4, ONE, ONE, ONE, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, None)
    for wm, rd in ((None, ONE), (ONE, None)):
        assert lib.foc_occ_tail_backward_dist(*ob, wm, rd, ONE, None) != 0 and b"occ_tail_backward_dist: grad_dist needs ray_wm and ray_dist" in err()
    assert lib.foc_occ_tail_backward_dist(*ob[:4], 8, *ob[5:], ONE, ONE, ONE, None) != 0 and b"occ_tail_backward_dist: c_width" in err()
