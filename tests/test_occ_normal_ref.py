"""CPU: tests/occ_normal_ref.py — the float64 composite of two payloads and the normal map's finish — pinned against an independent cumprod
formulation and the C oracle's composite_rays, its bound held by an fp32 evaluation of the same expressions and shown to reject each mutant."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import occ_normal_ref as R      # noqa: E402

RAYS, STEPS, T_THRESH = (1, 63, 65, 130, 1500), (16, 256), 1e-4
NAMES = ("W", "depth", "A", "B", "normal", "normal_rgb")


@functools.lru_cache(maxsize=None)
def _lists(n, S, thin=False):
    return R.random_lists(np.random.default_rng(1000 * S + n + (7 if thin else 0)), n, S, thin=thin)


@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("n", RAYS)
def test_composite_is_the_cumprod_formulation(n, S):
    """w_j = alpha_j prod_{i<j} (1 - alpha_i), summed up to and including the first sample whose transmittance BEFORE it is below the
    threshold — written with cumprod on whole arrays, no recurrence; both payloads, the depth from cumsum(dt1)."""
    sigma, dt0, dt1, a, b = _lists(n, S)
    ref = R.composite(sigma, dt0, dt1, a, b, T_THRESH)
    sg, d0, d1 = (torch.as_tensor(x) for x in (sigma, dt0, dt1))
    alpha = 1 - torch.exp(-sg * d0)
    before = torch.cumprod(torch.cat([torch.ones(n, 1, dtype=torch.float64), 1 - alpha], 1), 1)[:, :-1]
    valid = torch.cumprod((d0 != 0).double(), 1) > 0
    stopped = torch.cumsum(torch.cat([torch.zeros(n, 1), (before < T_THRESH).double()[:, :-1]], 1), 1) > 0
    w = alpha * before * (valid & ~stopped)
    t = torch.cumsum(d1, 1)
    want = dict(W=w.sum(1), depth=(w * t).sum(1), A=(w[:, :, None] * torch.as_tensor(a)).sum(1), B=(w[:, :, None] * torch.as_tensor(b)).sum(1))
    assert np.array_equal(ref["n_acc"], (valid & ~stopped).sum(1).numpy())
    for k, v in want.items():
        np.testing.assert_allclose(ref[k], v.numpy(), rtol=1e-11, atol=1e-300, err_msg=k)
    assert n == 1 or ((ref["W"] > 1 - T_THRESH).any() and (ref["W"] < 0.5).any() and (ref["n_acc"] < R.valid_counts(dt0)).any())


@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("n", RAYS)
def test_first_payload_is_the_oracles_composite_rays(n, S):
    """oracle/oracle.c composite_rays on the lists as ONE burst of S samples per ray, from zero accumulators: fp32 C against float64,
    inside the bound (first payload; the second through the same call with the payloads swapped: one definition of the weights)."""
    import oracle
    sigma, dt0, dt1, a, b = _lists(n, S)
    deltas = np.stack([dt0, dt1], 2).astype(np.float32)
    for first, second, name in ((a, b, "A"), (b, a, "B")):
        alive, t, W, depth, image = oracle.composite_rays(n, S, T_THRESH, np.arange(n, dtype=np.int32), np.zeros(n, np.float32), sigma.astype(np.float32),
                                                          first.astype(np.float32), deltas, np.zeros(n, np.float32), np.zeros(n, np.float32),
                                                          np.zeros((n, 3), np.float32))
        got = {"W": W, "depth": depth, name: image}
        ratio, _, _ = R.best_ratio(got, sigma, dt0, dt1, a, b, T_THRESH, ("W", "depth", name))
        assert ratio.max() <= 1.0, (name, ratio.max())
    ref = R.composite(sigma, dt0, dt1, a, b, T_THRESH)
    died = (ref["n_acc"] < S) | (ref["T"][:, S - 1] < T_THRESH)               # (the last sample's own test can end a full list too)
    undecided = R.best_ratio(got, sigma, dt0, dt1, a, b, T_THRESH, ("W",))[2]
    assert np.array_equal((alive < 0)[~undecided], died[~undecided])       # a ray is marked dead exactly where the reference stops it early


@pytest.mark.parametrize("S", STEPS)
@pytest.mark.parametrize("n", RAYS)
def test_fp32_evaluation_stays_inside_the_bound(n, S):
    """The same expressions in fp32 (alpha through exp2(a log2 e), as __expf): every output of every ray inside the counted bound; pixels
    whose |s| is within its own error have no direction to compare, and they stay under 5 % of the pixels with W > 0."""
    sigma, dt0, dt1, a, b = _lists(n, S)
    c = R.composite(sigma, dt0, dt1, a, b, T_THRESH, dtype=torch.float32)
    normal, rgb, _ = R.finish(c["B"], c["W"], dtype=torch.float32)
    got = dict(c, normal=normal, normal_rgb=rgb)
    ratio, unresolved, _ = R.best_ratio(got, sigma, dt0, dt1, a, b, T_THRESH, NAMES)
    assert ratio.max() <= 1.0, ratio.max()
    hit = R.composite(sigma, dt0, dt1, a, b, T_THRESH)["W"] > 0
    assert (unresolved & hit).sum() <= 0.05 * max(hit.sum(), 1), (int((unresolved & hit).sum()), int(hit.sum()))


def test_named_cases_of_the_finish():
    """No sample: normal 0, opacity 0, normal_rgb 1. One opaque sample with normal n: normal = n, normal_rgb = 0.5 + 0.5 n. Zero normals
    only: s = 0 exactly, normal 0. A non-finite accumulator: normal 0."""
    n0 = np.array([0.6, 0.0, -0.8])
    sigma, dt0, dt1 = np.array([[0.0, 0.0], [1e6, 0.0], [1e6, 1.0]]), np.array([[0.0, 0.0], [0.01, 0.0], [0.01, 0.01]]), np.zeros((3, 2))
    b = np.stack([np.zeros((2, 3)), np.stack([0.5 + 0.5 * n0, np.zeros(3)]), np.full((2, 3), 0.5)])
    r = R.render(sigma, dt0, dt1, np.zeros((3, 2, 3)), b, T_THRESH)
    assert np.array_equal(r["n_acc"], [0, 1, 2]) and np.array_equal(r["W"], [0.0, 1.0, 1.0])
    assert np.array_equal(r["normal"][0], np.zeros(3)) and np.array_equal(r["normal_rgb"][0], np.ones(3)) and r["unresolved"][0]
    np.testing.assert_allclose(r["normal"][1], n0, atol=1e-15)
    np.testing.assert_allclose(r["normal_rgb"][1], 0.5 + 0.5 * n0, atol=1e-15)
    assert np.array_equal(r["normal"][2], np.zeros(3)) and np.array_equal(r["normal_rgb"][2], np.full(3, 0.5))
    normal, _, _ = R.finish(np.array([[np.inf, 0.2, 0.1], [np.nan, 0.2, 0.1]]), np.array([0.5, 0.5]))
    assert np.array_equal(normal, np.zeros((2, 3)))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bound_rejects_each_mutant(mutant):
    """Evaluated in float64 — no rounding to hide behind — each wrong variant leaves the bound on the lists of 130 rays. The threshold is
    1e-2 here: what a stop leaves out is at most the transmittance behind it, and behind 1e-4 the lists' opaque rays have less left than fp32
    resolves (the bound does not depend on the threshold)."""
    assert set(R.MUTANTS) == {"late_weights", "stop_one_payload", "wrong_W"}
    thresh = 1e-2
    for S in STEPS:
        sigma, dt0, dt1, a, b = _lists(130, S)
        c = R.composite(sigma, dt0, dt1, a, b, thresh, mutant=mutant)
        normal, rgb, _ = R.finish(c["B"], c["W"], mutant=mutant)
        got = dict(c, normal=normal, normal_rgb=rgb)
        ratio, _, _ = R.best_ratio(got, sigma, dt0, dt1, a, b, thresh, NAMES)
        assert (ratio > 1.0).sum() >= 5, (S, mutant, ratio.max())
        right = R.composite(sigma, dt0, dt1, a, b, thresh)                  # and what the mutant does not touch is still right
        assert np.array_equal(c["W"], right["W"]) and np.array_equal(c["A"], right["A"]) and np.array_equal(c["depth"], right["depth"])


def test_thin_lists_never_stop_early():
    sigma, dt0, dt1, a, b = _lists(130, 16, thin=True)
    ref = R.composite(sigma, dt0, dt1, a, b, T_THRESH)
    assert np.array_equal(ref["n_acc"], R.valid_counts(dt0)) and ref["W"].max() < 0.9
