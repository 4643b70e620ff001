"""CPU: pin the float64 reference of the occupancy-grid path's compositing (tests/ragged_ref.py) that test_gpu_ragged_reference.py measures
the kernels against — against the C oracle, against autograd's numerical gradient — and its error bound C * 2^-24 * (T + K) * mag, C = 2,
K = 16, against an fp32 torch evaluation of the reference's own expressions (__expf modelled as exp2(fl32(a log2 e))) on every case the GPU
file draws. The kernels are held to exactly this C and K, measured against float64, never against the kernels.

Worst ratios |fp32 - float64| / (2^-24 (T + K) mag) of the fp32 evaluation over all cases (asserted <= C = 2):
    composite form: weights_sum / depth / image / grad_rgb 0.029, grad_sigma 0.018
    tail form:      weights_sum / image_raw / grad_c 0.029, image 0.016, depth 0.0005, sumsq 0.024, grad_h0 0.022
    burst:          weights_sum 0.042, depth 0.061, image 0.076, rays_t 0.16

Mutants (applied to the fp32 CPU evaluation only; worst ratio at the case that is asserted, the bound is 2):
    mutant                                                   case                      ratio
    T_carry dropped at a chunk seam                          constructed[37,0.0001]    inf (a weight where float64 has exactly 0)
    t_carry dropped at a chunk seam                          constructed[3,0]          3.3e2 (depth)
    colour carry dropped at a chunk seam (backward)          random[37,502]            2.1e3 (grad_sigma)
    `lane < first` in place of `lane <= first`               constructed[37,0.0001]    3.3e5
    stop before accumulating the threshold sample (forward)  constructed[37,0.0001]    3.3e5
    density_scale omitted in the backward                    random[37,502]            2.5e4 (grad_h0)
    -(g . bg) omitted from the opacity gradient              random[37,703]            4.2e4 (grad_h0)
    trunc_exp's backward without the clamp                   random[37,404]            6.9e5 (grad_h0)
    sumsq term only on rows before the stop                  constructed[37,0.0001]    1.9e5 (grad_h0)
    inference: T after the sample in the stop test           burst[63x3,41]            inf (another kill decision)
    inference: rays_t written for a ray that died            burst[63x3,41]            inf (rays_t must keep its bits)
"""
import numpy as np
import pytest
import torch

import oracle
import ragged_ref as R
from ragged_ref import C

CASES = R.train_cases()
BURSTS = R.burst_cases()
IDS = [d["name"] for d in CASES]
BURST_IDS = [b["name"] + "-" + form for form, b in BURSTS]
TAIL_ONLY = ("ds_backward", "no_bg_grad", "unclamped", "sumsq_before_stop")
WORST = {}


def _candidates(d, form, bg_ray=True):
    vals, mags, fwd = R.evaluate(d, form, None, bg_ray=bg_ray, mags=True)
    return R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]


def _fp32(d, form, bg_ray, on, mutant=None):
    """The fp32 evaluation (its own stop decisions) of a case against float64 at the candidate stops: per-ray worst ratio, per-output worst."""
    cands, L = _candidates(d, form, bg_ray)
    if mutant == "stop_before_fwd":                                   # the forward drops the threshold sample, the backward does not
        got = R.evaluate(d, form, None, on=on, bg_ray=bg_ray, dtype=torch.float32)[0]
        wrong = R.evaluate(d, form, None, on=on, bg_ray=bg_ray, dtype=torch.float32, mutant="lane_lt_first")[0]
        got.update({k: v for k, v in wrong.items() if not k.startswith("grad")})
    else:
        got = R.evaluate(d, form, None, on=on, bg_ray=bg_ray, dtype=torch.float32, mutant=mutant)[0]
    best, _, per = R.match(cands, lambda stops: R.evaluate(d, form, stops, on=on, bg_ray=bg_ray, mags=True)[:2], got, L, half=())
    return best, per


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_undecided_ray_cap(d):
    """At most 2 % of a case's rays have more than one stop candidate, none of a constructed case's; and the constructed stops are where
    they were placed."""
    for form in ("composite", "tail"):
        cands, L = _candidates(d, form)
        n = sum(len(c) > 1 for c in cands)
        assert n <= 0.02 * d["N"], (form, n)
        if "stops" in d:
            assert n == 0
            want = [p if p is not None else max(int(c) - 1, 0) for p, c in zip(d["stops"], d["rays"][:, 2])]
            assert R.stops_of(cands, 0).tolist() == want


@pytest.mark.parametrize("fb", BURSTS, ids=BURST_IDS)
def test_undecided_burst_cap(fb):
    form, b = fb
    ref = R.burst(*R.burst_args(b))
    m = R.burst_magnitudes(b["n_step"], *R.burst_args(b)[2:])
    cands = R.burst_candidates(b["n_step"], b["T_thresh"], b["deltas"], ref["T"], m["T"])
    n = sum(len(c) > 1 for c, l in zip(cands, ref["listed"]) if l)
    assert n <= 0.02 * ref["listed"].sum()
    regime = (np.arange(b["n_alive"]) + int(b["name"].split(",")[1][:-1])) % 8
    assert not any(len(c) > 1 for c, l, r in zip(cands, ref["listed"], regime) if l and r in (2, 3, 4, 5)), "a constructed row is undecided"


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_fp32_evaluation_of_the_training_forms_stays_within_the_bound(d):
    """Both forms, a per-ray and a scalar background, every incoming gradient term alone and all together."""
    for form in ("composite", "tail"):
        for bg_ray in ((True, False) if form == "tail" else (True,)):
            for on in R.combos(form):
                best, per = _fp32(d, form, bg_ray, on)
                for k, v in per.items():
                    WORST[f"{form}.{k}"] = max(WORST.get(f"{form}.{k}", 0.0), v)
                assert best.max() <= C, (form, bg_ray, on, per)


@pytest.mark.parametrize("fb", BURSTS, ids=BURST_IDS)
def test_fp32_evaluation_of_the_burst_stays_within_the_bound(fb):
    form, b = fb
    best, per, _ = R.burst_match(b, R.burst(*R.burst_args(b), dtype=torch.float32))
    for k, v in per.items():
        WORST[f"burst.{k}"] = max(WORST.get(f"burst.{k}", 0.0), v)
    assert best.max() <= C, per


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_reference_agrees_with_the_oracle_training_composite(d):
    """oracle.composite_rays_train_forward / _backward (fp32 C, sequential) on the case's sigma / rgb: outputs and gradients within the
    bound of the reference at a candidate stop; rows the oracle leaves alone are the reference's zeros."""
    sig, rgb = R.composite_inputs(d)
    N, M = d["N"], d["M"]
    ws, dp, im = oracle.composite_rays_train_forward(sig, rgb, d["deltas"], d["rays"], N, d["T_thresh"])
    g = R.grads_of(d, R.TERMS[:2], "composite")
    gs, gc = oracle.composite_rays_train_backward(g["grad_ws"], g["grad_image"], sig, rgb, d["deltas"], d["rays"], ws, im, d["T_thresh"])
    cands, L = _candidates(d, "composite")
    got = dict(weights_sum=R.by_list(L, ws), depth=R.by_list(L, dp), image=R.by_list(L, im), grad_sigma=R.gather(L, gs), grad_rgb=R.gather(L, gc))
    best, _, per = R.match(cands, lambda stops: R.evaluate(d, "composite", stops, on=R.TERMS[:2], mags=True)[:2], got, L, half=())
    assert best.max() <= C, per
    inside = np.zeros(M, bool)
    inside[L["rows"][L["valid"]]] = True
    assert not gs[~inside].any() and not gc[~inside].any()


@pytest.mark.parametrize("fb", BURSTS[:8], ids=BURST_IDS[:8])
def test_reference_agrees_with_the_oracle_burst(fb):
    """oracle.composite_rays on the listed rows (the oracle does not skip -1 entries)."""
    form, b = fb
    keep = b["rays_alive"] >= 0
    n, s = int(keep.sum()), b["n_step"]
    b = dict(b, n_alive=n, rays_alive=b["rays_alive"][keep], sigmas=b["sigmas"].reshape(-1, s)[keep].reshape(-1),
             rgbs=b["rgbs"].reshape(-1, s, 3)[keep].reshape(-1, 3), deltas=b["deltas"].reshape(-1, s, 2)[keep].reshape(-1, 2))
    alive, t, ws, dp, im = oracle.composite_rays(n, s, b["T_thresh"], b["rays_alive"], b["rays_t"], b["sigmas"], b["rgbs"], b["deltas"], b["weights_sum"],
                                                 b["depth"], b["image"])
    best, per, _ = R.burst_match(b, dict(rays_alive=alive, rays_t=t, weights_sum=ws, depth=dp, image=im))
    assert best.max() <= C, per
    out = np.ones(b["n_rays"], bool)
    out[b["rays_alive"]] = False
    assert np.array_equal(ws[out], b["weights_sum"][out]) and np.array_equal(t[out], b["rays_t"][out])


def _three_rays():
    rays = np.array([[2, 0, 3], [0, 3, 5], [1, 8, 2]], np.int32)
    rng = np.random.default_rng(0)
    deltas = np.stack([rng.uniform(0.05, 0.3, 10), rng.uniform(0.05, 0.3, 10)], 1).astype(np.float32)
    deltas[3:5, 0] = [2e-7, 3e-7]                                         # the samples at trunc_exp's clamp: short steps, so a gradient remains
    h0 = rng.uniform(-2, 2, (3, 5))
    h0[1, 0], h0[1, 1] = 15.0, -15.0
    return rays, deltas, h0, rng.standard_normal((3, 5, 3)), rng


def test_reference_gradcheck():
    """Autograd's backward through the tail form against finite differences: float64, 3 rays (one stopped before its end), h0 at
    trunc_exp's clamp +-15 (where the clamped backward is still the derivative), density_scale 2, a per-ray background, all three
    incoming terms; sigmoid without its fp16 rounding, whose derivative is zero almost everywhere."""
    rays, deltas, h0, c, rng = _three_rays()
    gi, gws, gsq = (torch.tensor(rng.standard_normal(s)) for s in ((3, 3), 3, 3))
    gsq = gsq * torch.tensor([1e-12, 1e-2, 1e-2])                   # output row 0 is the ray with exp(15)^2 = 1e13 in its sum
    bg, near, far = rng.random((3, 3)), np.full(3, 0.1, np.float32), np.full(3, 2.0, np.float32)
    stop = np.array([1, 4, 1])

    def loss(h0_, c_):
        o = R.train(rays, 10, deltas, stop, h0=h0_, c=c_, density_scale=2.0, bg=bg, nears=near, fars=far, half_rgb=False)
        return (gi * o["image"]).sum() + (gws * o["weights_sum"]).sum() + (gsq * o["sumsq"]).sum()

    h0t, ct = torch.tensor(h0, requires_grad=True), torch.tensor(c, requires_grad=True)
    assert torch.autograd.gradcheck(loss, (h0t, ct), eps=1e-6, atol=1e-7, rtol=1e-5)
    o = R.train(rays, 10, deltas, stop, h0=h0t, c=ct, density_scale=2.0, bg=bg, nears=near, fars=far, half_rgb=False)
    got = R.train_backward(o, gi, gws, gsq)
    want = torch.autograd.grad(loss(h0t, ct), (h0t, ct))
    torch.testing.assert_close(got["grad_h0"], want[0], rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(got["grad_c"], want[1], rtol=1e-12, atol=1e-14)


def test_reference_rules_of_the_operation():
    """The rules that are not arithmetic: an empty ray and a ray past the list give zeros (tail form: the background) and take no
    gradient; rays[:, 0] decides the output row; trunc_exp's backward is clamped beyond +-15; depth has no gradient; ray_sumsq and its
    backward cover the rows behind the stop; a ray that died in a burst keeps its rays_t, skipped entries change nothing."""
    rng = np.random.default_rng(1)
    rays = np.array([[3, 0, 4], [1, 4, 0], [0, 4, 3], [2, 7, 6]], np.int32)       # the last ray does not fit M = 10
    h0 = rng.uniform(-1, 1, 10)
    h0[0], h0[3] = 16.5, -15.0078125
    deltas = np.full((10, 2), 0.2, np.float32)
    deltas[0, 0] = 1e-8
    bg = rng.random((4, 3))
    near, far = np.full(4, 0.1), np.full(4, 2.0)
    stop = np.array([1, 0, 2, 5])
    o = R.train(rays, 10, deltas, stop, h0=h0, c=rng.standard_normal((10, 3)), bg=bg, nears=near, fars=far)
    ws, img = o["weights_sum"].detach().numpy(), o["image"].detach().numpy()
    assert ws[1] == 0 and ws[2] == 0 and ws[3] > 0 and ws[0] > 0
    np.testing.assert_array_equal(img[[1, 2]], bg[[1, 2]])
    assert o["depth"][1] == 0 and o["depth"][2] == 0 and o["sumsq"][1] == 0 and o["sumsq"][2] == 0 and not o["depth"].requires_grad
    np.testing.assert_allclose(o["sumsq"][3].item(), np.exp(2 * h0[:4]).sum(), rtol=1e-14)
    g = R.train_backward(o, np.zeros((4, 3)), grad_sumsq=np.ones(4))["grad_h0"].numpy()
    x = h0[:4]
    np.testing.assert_allclose(g[0, :4], 2 * np.exp(x) * np.exp(np.clip(x, -15, 15)), rtol=1e-14)      # rows 2, 3 lie behind the stop
    assert not g[1].any() and not g[3].any() and g[2, :3].all()
    g = R.train_backward(o, np.ones((4, 3)), grad_ws=np.ones(4))
    assert not g["grad_h0"].numpy()[0, 2:].any() and not g["grad_c"].numpy()[0, 2:].any() and g["grad_h0"].numpy()[0, :2].all()
    form, b = BURSTS[1]
    ref = R.burst(*R.burst_args(b))
    dead = ref["died"] & ref["listed"]
    assert dead.any() and (~dead & ref["listed"]).any() and (~ref["listed"]).any()
    assert np.array_equal(ref["rays_t"][ref["index"][dead]], b["rays_t"][ref["index"][dead]].astype(np.float64))
    assert (ref["rays_alive"][dead] == -1).all() and np.array_equal(ref["rays_alive"][~dead], b["rays_alive"][~dead])


_CAUGHT_BY = {"T_carry": 8, "t_carry": 11, "colour_carry": 5, "lane_lt_first": 8, "stop_before_fwd": 8, "ds_backward": 5, "no_bg_grad": 7,
              "unclamped": 4, "sumsq_before_stop": 8, "T_after_test": 1, "dead_rays_t": 1}
WIDE = 50 * C


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_bound_catches_the_mutant(mutant):
    """Each deliberately wrong fp32 evaluation leaves the bound by at least 50 x on the case named in the module docstring."""
    assert set(_CAUGHT_BY) == set(R.MUTANTS)
    if mutant in ("T_after_test", "dead_rays_t"):
        form, b = BURSTS[_CAUGHT_BY[mutant]]
        best, per, _ = R.burst_match(b, R.burst(*R.burst_args(b), dtype=torch.float32, mutant=mutant))
    else:
        d = CASES[_CAUGHT_BY[mutant]]
        form = "tail" if mutant in TAIL_ONLY else "composite"
        best, per = _fp32(d, form, True, R.combos(form)[-1], mutant=mutant)
    assert best.max() > WIDE, (mutant, per)
