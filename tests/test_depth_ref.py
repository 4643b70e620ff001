"""CPU: pin the float64 statement of the occupancy tail's differentiable depth (tests/depth_ref.py) that test_gpu_depth_grad.py measures
the kernels against — against finite differences, the kernel's closed form against autograd — and the bound C * 2^-24 * (T + K) * mag, C = 2,
K = 16, against an fp32 CPU evaluation of that closed form on every case the GPU file runs: the bound is attainable before a GPU sees it, and
it notices each way of getting the term wrong that depth_ref.MUTANTS names. The conditions on the cases (the clamp decided, the stops decided)
are asserted here on the reference alone. The host-side refusals of the new entry points need no GPU and are here too.

Worst ratio |fp32 - float64| / (2^-24 (T + K) mag) of grad_h0 over all cases (asserted <= C = 2): 0.018 (depth_raw 0.029). The mutants,
worst case each (cases above C of 12): no_depth 1284 (12), D_exclusive 1228 (12), no_clamp 1393 (8), no_span 675 (12), t_carry 344 (6),
behind_stop inf (7: the rows behind a stop have magnitude 0). The cases: 119 of the 156 fitting rays unclamped, the smallest
|depth_raw - near| 4.0 forward bounds away (the four rays whose margin depth_ref.cases() widens; 0.05 max(1, |depth_raw|) elsewhere).
"""
import ctypes

import numpy as np
import pytest
import torch

import depth_ref as DR
import ragged_ref as R
from depth_ref import C

CASES = DR.cases()
IDS = [d["name"] for d in CASES]
_CANDS = {}


def _candidates(d):
    if d["name"] not in _CANDS:
        vals, mags, fwd = R.evaluate(d, "tail", None, mags=True)
        _CANDS[d["name"]] = R.stop_candidates(fwd, mags, d["T_thresh"]), fwd["L"]
    return _CANDS[d["name"]]


def test_cases_leave_most_rays_unclamped_and_every_clamp_decided():
    """Three fitting rays of four are unclamped; no fitting ray's |depth_raw - near| lies within the forward bound of depth_raw at any of
    its stop candidates; at most 2 % of a case's rays have an undecided stop, none of a constructed case's."""
    total = unclamped = 0
    worst = np.inf
    for d in CASES:
        cands, L = _candidates(d)
        n = sum(len(c) > 1 for c in cands)
        assert n <= 0.02 * d["N"] and ("stops" not in d or n == 0), (d["name"], n)
        margin, u = DR.clamp_is_decided(d, cands)
        assert margin > 1.0, (d["name"], margin)
        worst = min(worst, margin)
        fits = L["fits"]
        want = int((~R.by_list(L, d["clamped"]) & fits).sum())
        assert u == want, (d["name"], u, want)
        assert (d["fars"] > d["nears"]).all()
        g = d["grad_depth"]
        assert d["N"] < 37 or ((g > 0).any() and (g < 0).any() and (g == 0).any())
        total += int(fits.sum())
        unclamped += u
    print("fitting rays", total, "unclamped", unclamped, "smallest clamp margin / bound", worst)
    assert unclamped >= 0.7 * total


def test_reference_gradcheck():
    """The float64 statement against finite differences: 3 rays (one stopped before its end, one clamped), density_scale 2, the depth term
    beside the image's; then the closed form against autograd on the same rays."""
    from test_ragged_ref import _three_rays
    rays, deltas, h0, c, rng = _three_rays()
    gi, gdep = torch.tensor(rng.standard_normal((3, 3))), torch.tensor(rng.standard_normal(3))
    bg = rng.random((3, 3))
    stop = np.array([1, 4, 1])
    o = R.train(rays, 10, deltas, stop, h0=torch.tensor(h0), c=torch.tensor(c), density_scale=2.0, bg=bg, nears=np.zeros(3), fars=np.ones(3), half_rgb=False)
    raw = o["depth_raw"].detach().numpy()
    near = np.array([raw[0] - 0.05, raw[1] + 0.05, raw[2] - 0.02])
    far = near + np.array([1.5, 0.7, 2.2])

    def loss(h0_, c_):
        o = R.train(rays, 10, deltas, stop, h0=h0_, c=c_, density_scale=2.0, bg=bg, nears=near, fars=far, half_rgb=False)
        return (gi * o["image"]).sum() + (gdep * DR.depth_of(o)).sum()

    h0t, ct = torch.tensor(h0, requires_grad=True), torch.tensor(c, requires_grad=True)
    assert torch.autograd.gradcheck(loss, (h0t, ct), eps=1e-6, atol=1e-7, rtol=1e-5)
    o = R.train(rays, 10, deltas, stop, h0=h0t, c=ct, density_scale=2.0, bg=bg, nears=near, fars=far, half_rgb=False)
    want, = torch.autograd.grad((gdep * DR.depth_of(o)).sum(), h0t, retain_graph=True)
    assert want.abs().max() > 0 and not want[int(np.nonzero(rays[:, 0] == 1)[0][0])].any(), "the clamped ray takes nothing"
    torch.testing.assert_close(DR.term(o, gdep.numpy()), want, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("d", CASES, ids=IDS)
def test_closed_form_is_autograd_on_every_case(d):
    """float64: depth_ref.term() — what the kernel evaluates — is the gradient torch.autograd.grad carries through the kept graph."""
    cands, L = _candidates(d)
    stops = R.stops_of(cands, 0)
    with_depth, _, fwd = DR.evaluate(d, stops, on=R.TERMS, grad_depth=d["grad_depth"])
    without = DR.evaluate(d, stops, on=R.TERMS)[0]
    got = DR.term(fwd, d["grad_depth"]).numpy()
    want = with_depth["grad_h0"] - without["grad_h0"]
    scale = max(np.abs(with_depth["grad_h0"]).max(), 1e-300)
    assert np.abs(got - want).max() <= 1e-11 * scale
    assert np.array_equal(with_depth["grad_c"], without["grad_c"]), "t, near and far carry no gradient: grad_c takes nothing"
    out = ~L["fits"]
    assert not with_depth["depth_raw"][out].any()


_FP32 = {}


def _fp32(d):
    """The fp32 evaluation of a case without the depth term (values) and its forward, once per case."""
    if d["name"] not in _FP32:
        vals, _, fwd = DR.evaluate(d, None, on=R.TERMS, dtype=torch.float32)
        _FP32[d["name"]] = vals, fwd
    return _FP32[d["name"]]


_WANT = {}


def _ratio(d, mutant=None):
    cands, L = _candidates(d)
    vals, fwd = _fp32(d)
    got = dict(vals, grad_h0=vals["grad_h0"] + DR.term(fwd, d["grad_depth"], mutant=mutant).to(torch.float64).numpy())

    def want(stops):
        key = (d["name"], tuple(int(x) for x in stops))
        if key not in _WANT:
            _WANT[key] = DR.evaluate(d, stops, on=R.TERMS, grad_depth=d["grad_depth"], mags=True)[:2]
        return _WANT[key]
    best, _, per = R.match(cands, want, got, L, half=())
    return float(best.max()), per


def test_fp32_evaluation_stays_within_the_bound_and_every_mutant_leaves_it():
    worst, per_all = 0.0, {}
    for d in CASES:
        r, per = _ratio(d)
        assert r <= C, (d["name"], per)
        worst = max(worst, r)
        for k, v in per.items():
            per_all[k] = max(per_all.get(k, 0.0), v)
    print("fp32 closed form, worst ratios", per_all)
    for mutant in DR.MUTANTS:
        rs = [_ratio(d, mutant)[0] for d in CASES]
        print(mutant, "worst case", max(rs), "cases above C", sum(r > C for r in rs))
        assert max(rs) > C, (mutant, rs)


ONE = ctypes.c_void_p(64)


def test_entry_points_refuse_inconsistent_pointer_sets():
    """Before any launch: ray_dist without ray_wm, grad_dist without the forward's totals, grad_depth without depth_raw / nears / fars, a
    c_width other than 4 or 16."""
    from focnerf_amd._lib import lib
    err = lib.foc_last_error
    of = (ONE, ONE, 4, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, ONE, ONE, ONE, ONE, None)
    for rd, wm in ((None, ONE), (ONE, None)):
        assert lib.foc_occ_tail_forward_depth(*of, rd, wm, ONE, None) != 0 and b"occ_tail_forward_depth: ray_dist and ray_wm come together" in err()
    assert lib.foc_occ_tail_forward_depth(*of[:2], 8, *of[3:], None, None, ONE, None) != 0 and b"occ_tail_forward_depth: c_width" in err()
    ob = (ONE, None, ONE, ONE, 4, ONE, ONE, ONE, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, None)
    for wm, rd in ((None, ONE), (ONE, None)):
        assert lib.foc_occ_tail_backward_depth(*ob, wm, rd, ONE, None, None, None, None, None) != 0
        assert b"occ_tail_backward_depth: grad_dist needs ray_wm and ray_dist" in err()
    for nr, fr, raw in ((None, ONE, ONE), (ONE, None, ONE), (ONE, ONE, None)):
        assert lib.foc_occ_tail_backward_depth(*ob, None, None, None, nr, fr, raw, ONE, None) != 0
        assert b"occ_tail_backward_depth: grad_depth needs depth_raw, nears and fars" in err()
    assert lib.foc_occ_tail_backward_depth(*ob[:4], 8, *ob[5:], None, None, None, ONE, ONE, ONE, ONE, None) != 0 and b"occ_tail_backward_depth: c_width" in err()


def test_tail_struct_matches_the_header_and_is_validated_on_the_host():
    """include/focnerf.h `FocOccTrainTail` (its layout against gcc's: tests/test_abi.py test_struct_layout_matches_the_header): the field
    names and order; a NULL tail, a wrong struct_bytes and inconsistent pointer sets are refused before any launch, for the plain and the
    object layout."""
    from focnerf_amd import _lib
    assert [f[0] for f in _lib.FocOccTrainTail._fields_] == ["struct_bytes", "ray_dist", "ray_wm", "depth_raw", "grad_dist", "grad_depth"]
    lib = _lib.lib
    node = _lib.FocOccTrainNode()
    node.struct_bytes, node.cap, node.n_rays = ctypes.sizeof(_lib.FocOccTrainNode), 128, 4
    node.grid_workspace, node.grid_workspace_bytes, node.offsets_host = 64, 64, 64
    node.sigma_layers, node.color_layers = 2, 3
    nd = ctypes.byref(node)
    for fn in (lib.foc_occ_train_forward_tail, lib.foc_occ_train_backward_tail):
        assert fn(None, None, 0.0, None, None) == 1 and b"null node" in lib.foc_last_error()
        assert fn(nd, None, 0.0, None, None) == 1 and b"null tail" in lib.foc_last_error()
        tail = _lib.FocOccTrainTail()
        tail.struct_bytes = ctypes.sizeof(_lib.FocOccTrainTail) - 8
        assert fn(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"FocOccTrainTail has" in lib.foc_last_error()
        tail.struct_bytes = ctypes.sizeof(_lib.FocOccTrainTail)
        tail.ray_dist = 64
        assert fn(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"ray_dist and ray_wm come together" in lib.foc_last_error()
        tail.ray_dist, tail.ray_wm = None, 64
        assert fn(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"ray_dist and ray_wm come together" in lib.foc_last_error()
        ob = _lib.FocOccTrainObject()
        ob.struct_bytes = ctypes.sizeof(_lib.FocOccTrainObject) - 8
        assert fn(nd, ctypes.byref(ob), 0.0, ctypes.byref(tail), None) == 1 and b"FocOccTrainObject has" in lib.foc_last_error()
    node.sigma_layers = 3                                             # (3, 2): no layer pair a pad is built for
    node.color_layers = 2
    tail = _lib.FocOccTrainTail()
    tail.struct_bytes = ctypes.sizeof(_lib.FocOccTrainTail)
    assert lib.foc_occ_train_forward_tail(nd, None, 1.0, ctypes.byref(tail), None) == 1 and b"a pad needs" in lib.foc_last_error()
    node.sigma_layers, node.color_layers = 2, 3
    tail.grad_dist = 64
    assert lib.foc_occ_train_backward_tail(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"grad_dist needs ray_wm and ray_dist" in lib.foc_last_error()
    tail.grad_dist, tail.grad_depth = None, 64
    assert lib.foc_occ_train_backward_tail(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"grad_depth needs depth_raw, nears and fars" in lib.foc_last_error()
    tail.depth_raw = 64                                               # the node's nears / fars are NULL
    assert lib.foc_occ_train_backward_tail(nd, None, 0.0, ctypes.byref(tail), None) == 1 and b"grad_depth needs depth_raw, nears and fars" in lib.foc_last_error()
