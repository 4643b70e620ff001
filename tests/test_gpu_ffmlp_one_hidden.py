"""GPU parity: the fused MLP with ONE hidden layer (num_layers = 1: input -> hidden -> 16 outputs, two matmuls; tcnn's FullyFusedMLP
with n_hidden_layers 1) against the unchanged CPU oracle, which loops over any layer count.

Method of tests/test_gpu_ffmlp.py: on small-integer data every product and partial sum is exact in fp32, so every summation order rounds
to the same fp16 and the comparison is bit-exact; on random data the bounds of that file apply. Every width pair the kernels take at
hidden 16 / 32 / 64 / 128 is covered, through the three backward forms: the single-pass kernel re-evaluating the activations
(FOC_MLP_RECOMPUTE, default), the single-pass kernel on stored activations (FOC_MLP_RECOMPUTE=0) and the two-kernel form (library option
FOC_MLP_BWD_FUSED=0; wide inputs and hidden 128 take it in every mode)."""
import math

import numpy as np
import pytest
import torch

import oracle
from util import assert_half_close, to_np

pytestmark = pytest.mark.gpu

HIDDEN = (16, 32, 64, 128)
INPUTS = (16, 32, 48, 64, 144)
MODES = ("recompute", "stored", "two_kernel")


def _n_params(I, Hd):
    return Hd * (I + 16)


def _mode(mode, monkeypatch, lib_option):
    monkeypatch.setenv("FOC_MLP_RECOMPUTE", "0" if mode == "stored" else "1")
    lib_option("FOC_MLP_BWD_FUSED", 0 if mode == "two_kernel" else 1)


def _integer_data(I, Hd, B, seed):
    rng = np.random.default_rng(seed)
    W = np.zeros(_n_params(I, Hd), np.float16)
    nz = rng.random(W.size) < (4.0 / max(I, Hd))
    W[nz] = rng.integers(-2, 3, nz.sum()).astype(np.float16)
    x = rng.integers(-3, 4, (B, I)).astype(np.float16)
    g = np.zeros((B, 16), np.float16)
    gz = rng.random(g.shape) < 0.25
    g[gz] = rng.integers(-2, 3, gz.sum()).astype(np.float16)
    return x, W, g


def _random_data(I, Hd, B, seed):
    rng = np.random.default_rng(seed)
    W = (rng.uniform(-1, 1, _n_params(I, Hd)) * math.sqrt(3 / Hd)).astype(np.float16)
    x = rng.standard_normal((B, I)).astype(np.float16)
    g = (rng.standard_normal((B, 16)) * 0.05).astype(np.float16)
    return x, W, g


def _run(x, W, g, I, Hd, act):
    """Through the autograd op the modules use (focnerf_amd.ffmlp.FusedMLP): training forward + backward, then the inference forward."""
    from focnerf_amd.ffmlp import ffmlp_forward
    xt = torch.from_numpy(x).cuda().requires_grad_(True)
    Wt = torch.from_numpy(W).cuda().requires_grad_(True)
    y = ffmlp_forward(xt, Wt, I, 16, Hd, 1, act, 6, False, True)
    y.backward(torch.from_numpy(g).cuda())
    with torch.no_grad():
        yi = ffmlp_forward(xt.detach(), Wt.detach(), I, 16, Hd, 1, act, 6, True, False)
    torch.cuda.synchronize()
    return to_np(y), to_np(yi), to_np(xt.grad), to_np(Wt.grad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [1, 127, 4097])
@pytest.mark.parametrize("Hd", HIDDEN)
@pytest.mark.parametrize("I", INPUTS)
def test_one_hidden_layer_exact_on_integer_data(I, Hd, B, mode, monkeypatch, lib_option):
    _mode(mode, monkeypatch, lib_option)
    for act in (0, 6):
        x, W, g = _integer_data(I, Hd, B, I * 1000 + Hd * 10 + B + act)
        ref_out, ref_fb = oracle.ffmlp_forward(x, W, I, Hd, 1, act)
        gw_r, gi_r, _ = oracle.ffmlp_backward(g, x, W, ref_fb, I, Hd, 1, act, True)
        assert np.abs(ref_out.astype(np.float32)).max() < 30000 and np.abs(gw_r.astype(np.float32)).max() < 30000
        if B > 1000:
            assert np.count_nonzero(ref_out) > 100 and np.count_nonzero(gw_r) > 50, "degenerate test data"
        first = _run(x, W, g, I, Hd, act)
        out, out_inf, gi, gw = first
        assert np.array_equal(out, ref_out), f"training forward, act {act}"
        assert np.array_equal(out_inf, ref_out), f"inference forward, act {act}"
        assert np.array_equal(gi, gi_r), f"grad_inputs, act {act}"
        assert np.array_equal(gw, gw_r), f"grad_weights, act {act}"
        again = _run(x, W, g, I, Hd, act)
        assert all(np.array_equal(a.view(np.uint16), b.view(np.uint16)) for a, b in zip(first, again)), "not deterministic"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B", [127, 4097])
@pytest.mark.parametrize("Hd", HIDDEN)
@pytest.mark.parametrize("I", INPUTS)
def test_one_hidden_layer_random(I, Hd, B, mode, monkeypatch, lib_option):
    _mode(mode, monkeypatch, lib_option)
    x, W, g = _random_data(I, Hd, B, 7 + I + Hd + B)
    ref_out, ref_fb = oracle.ffmlp_forward(x, W, I, Hd, 1, 0)
    out, out_inf, gi, gw = _run(x, W, g, I, Hd, 0)
    assert_half_close(out, ref_out, ulps=4.0, atol=4e-3, what="outputs")
    assert np.array_equal(out_inf, out), "inference and training kernels must agree bit for bit"
    # the oracle's backward on the kernel's own forward activations (the re-evaluating backward computes the same bits), as
    # tests/test_gpu_ffmlp.py::test_backward_random: a ReLU mask that a summation-order difference flips at 0 is not a finding
    from focnerf_amd.backend import _ffmlp as be
    fb = torch.empty(1, B, Hd, dtype=torch.float16, device="cuda")
    be.ffmlp_forward(torch.from_numpy(x).cuda(), torch.from_numpy(W).cuda(), B, I, 16, Hd, 1, 0, 6, fb, torch.empty(B, 16, dtype=torch.float16, device="cuda"))
    assert_half_close(to_np(fb), ref_fb, ulps=2.0, atol=2e-3, what="forward_buffer")
    gw_r, gi_r, _ = oracle.ffmlp_backward(g, x, W, to_np(fb), I, Hd, 1, 0, True)
    assert_half_close(gi, gi_r, ulps=4.0, atol=5e-4, what="grad_inputs")
    assert_half_close(gw, gw_r, ulps=4.0, atol=2e-3 * max(1.0, B / 1024), what="grad_weights")


def test_backend_buffers_at_one_hidden_layer():
    """The ABI's kept buffers at num_layers = 1: forward_buffer [1, B, hidden] (the post-activation) and, on the two-kernel form,
    backward_buffer [1, B, hidden] (the masked delta) equal the oracle's."""
    from focnerf_amd.backend import _ffmlp as be
    for I, Hd in [(32, 64), (144, 16), (48, 128)]:
        B = 1000
        x, W, g = _integer_data(I, Hd, B, I + Hd)
        ref_out, ref_fb = oracle.ffmlp_forward(x, W, I, Hd, 1, 0)
        gw_r, gi_r, bb_r = oracle.ffmlp_backward(g, x, W, ref_fb, I, Hd, 1, 0, True)
        t = lambda a: torch.from_numpy(a).cuda()
        out = torch.empty(B, 16, dtype=torch.float16, device="cuda")
        fb = torch.empty(1, B, Hd, dtype=torch.float16, device="cuda")
        be.ffmlp_forward(t(x), t(W), B, I, 16, Hd, 1, 0, 6, fb, out)
        assert np.array_equal(to_np(fb), ref_fb) and np.array_equal(to_np(out), ref_out)
        bb = torch.empty(1, B, Hd, dtype=torch.float16, device="cuda")
        gi = torch.empty(B, I, dtype=torch.float16, device="cuda")
        gw = torch.empty(W.size, dtype=torch.float16, device="cuda")
        be.ffmlp_backward(t(g), t(x), t(W), fb, B, I, 16, Hd, 1, 0, 6, True, bb, gi, gw)
        assert np.array_equal(to_np(bb), bb_r) and np.array_equal(to_np(gi), gi_r) and np.array_equal(to_np(gw), gw_r)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("I,Hd", [(32, 64), (48, 64), (144, 16)])
def test_one_hidden_layer_at_2m_rows(I, Hd, mode, monkeypatch, lib_option):
    """B = 2 097 152 (4096 rays x 512 samples) on integer data. Rows are independent: the outputs and input gradients of a row subset equal
    the oracle's on that subset, bit for bit. The weight gradient sums over all rows; its exact value is the fp64 chain on the GPU (every
    intermediate is an integer below 2^24, so fp64 and the kernels' fp32 sums are exact and round to the same fp16)."""
    _mode(mode, monkeypatch, lib_option)
    B = 4096 * 512
    rng = np.random.default_rng(I + Hd)
    x, W, _ = _integer_data(I, Hd, 64, I * 3 + Hd)
    xt = torch.randint(-3, 4, (B, I), device="cuda").half()
    gt = torch.zeros(B, 16, device="cuda")
    live = torch.rand(B, device="cuda") < 0.002                     # sparse output gradients keep the batch sums far below 2^24
    gt[live] = torch.randint(-2, 3, (int(live.sum()), 16), device="cuda").float()
    gt = gt.half()
    res = []
    for _ in range(2):
        from focnerf_amd.ffmlp import ffmlp_forward
        xr = xt.clone().requires_grad_(True)
        Wt = torch.from_numpy(W).cuda().requires_grad_(True)
        y = ffmlp_forward(xr, Wt, I, 16, Hd, 1, 0, 6, False, True)
        y.backward(gt)
        torch.cuda.synchronize()
        res.append((y.detach(), xr.grad, Wt.grad))
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(*res)), "not deterministic"
    y, gx, gw = res[0]
    sel = torch.from_numpy(rng.choice(B, 2048, replace=False)).cuda()
    sel = torch.cat([sel, torch.nonzero(live)[:256, 0], torch.tensor([0, 31, 32, B - 1], device="cuda")])
    xs, gs = to_np(xt[sel]), to_np(gt[sel])
    ref_out, ref_fb = oracle.ffmlp_forward(xs, W, I, Hd, 1, 0)
    _, gi_r, _ = oracle.ffmlp_backward(gs, xs, W, ref_fb, I, Hd, 1, 0, True)
    assert np.array_equal(to_np(y[sel]), ref_out)
    assert np.array_equal(to_np(gx[sel]), gi_r)
    W0 = torch.from_numpy(W[:Hd * I].astype(np.float64).reshape(Hd, I)).cuda()
    W1 = torch.from_numpy(W[Hd * I:].astype(np.float64).reshape(16, Hd)).cuda()
    h = torch.relu(xt.double() @ W0.T)
    assert float(h.abs().max()) < 2048 and float((h @ W1.T).abs().max()) < 2048
    d = (gt.double() @ W1) * (h > 0)
    want = torch.cat([(d.T @ xt.double()).reshape(-1), (gt.double().T @ h).reshape(-1)])
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(gw, want.half()), "grad_weights over 2 M rows"
