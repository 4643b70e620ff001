"""CPU: the float64 reference of the fused MLP (tests/mlp_ref.py) pinned to the C oracle and to float64 autograd, the properties its
cases promise asserted on the data alone, the per-element bound exercised on numpy fp32 models of the weight-gradient routes' summation
orders at all four gradient scales, every mutant of mlp_ref.MUTANTS outside the bound on the case named in CAUGHT_BY, and the plan
covering every row of the route table.

The GPU comparison is tests/test_gpu_mlp_reference.py; it walks the same cases and routes (mlp_ref.PLAN)."""
import numpy as np
import pytest
import torch

import mlp_ref as M
import oracle


def _ratio(got, q):
    """max |got - ref| / bound without asserting (bound-0 elements that are not 0 count as inf)."""
    got = np.asarray(got).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(q["bound"] > 0, np.abs(got - q["ref"]) / q["bound"], np.where(got == 0, 0.0, np.inf))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


def _oracle_run(c, act):
    out, fb = oracle.ffmlp_forward(c["x"], c["W"], c["I"], c["H"], c["nl"], act)
    gw, gi, bb = oracle.ffmlp_backward(c["grad"], c["x"], c["W"], fb, c["I"], c["H"], c["nl"], act, True)
    return out, fb, gw, gi, bb


_SHAPE_CASES = [f"shape_{M.shape_name(*s)}_B333" for s in M.SHAPES]


@pytest.mark.parametrize("name", _SHAPE_CASES + M.names("scale") + M.names("cancel"))
@pytest.mark.parametrize("act", [M.RELU, M.NONE])
def test_reference_pinned_to_the_oracle(name, act):
    """mlp_ref on the oracle's own fb / bb reproduces the oracle within the bound: a k-ordered fmaf chain is one of the orders it covers."""
    c = M.case(name)
    nl = c["nl"]
    Ws = M.split(c["W"], c["I"], c["H"], nl)
    out, fb, gw, gi, bb = _oracle_run(c, act)
    worst = {}
    worst["fb"] = max(M.worst_ratio(fb[l], M.forward_layer(l, c["x"], fb, Ws, act), f"fb[{l}]") for l in range(nl))
    worst["out"] = M.worst_ratio(out, M.output(fb, Ws), "out")
    worst["bb"] = max(M.worst_ratio(bb[k], M.delta(k, c["grad"], fb, bb, Ws, act), f"bb[{k}]") for k in range(nl))
    worst["grad_inputs"] = M.worst_ratio(gi, M.grad_inputs(bb, Ws), "grad_inputs")
    worst["grad_weights"] = M.worst_ratio(gw, M.grad_weights(c["x"], fb, bb, c["grad"], nl), "grad_weights")
    print(f"\n{name} act {act}: oracle worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("I,H,nl", [(32, 64, 2), (48, 32, 4), (64, 64, 1)])
@pytest.mark.parametrize("act", [M.RELU, M.NONE])
def test_reference_pinned_to_float64_autograd(I, H, nl, act):
    """An unrounded float64 torch MLP: autograd's dW and dX equal the formulas on ITS activations and deltas to 1e-12 (the deltas are fed in,
    nothing propagates), and each delta equals the formula on the delta before it."""
    rng = np.random.default_rng(I + H + nl)
    B = 77
    W = rng.uniform(-1, 1, M.n_params(I, H, nl)) * np.sqrt(3 / H)
    Wt = [torch.tensor(w, requires_grad=True) for w in M.split(W, I, H, nl)]
    x = torch.tensor(rng.standard_normal((B, I)), requires_grad=True)
    g = rng.standard_normal((B, 16))
    h, pre, post = x, [], []
    for l in range(nl):
        s = h @ Wt[l].T
        s.retain_grad()
        pre.append(s)
        h = torch.relu(s) if act == M.RELU else s
        post.append(h)
    out = h @ Wt[nl].T
    (out * torch.tensor(g)).sum().backward()
    fb = np.stack([p.detach().numpy() for p in post])
    bb = np.stack([pre[nl - 1 - k].grad.numpy() for k in range(nl)])         # bb[k] is the delta of forward layer nl - 1 - k
    Ws = [w.detach().numpy() for w in Wt]
    xs = x.detach().numpy()
    tol = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    for l in range(nl):
        assert tol(M.forward_layer(l, xs, fb, Ws, act)["ref"], fb[l])
    assert tol(M.output(fb, Ws)["ref"], out.detach().numpy())
    for k in range(nl):
        assert tol(M.delta(k, g, fb, bb, Ws, act)["ref"], bb[k])
    assert tol(M.grad_inputs(bb, Ws)["ref"], x.grad.numpy())
    assert tol(M.grad_weights(xs, fb, bb, g, nl)["ref"], np.concatenate([w.grad.numpy().reshape(-1) for w in Wt]))


def _dw_operand_sets(c, act):
    """[(j, D, A)] of every blob matrix from the oracle's buffers."""
    out, fb, gw, gi, bb = _oracle_run(c, act)
    return [(j,) + tuple(np.asarray(a) for a in M.dw_operands(j, c["x"], fb, bb, c["grad"], c["nl"])) for j in range(c["nl"] + 1)]


@pytest.mark.parametrize("name", M.names("scale_32x64x2") + ["cancel_32x64x2", "shape_32x64x2_B1000", "shape_48x32x4_B333", "shape_16x16x2_B129"])
@pytest.mark.parametrize("order", M.ORDERS)
def test_summation_orders_stay_within_the_bound(name, order):
    """numpy fp32 emulations of the routes' orders (128-row partials then the 16-way and serial slot sums; 64-row chunks in a shuffled
    order; 32 images in order) at the four gradient scales, under cancellation and at the largest batch."""
    c = M.case(name)
    worst = 0.0
    for j, D, A in _dw_operand_sets(c, M.RELU):
        q = M.product(D.T, A.T)
        got = M.model_dw(D, A, order, seed=j)
        assert got.dtype == np.float16
        worst = max(worst, M.worst_ratio(got, q, f"{name} dW_{j} {order}"))
    print(f"\n{name} / {order}: worst error / bound {worst:.3f}")


def _sparse_rows_case(B, n_rows, seed):
    """D [B, 64], A [B, 64] with n_rows evenly spread nonzero rows of D: the loop-edge cases' shape of data."""
    rng = np.random.default_rng(seed)
    D = np.zeros((B, 64), np.float16)
    rows = np.linspace(0, B - 1, n_rows).astype(np.int64)
    D[rows] = (rng.standard_normal((n_rows, 64)) * 0.05).astype(np.float16)
    A = np.maximum(rng.standard_normal((B, 64)), 0).astype(np.float16)
    return D, A


# mutant -> the case on which the bound notices it
CAUGHT_BY = {
    "drop_ragged_last_row": "shape_32x64x2_B333",
    "drop_second_pass": "shape_32x64x2_B333 (two workgroups)",
    "slot0_twice": "shape_32x64x2_B333",
    "skip_slots_from_512": "600 nonzero rows in 600 groups",
    "delta_before_mask": "scale_32x64x2_2^0",
    "flush_subnormal_delta": "scale_32x64x2_2^-16",
    "truncate_final": "shape_32x64x2_B333",
    "fb_l_for_fb_l_minus_1": "shape_32x64x3_B333",
}


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    assert set(CAUGHT_BY) == set(M.MUTANTS)
    if mutant == "skip_slots_from_512":
        D, A = _sparse_rows_case(128 * 600, 600, 7)
        q = M.product(D.T, A.T)
        assert _ratio(M.model_dw(D, A, "slots"), q) <= 1.0
        r = _ratio(M.model_dw(D, A, "slots", mutant), q)
    elif mutant in ("delta_before_mask", "flush_subnormal_delta"):
        c = M.case(CAUGHT_BY[mutant])
        Ws = M.split(c["W"], c["I"], c["H"], c["nl"])
        out, fb, gw, gi, bb = _oracle_run(c, M.RELU)
        r = 0.0
        for k in range(c["nl"]):
            q = M.delta(k, c["grad"], fb, bb, Ws, M.RELU)
            assert _ratio(M.model_delta(k, c["grad"], fb, bb, Ws, M.RELU), q) <= 1.0
            r = max(r, _ratio(M.model_delta(k, c["grad"], fb, bb, Ws, M.RELU, mutant), q))
    elif mutant == "fb_l_for_fb_l_minus_1":
        c = M.case(CAUGHT_BY[mutant])
        out, fb, gw, gi, bb = _oracle_run(c, M.RELU)
        D, A = M.dw_operands(2, c["x"], fb, bb, c["grad"], c["nl"])           # hidden matrix 2: A is fb[1]
        assert A is not None and np.array_equal(A, fb[1])
        q = M.product(np.asarray(D).T, np.asarray(A).T)
        assert _ratio(M.model_dw(D, A, "slots"), q) <= 1.0
        r = _ratio(M.model_dw(D, fb[2], "slots"), q)
    else:
        c = M.case(CAUGHT_BY[mutant].split()[0])
        grid = 2 if mutant == "drop_second_pass" else None
        r = 0.0
        for j, D, A in _dw_operand_sets(c, M.RELU):
            q = M.product(D.T, A.T)
            assert _ratio(M.model_dw(D, A, "slots", grid=grid), q) <= 1.0
            r = max(r, _ratio(M.model_dw(D, A, "slots", mutant, grid=grid), q))
        if mutant == "truncate_final":                                    # and on a row-wise quantity
            Ws = M.split(c["W"], c["I"], c["H"], c["nl"])
            out, fb, gw, gi, bb = _oracle_run(c, M.RELU)
            assert _ratio(M.model_delta(0, c["grad"], fb, bb, Ws, M.RELU, mutant), M.delta(0, c["grad"], fb, bb, Ws, M.RELU)) > 1.0
    print(f"\n{mutant}: worst error / bound {r:.2f} on {CAUGHT_BY[mutant]}")
    assert r > 1.0, f"{mutant} stays within the bound"


def test_dropped_row_share_outside_the_bound():
    """The reason for MAX_NONZERO_ROWS: one row dropped from dW puts nearly every element it touches outside at B <= 1000."""
    for name in ("shape_32x64x2_B333", "shape_32x64x2_B1000"):
        c = M.case(name)
        j, D, A = _dw_operand_sets(c, M.RELU)[1]
        q = M.product(D.T, A.T)
        D2 = D.copy()
        r = c["B"] // 2
        D2[r] = 0
        got = M.model_dw(D2, A, "slots").astype(np.float64)
        touched = np.outer(D[r] != 0, A[r] != 0)
        outside = (np.abs(got - q["ref"]) > q["bound"]) & touched
        share = outside.sum() / max(touched.sum(), 1)
        print(f"\n{name}: {share:.3f} of the {int(touched.sum())} elements a dropped row touches are outside the bound")
        assert share >= 0.9


def test_plan_covers_the_route_table():
    on_plan = {r for n in M.PLAN for r in M.PLAN[n]}
    for row, routes in M.TABLE.items():
        assert set(routes) <= on_plan, f"route table row '{row}' is not on the plan"
    assert set(M.ROUTES) == {r for rs in M.TABLE.values() for r in rs}
    # both activations on the stored and two-kernel routes; every route with and without input gradients, the lean form aside
    for r in ("stored", "two_kernel", "two_kernel_det", "hidden256", "wide_input"):
        assert M.acts_for(r) == (M.RELU, M.NONE)
    for I, H, nl in M.SHAPES:
        for act in (M.RELU, M.NONE):
            rs = M.routes_for(I, H, nl, act)
            assert rs, f"no route serves {I} x {H} x {nl}"
            for r in rs:
                assert M.kernels(r, I, H, nl, act, True) is not None
                assert (M.kernels(r, I, H, nl, act, False) is None) == (r == "lean")
    assert "lean" in M.routes_for(32, 64, 2, M.RELU) and "lean" not in M.routes_for(32, 64, 2, M.NONE)
    assert M.kernels("recompute", 32, 64, 2, M.RELU, True)[0] == "k_mlp_bwd_fused<64, 2, RECOMP=true, IMODE=0, IN32>"
    assert M.kernels("wide_input", 144, 32, 3, M.RELU, True)[1] == "k_mlp_dw<32,256>"
    assert M.kernels("hidden256_det", 32, 256, 2, M.RELU, True) == ("k_wide_layer", "k_mlp_dw<256>", "k_mlp_dw_finalize_slots")
    # the scale, cancellation and non-finite cases run on every route their shapes have
    for n in M.names("scale") + M.names("cancel") + M.names("nonfinite"):
        assert set(M.PLAN[n]) == set(M.routes_for(*M.BUILDERS[n][:3], M.RELU))
    # one hidden layer at every width that has those kernels, and every batch edge on every shape
    assert {H for _, H, nl in M.SHAPES if nl == 1} == {16, 32, 64, 128}
    assert all(f"shape_{M.shape_name(*s)}_B{B}" in M.PLAN for s in M.SHAPES for B in M.BATCHES)


@pytest.mark.parametrize("name", M.names())
def test_case_data_keeps_its_promises(name):
    c = M.case(name)
    B, nl = c["B"], c["nl"]
    assert np.count_nonzero(np.any(c["grad"] != 0, axis=1)) <= M.MAX_NONZERO_ROWS
    for act in (M.RELU, M.NONE):
        out, fb, gw, gi, bb = _oracle_run(c, act)
        fb32 = fb.astype(np.float32)
        assert np.abs(fb32).max() < M.HALF_MAX
        for l in range(nl):
            assert np.count_nonzero(fb32[l]) > 0.2 * fb32[l].size, f"layer {l} is degenerate"
        if c["kind"] == "nonfinite":
            assert np.isinf(c["grad"].astype(np.float32)).sum() == 1 and np.isfinite(c["grad_finite"].astype(np.float32)).all()
            continue
        assert np.isfinite(bb.astype(np.float32)).all(), "every delta is finite"
        for k in range(nl):
            assert np.count_nonzero(bb[k]) > 0.2 * bb[k].size or B == 1, f"delta {k} is degenerate"
        q = M.grad_weights(c["x"], fb, bb, c["grad"], nl)
        if c["kind"] == "overflow":
            assert (np.abs(q["ref"]) > M.HALF_OVER + q["bound"]).sum() >= 16, "elements that must overflow"
            assert ((q["mag"] < M.HALF_MAX - q["bound"]) & (q["count"] > 0)).sum() >= 16, "elements that must hold"
        else:
            assert (np.abs(q["ref"]) + q["bound"]).max() < M.HALF_MAX
        if c["kind"] == "cancel":
            assert np.array_equal(c["x"][:B // 2], c["x"][B // 2:]) and np.array_equal(c["grad"][:B // 2], -c["grad"][B // 2:])
            assert np.abs(q["ref"]).max() <= 1e-3 * q["mag"].max(), "the float64 totals cancel"
        if name.startswith("scale") and c["scale"] == 2.0 ** -16:
            d = np.abs(bb.astype(np.float32))
            assert ((d > 0) & (d < 2.0 ** -14)).sum() > 0.5 * np.count_nonzero(d), "most deltas are subnormal halves"


@pytest.mark.parametrize("kind", M.LOOPS)
@pytest.mark.parametrize("cus", [256, 304, 64])
def test_loop_cases_reach_a_second_pass(kind, cus):
    lc = M.loop_case(kind, cus)
    assert lc["B"] > lc["grid"] * lc["wg_rows"] + lc["wg_rows"], "at least one workgroup meets a second full pass and the tail is ragged"
    assert lc["B"] % lc["wg_rows"] and lc["B"] % 32
    rows = M.loop_rows(lc, np.random.default_rng(1))
    assert rows.size <= 608 and rows[0] == 0 and rows[-1] == lc["B"] - 1 and np.all(np.diff(rows) > 0)
    assert (rows >= lc["grid"] * lc["wg_rows"]).sum() >= 64, "rows of the second pass carry gradients"
    if kind == "fused":
        assert lc["B"] == 128 * min(2 * cus, 1024) + 128 + 17
    if kind == "dw_det":
        assert lc["B"] == 64 * 32 + 65
    if kind == "dw":
        assert lc["B"] == 64 * -(-8 * cus // 3) + 65
    if kind == "bwd":
        assert lc["B"] == 256 * 4 * cus + 256 + 17
    if kind == "forward":
        assert lc["B"] == 128 * 8 * cus + 128 + 17
