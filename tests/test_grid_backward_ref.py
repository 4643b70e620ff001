"""CPU: the float64 reference of the hash-grid backward (tests/grid_backward_ref.py) pinned to the C oracle and to torch autograd, the
input condition and the properties its cases promise asserted on the reference alone, and the per-element bound exercised on the numpy
model of every route: the unmutated model stays inside it on every case and route of the plan, every mutant leaves it on the case named
in CAUGHT_BY.

The GPU comparison is tests/test_gpu_grid_backward_reference.py; it walks the same cases and routes (grid_backward_ref.PLAN)."""
import numpy as np
import pytest
import torch

import grid_backward_ref as G
import oracle

# mutant -> (case, route) on which the bound notices it (worst |model - reference| / bound there, measured: NOTEBOOK.md)
CAUGHT_BY = {
    "drop_run_tail": ("runs_3051", "binned16"),
    "run_ignores_group_edge": ("runs_3051", "binned16"),
    "zero_grad_tail_skips_run": ("runs_3051", "binned16"),
    "subnormal_flush": ("edges_2^-14", "binned16_unfactored"),
    "neg_fract_carry": ("edges_2^-20", "binned16"),
    "fx_14_bits": ("edges_2^10", "binned16"),
    "pair_straddle_lost": ("straddle", "binned16"),
    "chunk_off_by_one": ("chunks_8193", "binned16"),
    "odd_x_pair_twice": ("edges_2^0", "binned16"),
    "round_per_addend": ("runs_3051", "binned16_12byte"),
    "oob_counts": ("edges_2^0", "binned16"),
}


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; an element with bound 0 (untouched) must be exactly 0."""
    got = got.astype(np.float64)
    err = np.abs(got - ref)
    assert np.all(got[bound == 0] == 0), "untouched rows are exactly zero"
    sel = bound > 0
    return float((err[sel] / bound[sel]).max()) if sel.any() else 0.0


def _oracle_backward(case, dtype, grad=None, dy=None):
    D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
    g = (case["grad"] if grad is None else grad).astype(dtype)
    return oracle.grid_encode_backward(g, case["x"], case["off"], int(case["off"][-1]), D, C, L, case["S"], H, dy, gridtype, ac, interp)


@pytest.mark.parametrize("name", G.names())
def test_input_condition_and_oracle_pin(name):
    case = G.case(name)
    assert G.near_integer(case) == 0, "a position within 2^-18 of a cell boundary"
    ref = G.reference(case)
    # the rows a unit gradient reaches are exactly the oracle's: the rows of the corners whose fp32 weight is not 0 (a point on a cell
    # boundary, x = 0 or 1, has corners of weight 0: touched, and the reference's float64 weight there is within the bound of 0)
    ones = dict(case, grad=np.ones_like(case["grad"]), _ref=None, _bound={})
    reached = _oracle_backward(ones, np.float32) != 0
    assert np.array_equal(reached, G.model(ones, "atomic32") != 0)
    assert not (reached.any(axis=1) & ~ref["touched"]).any()
    inb = np.all((case["x"] >= 0) & (case["x"] <= 1), axis=1)
    assert ref["outside"] == case["L"] * int((~inb).sum())
    assert ref["count"].sum() == case["C"] * case["L"] * int(inb.sum()) * 2 ** case["D"]
    if name == "overflow":
        return                                              # totals beyond half: the GPU test and test_overflow_case below
    for dtype, rname in ((np.float32, "single32"), (np.float16, "single16")):
        got = _oracle_backward(case, dtype)
        r = worst_ratio(got, ref["ge"], G.bound(case, rname))
        print(f"{name}: oracle {dtype.__name__} worst error / bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("name", ["shape_D2_C2", "shape_ac_smooth", "shape_D5"])
def test_grad_inputs_and_small_dimensions_against_autograd(name):
    """A float64 torch restatement of the forward (cells and rows from the reference, everything else differentiable) -> autograd's
    gradients of sum(grad * out) with respect to the table and the points."""
    case = G.case(name)
    D, C, L, B = case["D"], case["C"], case["L"], case["B"]
    table = torch.tensor(case["table"].astype(np.float64), requires_grad=True)
    x = torch.tensor(case["x"].astype(np.float64), requires_grad=True)
    k = np.arange(1 << D)
    loss = 0
    for l in range(L):
        lv = G.level(case, l)
        idx = torch.from_numpy(lv["idx"])
        pos = x[idx] * float(lv["scale"]) + (0.0 if case["ac"] else 0.5)
        f = pos - torch.from_numpy(lv["cell"].astype(np.float64))
        if case["interp"] == 1:
            f = f * f * (3 - 2 * f)
        w = torch.ones(idx.numel(), 1 << D, dtype=torch.float64)
        for d in range(D):
            bit = torch.from_numpy(((k >> d) & 1).astype(bool))[None]
            w = w * torch.where(bit, f[:, d:d + 1], 1 - f[:, d:d + 1])
        vals = table[torch.from_numpy(lv["rows"] + int(case["off"][l]))]
        out = (w[:, :, None] * vals).sum(1)
        loss = loss + (out * torch.from_numpy(case["grad"][l][lv["idx"]].astype(np.float64))).sum()
    gt, gx = torch.autograd.grad(loss, (table, x))
    ref = G.reference(case)
    assert np.abs(gt.numpy() - ref["ge"]).max() <= 1e-12 * max(1.0, ref["mag"].max())
    out64, dy64 = G.forward64(case, case["table"])
    gi, _ = G.grad_inputs(case, dy64, half=False)
    assert np.abs(gx.numpy() - gi).max() <= 1e-10 * max(1.0, np.abs(gi).max())
    # and the oracle's grad_inputs from its own half dy_dx lies inside the bound of the reference taken at that dy_dx
    Dn, Cn, Ln, H, _, _, gridtype, ac, interp = case["spec"]
    out_o, dy_o = oracle.grid_encode_forward(case["x"], case["table"], case["off"], Dn, Cn, Ln, case["S"], H, True, gridtype, ac, interp, acc_mode=1)
    _, gi_o = _oracle_backward(case, np.float16, dy=dy_o)
    gi_ref, gi_b = G.grad_inputs(case, dy_o, half=True)
    assert np.all(np.abs(gi_o.astype(np.float64) - gi_ref) <= gi_b)
    # the oracle's forward lies inside the forward reference's per-element bound (grid_forward_ref: the float64 forward at the fp32 fraction)
    import grid_forward_ref as F
    fref = F.reference(case, case["table"])
    assert np.all(np.abs(out_o.astype(np.float64) - fref["out"]) <= fref["out_b"]) and np.all(np.abs(dy_o.astype(np.float64) - fref["dy"]) <= fref["dy_b"])
    assert (fref["out_b"] > 0).mean() > 0.9


def test_case_properties():
    """What the cases promise, from the reference alone."""
    for s in (0, -14, -20, 10):
        c = G.case(f"edges_2^{s}")
        x, g = c["x"], c["grad"]
        assert np.all(x[0] == 0) and np.all(x[1] == 1) and np.all(x[2] == np.float32(1) - np.float32(2.0 ** -24))
        assert (x < 0).any() and (x > 1).any()
        plain = np.setdiff1d(np.arange(c["B"]), c["fx_points"])                  # the fx points carry gradients of their own
        assert np.all(g[:, plain[plain % 7 == 0]] == 0) and np.signbit(g[:, plain[plain % 7 == 3], 0]).all() and (g > 0).any() and (g < 0).any()
        prod = np.concatenate([np.abs(G._emit64(c, l, G.ROUTES["atomic16"])["a"]).reshape(-1) for l in range(16)])
        prod = prod[prod > 0]
        if s == -14:
            assert (prod < 2.0 ** -14).mean() >= 0.9, "share of subnormal products"
        if s == -20:
            assert (prod < 2.0 ** -25).mean() >= 0.5, "most products below the half quantum"
        modes = [G._level_mode(c, G.level(c, l), G.ROUTES["binned16"]) for l in range(16)]
        assert modes == ["run"] * 11 + ["fact"] * 5
    c = G.case("cancel")
    n = c["B"] // 2
    assert np.array_equal(c["x"][:n], c["x"][n:]) and np.array_equal(c["grad"][:, :n], -c["grad"][:, n:])
    ref = G.reference(c)
    assert np.all(np.abs(ref["ge"]) <= 1e-15 * ref["mag"]) and ref["mag"].max() > 0.1
    # runs: same-cell stretches of every length 1 .. 17, runs starting at every lane, zero / out-of-range samples at head, inside and tail
    c = G.case("runs_3051")
    lengths, lanes = set(), set()
    zero = np.all(c["grad"][0] == 0, axis=1)
    at = dict(head=0, inside=0, tail=0)
    for l in range(11):
        lv = G.level(c, l)
        head, tail = G._run_heads(c, lv, ignore_group_edge=True)
        starts = np.nonzero(head & lv["inside"])[0]
        ends = np.nonzero(tail)[0]
        lengths |= set((ends - starts + 1).tolist())
        h16, t16 = G._run_heads(c, lv)
        lanes |= set((np.nonzero(h16 & lv["inside"])[0] & 15).tolist())
        s16, e16 = np.nonzero(h16 & lv["inside"])[0], np.nonzero(t16)[0]
        long = e16 - s16 >= 2
        at["head"] += int(zero[s16[long]].sum()); at["tail"] += int(zero[e16[long]].sum())
        at["inside"] += int(sum(zero[a + 1:b].any() for a, b in zip(s16[long], e16[long])))
    assert set(range(1, 18)) <= lengths, sorted(set(range(1, 18)) - lengths)
    assert lanes == set(range(16))
    assert min(at.values()) >= 3, at
    out = ~G.level(c, 0)["inside"]
    assert out[48] and out[63] and out[33:37].all() and out.sum() >= 30
    assert [G.case(n)["B"] for n in G.names("runs")] == [1, 15, 17, 1023, 1025, 3051]
    # chunks of the level-0 slot: 4 records per in-range point
    for B, recs, chunks in ((8192, 32768, 1), (8193, 32772, 2), (20000, 80000, 3)):
        c = G.case(f"chunks_{B}")
        for rname in ("binned16", "binned32"):
            rec = G.slot_records(c, G.ROUTES[rname])
            assert rec[0, 0] == recs and rec[0, 1:].sum() == 0 and -(-rec[0, 0] // G.CHUNK) == chunks
    c = G.case("straddle")
    lv = G.level(c, c["straddle_level"])
    assert not lv["hashed"] and lv["size"] > G.SEG
    assert G._emit64(c, c["straddle_level"], G.ROUTES["binned16"])["straddles"] >= 100
    # single-chunk slots wherever the plan relies on them
    for name in ("overflow", "cancel", "edges_2^0"):
        assert G.slot_records(G.case(name), G.ROUTES["binned16_12byte"]).max() <= G.CHUNK
    assert sorted(G.PLAN) == sorted(G.BUILDERS)


def test_overflow_case():
    c = G.case("overflow")
    ref = G.reference(c)
    for rname in G.PLAN["overflow"]:
        b = G.bound(c, rname)
        must_overflow = np.abs(ref["ge"]) > 65520 + b
        must_hold = (ref["mag"] < G.HALF_MAX - b) & (ref["count"] > 0)
        assert must_overflow.sum() >= 20 and must_hold.sum() >= 20 and ((ref["count"] > 0) & ~must_overflow & ~must_hold).sum() >= 20
        got = G.model(c, rname).astype(np.float64)
        assert not np.isfinite(got[must_overflow]).any()
        assert np.isfinite(got[must_hold]).all() and np.all(np.abs(got - ref["ge"])[must_hold] <= b[must_hold])
        assert np.all(got[ref["count"] == 0] == 0)


@pytest.mark.parametrize("name", [n for n in G.PLAN if n != "overflow"])
def test_model_stays_inside_the_bound(name):
    case = G.case(name)
    ref = G.reference(case)
    for rname in G.PLAN[name]:
        got = G.model(case, rname)
        r = worst_ratio(got, ref["ge"], G.bound(case, rname))
        print(f"{name} / {rname}: model worst error / bound {r:.3f}")
        assert r <= 1.0, (name, rname, r)
        if name == "cancel" and rname == "binned16_12byte":
            assert np.all(got == 0), "exact cancellation on the two-corner records without merging"


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    name, rname = CAUGHT_BY[mutant]
    case = G.case(name)
    got = G.model(case, rname, mutant).astype(np.float64)
    ref, b = G.reference(case)["ge"], G.bound(case, rname)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, np.abs(got - ref) / b, np.where(got == 0, 0.0, np.inf))
    print(f"{mutant}: {name} / {rname}: worst error / bound {ratio.max():.3g} on {(ratio > 1).sum()} elements")
    assert ratio.max() > 1.0
    assert set(CAUGHT_BY) == set(G.MUTANTS)
