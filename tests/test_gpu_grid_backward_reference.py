"""GPU: the hash-grid encoder's backward, every route a call can take, against the float64 reference of tests/grid_backward_ref.py with
its per-element bound (derivation: that module's docstring; the same cases and routes as the numpy model in test_grid_backward_ref.py,
grid_backward_ref.PLAN).

Every element of grad_embeddings (and of grad_inputs where computed) must lie within the bound of its route; rows no in-range point
touches must be exactly zero; both gradient layouts ([L,B,C] and [B, L*C]) run in every test. Each test prints the worst
|kernel - float64| / bound of its case and route (measured on MI355X: NOTEBOOK.md, "Grid backward against float64").

Routes: binned default (fp16), binned fp32, FOC_GB_FACTORED=0, FOC_GB_MERGE_MAX_RES=0, both together (12-byte records, nothing merged),
FOC_DETERMINISTIC 1 and 2, and the scattered-atomic kernel (FOCNERF_GRID_ATOMIC=1) in fp16 and fp32.

Measured on MI355X, worst ratio over every case (asserted <= 1): binned fp16 routes 0.853, binned fp32 0.031, atomic fp16 0.584, atomic
fp32 0.029, grad_inputs 0.986 (half: the output's own rounding is nearly all of its bound) / 0.039 (fp32), the precounted form 0.812;
the cancellation case is exactly 0 on the unmerged 12-byte records and 0.391 on the factored default. Wall time of the file: 31 s for
its 87 tests, 0.3 .. 0.9 s each.
"""
import numpy as np
import pytest
import torch

import grid_backward_ref as G
import oracle
from util import to_np

pytestmark = pytest.mark.gpu

CASES = {n: G.case(n) for n in G.PLAN}
PAIRS = [(n, r) for n in G.PLAN if n != "overflow" for r in G.PLAN[n]]
_DY = {}


def _be():
    from focnerf_amd.backend import _gridencoder
    return _gridencoder


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _select(rname, lib_option, monkeypatch):
    """Put the library and the wrapper on route `rname`; the defaults the reference assumes are asserted, not assumed."""
    from focnerf_amd import _lib
    r = G.ROUTES[rname]
    assert (_lib.get_option("FOC_GB_MERGE_MAX_RES"), _lib.get_option("FOC_GB_FACTORED")) == (G.MERGE_MAX_RES, 1)
    monkeypatch.setenv("FOCNERF_GRID_ATOMIC", "1" if r["kind"] == "atomic" else "0")
    lib_option("FOC_DETERMINISTIC", r["det"])
    if r["kind"] == "binned":
        lib_option("FOC_GB_MERGE_MAX_RES", r["merge_max"])
        lib_option("FOC_GB_FACTORED", int(r["factored"] or not r["half"]))
    return r


def _dy(case, half):
    """dy_dx [B, L, D, C] of the case's table in the table dtype (the oracle's forward), once per case and dtype."""
    key = (case["name"], half)
    if key not in _DY:
        D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
        table = case["table"].astype(np.float16 if half else np.float32)
        _DY[key] = oracle.grid_encode_forward(case["x"], table, case["off"], D, C, L, case["S"], H, True, gridtype, ac, interp, acc_mode=1)[1]
    return _DY[key]


def _run(case, r, bl, dy=None, precount=None, table=None):
    D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
    B, n_rows = case["B"], int(case["off"][-1])
    tdt = torch.float16 if r["half"] else torch.float32
    g = _cuda(case["grad"]).to(tdt)
    if bl:
        g = g.permute(1, 0, 2).reshape(B, L * C).contiguous()
    xt, ot = _cuda(case["x"]), _cuda(case["off"])
    tt = table if table is not None else torch.zeros(n_rows, C, dtype=tdt, device="cuda")
    ge = torch.zeros(n_rows, C, dtype=tdt, device="cuda")
    gi = torch.zeros(B, D, dtype=tdt, device="cuda") if dy is not None else None
    dyt = _cuda(dy.reshape(B, -1)) if dy is not None else None
    be = _be()
    from focnerf_amd._lib import dtype_code
    binned = be.binned_workspace_bytes(ot, B, D, C, L, case["S"], H, gridtype, dtype_code(ge)) > 0
    assert binned == (r["kind"] == "binned"), "the call takes the route under test"
    be.grid_encode_backward(g, xt, tt, ot, ge, B, D, C, L, case["S"], H, dyt, gi, gridtype, ac, interp, grad_bl=bl, precount=precount)
    torch.cuda.synchronize()
    return to_np(ge).astype(np.float64), (to_np(gi).astype(np.float64) if gi is not None else None)


def _ratio(got, ref, bound, what):
    assert np.all(got[bound == 0] == 0), f"{what}: rows no in-range point touches are exactly zero"
    sel = bound > 0
    err = np.abs(got - ref)[sel]
    ratio = err / bound[sel]
    bad = ~(ratio <= 1.0)                                    # NaN counts as outside
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the bound, worst error / bound {worst:.3f}"
    return worst


def test_reference_layout_is_the_library_s():
    from focnerf_amd.gridencoder import level_offsets
    for case in CASES.values():
        D, C, L, H, lh, desired, _, ac, _ = case["spec"]
        assert np.array_equal(case["off"], level_offsets(D, L, np.exp2(np.log2(desired / H) / (L - 1)), H, lh, ac))


@pytest.mark.parametrize("name,rname", PAIRS, ids=[f"{n}-{r}" for n, r in PAIRS])
def test_backward_within_the_bound_of_its_route(name, rname, lib_option, monkeypatch):
    case = CASES[name]
    r = _select(rname, lib_option, monkeypatch)
    ref, b = G.reference(case)["ge"], G.bound(case, rname)
    shape = name.startswith("shape")
    dy = _dy(case, r["half"]) if shape else None
    worst = {}
    for bl in (False, True):
        got, gi = _run(case, r, bl, dy)
        worst["[B,L*C]" if bl else "[L,B,C]"] = _ratio(got, ref, b, f"{name} / {rname}")
        if name == "cancel" and rname == "binned16_12byte":
            assert np.all(got == 0), "g and -g cancel exactly on the two-corner records without merging"
        if gi is not None:
            gi_ref, gi_b = G.grad_inputs(case, dy, r["half"])
            worst["grad_inputs"] = _ratio(gi, gi_ref, gi_b, f"{name} / {rname} grad_inputs")
    print(f"\n{name} / {rname}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("rname", G.PLAN["overflow"])
def test_totals_beyond_half_are_not_finite(rname, lib_option, monkeypatch):
    """64 copies of one point with |g| = 60000 on fp16 tables (single-chunk slots): an element whose float64 total lies beyond the largest
    half by more than the bound must come out inf or NaN (what GradScaler looks for), an element whose addends cannot reach it even when
    they all align must be finite and within the bound; the elements in between may be either."""
    case = CASES["overflow"]
    r = _select(rname, lib_option, monkeypatch)
    ref, b = G.reference(case), G.bound(case, rname)
    must_overflow = np.abs(ref["ge"]) > 65520 + b
    must_hold = (ref["mag"] < G.HALF_MAX - b) & (ref["count"] > 0)
    for bl in (False, True):
        got, _ = _run(case, r, bl)
        assert not np.isfinite(got[must_overflow]).any()
        assert np.isfinite(got[must_hold]).all() and np.all(np.abs(got - ref["ge"])[must_hold] <= b[must_hold])
        assert np.all(got[ref["count"] == 0] == 0)
        either = (ref["count"] > 0) & ~must_overflow & ~must_hold
        print(f"\noverflow / {rname}: {int(must_overflow.sum())} elements not finite, {int(must_hold.sum())} finite and within the bound, "
              f"{int(either.sum())} in between of which {int(np.isfinite(got[either]).sum())} finite")


def test_precounted_backward_within_the_bound(lib_option, monkeypatch):
    """The count pass riding in the forward's launch (grid_encode_forward_counted -> ticket -> the scatter starts from its header)."""
    case = CASES["edges_2^0"]
    r = _select("binned16", lib_option, monkeypatch)
    D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
    B = case["B"]
    xt, ot = _cuda(case["x"]), _cuda(case["off"])
    table = _cuda(np.random.default_rng(1).uniform(-1, 1, (int(case["off"][-1]), C)).astype(np.float16))
    planes = torch.empty(L, B, C, dtype=torch.float16, device="cuda")
    be = _be()
    ticket = be.grid_encode_forward_counted(xt, table, ot, planes, B, D, C, L, case["S"], H, gridtype, ac, interp)
    assert ticket is not None
    g = _cuda(case["grad"])
    ge = torch.zeros(int(case["off"][-1]), C, dtype=torch.float16, device="cuda")
    from focnerf_amd import backend
    from focnerf_amd._lib import dtype_code
    dt = dtype_code(table)
    ws = backend._scratch.get("grid_bwd", be.binned_workspace_bytes(ot, B, D, C, L, case["S"], H, gridtype, dt), xt.device)
    assert be._precount_valid(ticket, xt, B, L, dt, ws), "the backward below starts from the forward's counts"
    be.grid_encode_backward(g, xt, table, ot, ge, B, D, C, L, case["S"], H, None, None, gridtype, ac, interp, grad_bl=False, precount=ticket)
    torch.cuda.synchronize()
    worst = _ratio(to_np(ge).astype(np.float64), G.reference(case)["ge"], G.bound(case, "binned16"), "precounted")
    print(f"\nedges_2^0 / binned16 precounted: worst error / bound {worst:.3f}")
