"""CPU: the float64 reference of the hash-grid forward, dy_dx and grad_tv (tests/grid_forward_ref.py) pinned to torch float64 autograd of
a plain interpolation written here, the C oracle held inside the reference's bound on every case (the check of oracle.c against the
definition), the scale / position / index assertions the reference's operands rest on, what the cases promise asserted on the reference
alone, and the bound exercised on the numpy model: the unmutated model is inside on every case, every mutant is outside on the case named
in CAUGHT_BY.

The GPU comparison is tests/test_gpu_grid_forward_reference.py; it walks the same cases (grid_forward_ref.PLAN / TV_PLAN)."""
import numpy as np
import pytest
import torch

import grid_backward_ref as G
import grid_forward_ref as F
import oracle

FWD = [n for n in F.PLAN if n not in F.TV_PLAN]
TV = list(F.TV_PLAN)
DTYPES = [np.float32, np.float16]

# mutant -> (case, half table, quantity) on which the bound notices it
CAUGHT_BY = {
    "drop_corner": ("focs", False, "out"),
    "half_accumulation": ("focs", True, "out"),
    "no_half_offset": ("focs", False, "out"),
    "ac_stride_plus_one": ("D2_tiled_ac", False, "out"),
    "smooth_deriv_6v": ("D3_C4_smooth", False, "dy"),
    "smooth_deriv_linear": ("D3_C4_smooth", False, "dy"),
    "primes_swapped": ("focs", False, "out"),
    "dense_index_on_hashed": ("focs", False, "out"),
    "subnormal_flush": ("focs_subnormal", True, "out"),
    "dy_without_scale": ("D3_C4_smooth", False, "dy"),
    "tv_right_le": ("tv_face", False, "tv"),
    "tv_weight_over_d": ("tv_D3_tiled", False, "tv"),
    "tv_no_eps": ("tv_D3_hash_ac_constant", False, "tv"),
}


def ratios(got, ref, bound):
    """|got - ref| / bound per element; an element with bound 0 must be exactly 0 (inf otherwise); NaN counts as outside."""
    got = np.asarray(got, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, np.abs(got - ref) / bound, np.where(got == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


def _oracle_forward(case, table):
    D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
    return oracle.grid_encode_forward(case["x"], table, case["off"], D, C, L, case["S"], H, True, gridtype, ac, interp, acc_mode=1)


def _oracle_tv(case, table, weight=F.TV_WEIGHT):
    D, C, L, H, _, _, gridtype, ac, _ = case["spec"]
    return oracle.grad_total_variation(case["x"], table, np.zeros_like(table), case["off"], weight, D, C, L, case["S"], H, gridtype, ac)


def test_the_specs_hold_every_case_of_the_bit_exact_test():
    import test_gpu_gridencoder as T
    assert set(T.CASES) <= set(F.SPECS.values())
    assert {F.PLAN[n][1] for n in F.PLAN if F.PLAN[n][0] == "focs"} >= set(F.BATCHES)


@pytest.mark.parametrize("name", list(F.PLAN))
def test_scale_position_and_index(name):
    """scale32 against the float64 2^(l S) H - 1 within the three fp32 roundings; resolution == ceil(scale32) + 1; pos32 within half an
    fp32 ulp of the float64 position; a cell never reaches the resolution; index() (get_grid_index restated here) gives the rows of
    grid_backward_ref._rows, which the backward's reference rests on."""
    case = F.case(name)
    add = 0.0 if case["ac"] else 0.5
    for l in range(case["L"]):
        lv = G.level(case, l)
        assert abs(lv["scale"] - F.scale64(case, l)) <= F.scale_allowance(case, l), (l, lv["scale"], F.scale64(case, l))
        assert lv["res"] == int(np.ceil(lv["scale"])) + 1
        x = case["x"][lv["idx"]]
        pos32, _ = G._fma32(x, lv["scale"], add)
        pos64 = x.astype(np.float64) * lv["scale"] + add
        assert np.all(np.abs(pos32.astype(np.float64) - pos64) <= 0.5 * np.spacing(np.abs(pos32)).astype(np.float64) + 2.0 ** -60)
        assert np.array_equal(np.floor(pos32).astype(np.int64), lv["cell"]) and np.array_equal((pos32 - np.floor(pos32)), lv["frac32"])
        assert lv["cell"].min(initial=0) >= 0 and lv["cell"].max(initial=0) <= lv["res"] - 1
        assert np.array_equal(F.index(case, F.corners(lv["cell"], case["D"]), lv["size"], lv["res"]), lv["rows"])
        assert lv["size"] == int(case["off"][l + 1] - case["off"][l]) and lv["rows"].max(initial=0) < lv["size"]


@pytest.mark.parametrize("name", ["D2_tiled_ac", "D3_C4_smooth", "D5_C1_smooth", "mod_tiled_ac"])
def test_reference_against_autograd(name):
    """A plain float64 interpolation in torch (cells and rows from the reference, the position pinned to pos32 with slope scale): the
    forward values, and dy_dx as d out / d x through autograd."""
    case = F.case(name)
    table = F.case_table(name, False)
    ref = F.reference(case, table)
    D, C, L = case["D"], case["C"], case["L"]
    tt = torch.tensor(table.astype(np.float64))
    k = np.arange(1 << D)
    for l in range(L):
        lv = F.flevel(case, l)
        x = torch.tensor(case["x"][lv["idx"]].astype(np.float64), requires_grad=True)
        pos32 = torch.from_numpy((lv["cell"] + lv["frac64"]).astype(np.float64))
        f = (x - x.detach()) * float(lv["scale"]) + pos32 - torch.from_numpy(lv["cell"].astype(np.float64))
        if case["interp"] == 1:
            f = f * f * (3 - 2 * f)
        w = torch.ones(x.shape[0], 1 << D, dtype=torch.float64)
        for d in range(D):
            bit = torch.from_numpy(((k >> d) & 1).astype(bool))[None]
            w = w * torch.where(bit, f[:, d:d + 1], 1 - f[:, d:d + 1])
        out = (w[:, :, None] * tt[torch.from_numpy(lv["rows"] + int(case["off"][l]))]).sum(1)
        assert np.abs(out.detach().numpy() - ref["out"][l, lv["idx"]]).max() <= 1e-13
        for c in range(C):
            gx, = torch.autograd.grad(out[:, c].sum(), x, retain_graph=True)
            want = ref["dy"][lv["idx"], l, :, c]
            assert np.abs(gx.numpy() - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    out64, dy64 = F.forward64(case, table, fp32_fraction=True)
    assert np.abs(out64 - ref["out"]).max() <= 1e-13 and np.abs(dy64 - ref["dy"]).max() <= 1e-9
    inb = np.all((case["x"] >= 0) & (case["x"] <= 1), axis=1)
    assert (~inb).sum() >= 2 and np.all(ref["out"][:, ~inb] == 0) and np.all(ref["dy"][~inb] == 0) and np.all(ref["out_b"][:, ~inb] == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", FWD)
def test_oracle_forward_inside_the_bound(name, dtype):
    case = F.case(name)
    table = F.case_table(name, dtype == np.float16)
    ref = F.reference(case, table)
    out, dy = _oracle_forward(case, table)
    ro, rd = ratios(out, ref["out"], ref["out_b"]).max(), ratios(dy, ref["dy"], ref["dy_b"]).max()
    print(f"{name} {dtype.__name__}: oracle worst error / bound out {ro:.3f} dy_dx {rd:.3f}")
    assert ro <= 1.0 and rd <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", TV)
def test_oracle_total_variation_inside_the_bound(name, dtype):
    """fp32 tables: the bound the kernel is held to. Half tables: oracle.c keeps the reference's half arithmetic (a rounding to half after
    every operation of kernel_grad_tv); it is held to the bound of that arithmetic (tv_reference(literal_half=True))."""
    case = F.case(name)
    half = dtype == np.float16
    table = F.case_table(name, half)
    ref, b = F.tv_reference(case, table, literal_half=half)
    r = ratios(_oracle_tv(case, table), ref, b).max()
    print(f"{name} {dtype.__name__}: oracle grad_tv worst error / bound {r:.3f}")
    assert r <= 1.0
    assert (b > 0).any() == (case["kind"] != "constant")


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", FWD)
def test_model_forward_inside_the_bound(name, dtype):
    case = F.case(name)
    table = F.case_table(name, dtype == np.float16)
    ref = F.reference(case, table)
    out, dy = F.model(case, table)
    ro, rd = ratios(out, ref["out"], ref["out_b"]).max(), ratios(dy, ref["dy"], ref["dy_b"]).max()
    print(f"{name} {dtype.__name__}: model worst error / bound out {ro:.3f} dy_dx {rd:.3f}")
    assert ro <= 1.0 and rd <= 1.0
    # the model IS the oracle's fmaf sequence: the same bits (a second, independent statement of oracle.c's forward)
    o_out, o_dy = _oracle_forward(case, table)
    assert np.array_equal(out, o_out)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", TV + ["tv_face"])
def test_model_total_variation_inside_the_bound(name, dtype):
    case = F.case(name)
    table = F.case_table(name, dtype == np.float16)
    cells = case.get("cells")
    ref, b = F.tv_reference(case, table, cells=cells)
    got = F.tv_model(case, table, cells=cells)
    r = ratios(got, ref, b).max()
    print(f"{name} {dtype.__name__}: model grad_tv worst error / bound {r:.3f}")
    assert r <= 1.0
    if case["kind"] == "constant":
        assert np.all(got == 0) and np.all(b == 0)


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    name, half, what = CAUGHT_BY[mutant]
    case = F.case(name)
    table = F.case_table(name, half)
    if what == "tv":
        cells = case.get("cells")
        ref, b = F.tv_reference(case, table, cells=cells)
        r = ratios(F.tv_model(case, table, mutant=mutant, cells=cells), ref, b)
        if mutant == "tv_right_le":
            # the same bits wherever a position of [0, 1] put the stencil: the mutant shows on cells handed over directly only
            for n in TV:
                c, t = F.case(n), F.case_table(n, half)
                assert np.array_equal(F.tv_model(c, t, mutant=mutant), F.tv_model(c, t))
    else:
        ref = F.reference(case, table)
        out, dy = F.model(case, table, mutant)
        r = ratios(out, ref["out"], ref["out_b"]) if what == "out" else ratios(dy, ref["dy"], ref["dy_b"])
    print(f"{mutant}: {name} {'fp16' if half else 'fp32'} {what}: worst error / bound {r.max():.3g} on {(r > 1).sum()} elements")
    assert r.max() > 1.0
    assert set(CAUGHT_BY) == set(F.MUTANTS)


def test_case_promises():
    """What the cases promise, from the reference alone. From B = 64 on every case holds: 0, 1 and 1 - 2^-24 on every axis, -0.0, a
    coordinate just below 0 and one just above 1 on different points, points whose pos32 is a whole number (cell boundaries) at the first,
    a middle and the last level, ten points in one cell of the coarse levels; the random points give even and odd cell_x on the hashed
    levels and the last cell along every axis comes from x = 1."""
    for name in F.PLAN:
        case = F.case(name)
        x, sp, D, L = case["x"], case["special"], case["D"], case["L"]
        assert case["B"] == F.PLAN[name][1]
        if case["B"] < 64:
            continue
        assert np.all(x[sp["zero"]] == 0) and np.all(x[sp["one"]] == 1) and np.all(x[sp["below_one"]] == np.float32(1) - np.float32(2.0 ** -24))
        assert np.all(x[sp["neg_zero"]] == 0) and np.signbit(x[sp["neg_zero"]]).all()
        assert -1e-30 < x[sp["below_zero"], 0] < 0 and 1 < x[sp["above_one"], D - 1] < 1 + 1e-6
        inside = G.level(case, 0)["inside"]
        assert not inside[sp["below_zero"]] and not inside[sp["above_one"]] and inside[[sp["zero"], sp["one"], sp["below_one"], sp["neg_zero"]]].all()
        for r, l, d in sp["whole"]:
            lv = G.level(case, l)
            at = int(np.nonzero(lv["idx"] == r)[0][0])
            assert lv["frac32"][at, d] == 0 and lv["cell"][at, d] >= 1
        lv0 = G.level(case, 0)
        at = np.nonzero(np.isin(lv0["idx"], sp["cluster"]))[0]
        assert at.size == 10 and np.all(lv0["cell"][at] == lv0["cell"][at[0]]), "ten points in one cell"
        for l in range(L):
            lv = G.level(case, l)
            one = int(np.nonzero(lv["idx"] == sp["one"])[0][0])
            last = np.floor(G._fma32(np.ones(1, np.float32), lv["scale"], 0.0 if case["ac"] else 0.5)[0][0])
            assert np.all(lv["cell"][one] == last) and last >= lv["res"] - 2 and lv["cell"].max() == last
            if lv["hashed"] and case["B"] >= 255:
                assert set((lv["cell"][:, 0] & 1).tolist()) == {0, 1}, "even and odd cell_x on a hashed level"
    # focs: dense levels, hashed levels, eight levels in the shared workgroup; every arithmetic form of the fp16 fast shape
    c = F.case("focs")
    hashed = [G.level(c, l)["hashed"] for l in range(16)]
    assert hashed[:3] == [False] * 3 and all(hashed[3:]) and F.small_levels(c) == 8 and F.small_levels(c, 0) == 0
    assert F.forms(c, True, False, False) == ("k_grid_fwd_lbc", 8, ["hash3"] * 16)
    assert F.forms(c, True, False, False, fast=0)[2] == ["pairs"] * 16 and F.forms(c, True, True, False)[2] == ["one"] * 16
    assert F.forms(c, True, False, False, table_aligned=False)[2] == ["one"] * 16 and F.forms(c, False, False, False)[2] == ["one"] * 16
    assert F.forms(c, True, False, True)[0] == "k_grid_fwd_bl" and F.forms(F.case("D4"), True, False, False)[0] == "k_grid_fwd_pl"
    assert F.small_levels(F.case("D3_C1")) >= 2 and F.small_levels(F.case("mod_tiled_ac")) >= 2
    # the level sizes that are no power of two take `% size`: a raw index at or beyond the size
    c = F.case("mod_tiled_ac")
    sizes = [G.level(c, l)["size"] for l in range(4)]
    assert sizes == [216, 1728, 13824, 16384] and (sizes[0] // 8) % 2 == 1
    for l in (0, 1, 2):
        lv = G.level(c, l)
        raw = F.index(c, F.corners(lv["cell"], 3), lv["size"], lv["res"], raw=True)
        assert (raw >= lv["size"]).sum() >= 1, "a row of this level wraps"
    assert F.forms(c, True, False, False)[2] == ["pairs"] * 4
    # L = 9: a level in the second group of eight block slots
    assert F.case("D4_L9")["L"] == 9 and F.case("D5_L9")["L"] == 9 and F.case("tv_D4_hash_L9")["L"] == 9
    # subnormal tables: every value a half subnormal, outputs below the smallest normal half
    c, t = F.case("focs_subnormal"), F.case_table("focs_subnormal", True)
    assert np.abs(t.astype(np.float32)).max() < 2.0 ** -14 and (t != 0).mean() > 0.99
    ref = F.reference(c, t)
    assert np.abs(ref["out"]).max() < 2.0 ** -14 and (ref["out"] != 0).mean() > 0.9
    # cancellation: on the centred points of the dense level sum w v is a hundredth of sum |w v|, which is about 1
    c, t = F.case("focs_cancel"), F.case_table("focs_cancel", False)
    lv = F.flevel(c, F.CANCEL_LEVEL)
    assert not lv["hashed"]
    at = np.nonzero(np.isin(lv["idx"], c["special"]["centred"]))[0]
    w, _ = G._weights(c, lv)
    vals = t[lv["rows"][at] + int(c["off"][F.CANCEL_LEVEL])].astype(np.float64)
    s, a = (w[at, :, None] * vals).sum(1), np.abs(w[at, :, None] * vals).sum(1)
    assert at.size >= 400 and np.all(a > 0.9) and np.all(np.abs(s) <= 1e-2 * a)
    # grad_tv: at least 8 points in one cell, cells at both faces of the box, a constant table with every addend exactly 0
    for name in F.TV_PLAN:
        c = F.case(name)
        if c["B"] < 64:
            continue
        tc = F.tv_positions(c, True)
        for cc in (c, tc):
            lv = G.level(cc, 0)
            _, counts = np.unique(lv["cell"], axis=0, return_counts=True)
            assert counts.max() >= 8
            for l in range(c["L"]):
                lv = G.level(cc, l)
                assert (lv["cell"] == 0).any() and (lv["cell"] >= lv["res"] - 2).any()
    ref, b = F.tv_reference(F.case("tv_D3_hash_ac_constant"), F.case_table("tv_D3_hash_ac_constant", False))
    assert np.all(ref == 0) and np.all(b == 0)
    ref, _ = F.tv_reference(F.case("tv_D3_tiled"), F.case_table("tv_D3_tiled", False))
    assert (ref != 0).sum() > 100
    face = F.case("tv_face")
    assert all((face["cells"][l] == G.level(face, l)["res"]).any() for l in range(face["L"]))
