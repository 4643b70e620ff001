"""GPU: the hash-grid encoder's forward, dy_dx and grad_tv, every launch form a call can take, against the float64 reference of
tests/grid_forward_ref.py with its per-element bound (derivation: that module's docstring; the same cases as the numpy model in
test_grid_forward_ref.py, grid_forward_ref.PLAN / TV_PLAN). This is the check of the forward against the DEFINITION; the bit comparison
with oracle.c (test_gpu_gridencoder.py::test_forward_bit_exact) cannot see a misreading the two ports share.

Every element of out, dy_dx and the TV gradient must lie within its bound: nothing is excluded, no share of failures is allowed, an
element with bound 0 (an out-of-range point, a table row no cell touches) must be exactly 0. Output buffers start at FILL and carry a guard
band past their end that must come back untouched (grad_tv accumulates: its gradient starts at 0 in front of the same guard band). Every
test asserts the launch form its call takes (grid_forward_ref.forms(): ge_forward_launch / ge_pairs_mode / ge_forward_level restated
from the live option values, the table's alignment and foc_grid_forward_index_path). Forms that must give identical bits are asserted
bit-equal to the bounded one ("bits" below).

Measured on MI355X, worst |kernel - float64| / bound over every case (asserted <= 1):

    form                                                          quantity   fp32     fp16
    k_grid_fwd_lbc [L,B,C], plain walk + shared coarse group      out        0.019    0.989
      per level: ge_forward_hash3 (fp16 D=3 C=2 hash)             out        -        0.989 (focs_subnormal; 0.964 on uniform tables)
      per level: row pairs (FOC_GRID_FAST=0; mod_tiled_ac)        out        -        bits
      per level: one load per corner (FOC_GRID_PAIRS=0)           out        -        bits
      table only 4-byte aligned (pairs fallback)                  out        -        bits
      FOC_GRID_FUSE_SMALL=0 (no shared coarse group)              out        bits     bits
      with dy_dx (pairs off)                                      out        bits     bits
                                                                  dy_dx      0.016    0.969
    k_grid_fwd_bl [B, L*C] (out_bl=True)                          out        bits     bits
                                                                  dy_dx      bits     bits
    k_grid_fwd_pl (D = 4 / 5), [L,B,C]                            out        0.012    0.974
                                                                  dy_dx      0.012    0.945
    k_grid_fwd_pl, [B, L*C]                                       out, dy_dx bits     bits
    foc_grid_encode_forward_counted                               out        bits     bits
    tcnn.Encoding (HashGrid, TiledGrid, Smoothstep), B = 257      out        0.016    0.941
    k_grad_tv, D = 2..5, hash / tiled, align_corners on / off     grad       0.009    0.596
    foc_grid_planes_to_rows / foc_grid_rows_to_planes             exact permutations, round trip

fp16: the output's own rounding to half, h (|ref| + E) + q, is nearly all of the bound and is nearly used up (on the table of half
subnormals the bound is almost all q, 0.989). fp32 sits at 0.01 .. 0.02 on every form, and grad_tv at 0.002 .. 0.009: a slack bound
whose dominant term is the chain constant C (T + K) = 48 (forward, D = 3), 40 (dy_dx), C (n + K) >= 34 (grad_tv) of the module's rules
in front of sum |w v|, where the kernels' 2^D fmaf with weights that sum to 1 commit about one U |result|; the rules are the other
reference modules' and are not tuned here. grad_tv fp16 (0.24 .. 0.60) is the n packed half atomics. Wall time of the file: 3.6 s for
its 124 tests, 0.39 s the slowest (the 6 M-row table of foc19).
"""
import numpy as np
import pytest
import torch

import grid_forward_ref as F
from util import to_np

pytestmark = pytest.mark.gpu

FILL = 777.0
GUARD = 4096
FWD = [n for n in F.PLAN if n not in F.TV_PLAN]
DTYPES = [np.float32, np.float16]
IDS = ["fp32", "fp16"]


def _be():
    from focnerf_amd.backend import _gridencoder
    return _gridencoder


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Guarded:
    """A buffer of `shape` in front of a guard band of FILL; the buffer itself starts as `fill` (FILL: an element a kernel leaves out is
    outside its bound)."""

    def __init__(self, shape, dtype, fill=FILL):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), FILL, dtype=dtype, device="cuda")
        self.flat[:n] = fill
        self.t = self.flat[:n].view(*shape)
        self.n = n

    def intact(self):
        return bool(torch.all(self.flat[self.n:] == FILL))


def _ratio(got, ref, bound, what):
    got = got.astype(np.float64)
    assert np.all(got[bound == 0] == 0), f"{what}: an element with bound 0 is exactly zero"
    sel = bound > 0
    ratio = np.abs(got - ref)[sel] / bound[sel]
    bad = ~(ratio <= 1.0)                                    # NaN counts as outside
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the bound, worst error / bound {worst:.3f}"
    return worst


def _forms(case, tt, dy, bl):
    """The launch form of a forward call on table tensor `tt` under the library's live options."""
    from focnerf_amd import _lib
    opt = _lib.get_option
    return F.forms(case, tt.dtype == torch.float16, dy, bl, pairs=opt("FOC_GRID_PAIRS"), fast=opt("FOC_GRID_FAST"), fuse_small=opt("FOC_GRID_FUSE_SMALL"),
                   table_aligned=tt.data_ptr() % 8 == 0, index_path=_lib.lib.foc_grid_forward_index_path)


def _forward(case, tt, dy=False, bl=False, counted=False):
    """One forward call -> (out [L, B, C], dy_dx [B, L, D, C] or None) as numpy arrays in the table's type; guard bands checked."""
    D, C, L, H, _, _, gridtype, ac, interp = case["spec"]
    B = case["B"]
    xt, ot = _cuda(case["x"]), _cuda(case["off"])
    out = _Guarded((B, L * C) if bl else (L, B, C), tt.dtype)
    dyb = _Guarded((B, L * D * C), tt.dtype) if dy else None
    if counted:
        ticket = _be().grid_encode_forward_counted(xt, tt, ot, out.t, B, D, C, L, case["S"], H, gridtype, ac, interp)
        assert ticket is not None, "the counted forward serves this call"
    else:
        _be().grid_encode_forward(xt, tt, ot, out.t, B, D, C, L, case["S"], H, dyb.t if dy else None, gridtype, ac, interp, out_bl=bl)
    torch.cuda.synchronize()
    assert out.intact() and (dyb is None or dyb.intact()), "a write past the end of a buffer"
    o = to_np(out.t)
    if bl:
        o = np.ascontiguousarray(np.transpose(o.reshape(B, L, C), (1, 0, 2)))
    return o, (to_np(dyb.t).reshape(B, L, D, C) if dy else None)


def _bits(a, b, what):
    assert a.dtype == b.dtype and np.array_equal(a.view(np.uint16 if a.dtype == np.float16 else np.uint32), b.view(np.uint16 if b.dtype == np.float16 else np.uint32)), what


def test_reference_layout_is_the_library_s():
    from focnerf_amd.gridencoder import level_offsets
    for name in F.PLAN:
        case = F.case(name)
        D, C, L, H, lh, desired, _, ac, _ = case["spec"]
        assert np.array_equal(case["off"], level_offsets(D, L, np.exp2(np.log2(desired / H) / (L - 1)), H, lh, ac))
    from focnerf_amd import _lib
    assert (_lib.get_option("FOC_GRID_PAIRS"), _lib.get_option("FOC_GRID_FAST"), _lib.get_option("FOC_GRID_FUSE_SMALL")) == (1, 1, 1)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", FWD)
def test_forward_and_dy_dx_within_the_bound(name, dtype):
    """The four calls of a case: [L,B,C] and [B, L*C], each without and with dy_dx. The [L,B,C] call without dy_dx is bounded (for fp16
    D = 3 C = 2 hash grids that is ge_forward_hash3 under the shared coarse group, for other fp16 D = 3 C = 2 tables the row pairs, else one
    load per corner; D = 4 / 5: k_grid_fwd_pl); dy_dx of the [L,B,C] call is bounded; everything else must repeat those bits."""
    case = F.case(name)
    half = dtype == np.float16
    table = F.case_table(name, half)
    tt = _cuda(table)
    ref = F.reference(case, table)
    kernel, lc, per = _forms(case, tt, False, False)
    nd = case["D"] >= 4
    assert kernel == ("k_grid_fwd_pl" if nd else "k_grid_fwd_lbc")
    if not nd:
        fast = half and case["D"] == 3 and case["C"] == 2
        want = "hash3" if fast and case["gridtype"] == 0 and not case["ac"] and case["interp"] == 0 else ("pairs" if fast else "one")
        assert per == [want] * case["L"] and lc == F.small_levels(case) and _forms(case, tt, True, False)[2] == ["one"] * case["L"]
        assert _forms(case, tt, False, True)[0] == "k_grid_fwd_bl"
    out, _ = _forward(case, tt)
    w_out = _ratio(out, ref["out"], ref["out_b"], f"{name} out")
    out_d, dy = _forward(case, tt, dy=True)
    _bits(out_d, out, "[L,B,C] with dy_dx")
    w_dy = _ratio(dy, ref["dy"], ref["dy_b"], f"{name} dy_dx")
    out_bl, _ = _forward(case, tt, bl=True)
    _bits(out_bl, out, "[B, L*C]")
    out_bld, dy_bl = _forward(case, tt, dy=True, bl=True)
    _bits(out_bld, out, "[B, L*C] with dy_dx")
    _bits(dy_bl, dy, "dy_dx of the [B, L*C] call")
    print(f"\n{name} {IDS[half]} {kernel} lc={lc} {per[0]}: worst error / bound out {w_out:.3f} dy_dx {w_dy:.3f}")


@pytest.mark.parametrize("name", ["focs", "focs_B513", "foc19", "mod_tiled_ac", "focs_subnormal", "focs_cancel"])
def test_row_pair_forms_repeat_the_bounded_bits(name, lib_option):
    """fp16 D = 3 C = 2: ge_forward_hash3 (the default on a hash grid), the row pairs of ge_forward_one (FOC_GRID_FAST=0; the default
    of the tiled align_corners grid, whose first levels take `% size`), one load per corner (FOC_GRID_PAIRS=0), a table whose base is
    only 4-byte aligned, and the walk without the shared coarse group (FOC_GRID_FUSE_SMALL=0): one bounded, the rest the same bits."""
    case = F.case(name)
    table = F.case_table(name, True)
    L = case["L"]
    tt = _cuda(table)
    ref = F.reference(case, table)
    base_form = _forms(case, tt, False, False)
    hashgrid = case["gridtype"] == 0
    assert base_form == ("k_grid_fwd_lbc", F.small_levels(case), ["hash3" if hashgrid else "pairs"] * L) and base_form[1] >= 2
    out, _ = _forward(case, tt)
    worst = _ratio(out, ref["out"], ref["out_b"], f"{name} out")
    seen = {base_form[2][0]}
    for option, value, want in (("FOC_GRID_FAST", 0, "pairs"), ("FOC_GRID_PAIRS", 0, "one")):
        lib_option(option, value)
        assert _forms(case, tt, False, False)[2] == [want] * L
        _bits(_forward(case, tt)[0], out, f"{option}={value}")
        seen.add(want)
        lib_option(option, 1)
    # the same table 4 bytes past an 8-byte boundary: the whole launch falls back to one load per corner
    shifted = torch.empty(table.shape[0] + 1, 2, dtype=torch.float16, device="cuda")
    shifted[1:] = tt
    t4 = shifted[1:]
    assert t4.data_ptr() % 8 == 4 and _forms(case, t4, False, False)[2] == ["one"] * L
    _bits(_forward(case, t4)[0], out, "4-byte aligned table")
    lib_option("FOC_GRID_FUSE_SMALL", 0)
    assert _forms(case, tt, False, False)[1] == 0
    _bits(_forward(case, tt)[0], out, "FOC_GRID_FUSE_SMALL=0")
    # fp32 tables walk with and without the shared group too
    t32 = F.case_table(name, False)
    tt32 = _cuda(t32)
    plain32, _ = _forward(case, tt32)
    lib_option("FOC_GRID_FUSE_SMALL", 1)
    assert _forms(case, tt32, False, False)[1] >= 2
    _bits(_forward(case, tt32)[0], plain32, "fp32, shared coarse group")
    assert seen == {"hash3", "pairs", "one"} if hashgrid else seen == {"pairs", "one"}
    print(f"\n{name} fp16 {base_form[2][0]}: worst error / bound out {worst:.3f}; pairs / one load per corner / 4-byte table / no shared group: bits")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["focs_B1", "focs_B255", "focs_B256", "focs", "focs_B513", "foc19", "focs_subnormal"])
def test_counted_forward_repeats_the_bounded_bits(name, dtype, lib_option):
    """foc_grid_encode_forward_counted (k_grid_fwd_counted: the backward's count pass among the encoding workgroups): the plain call's
    bits, which are bounded here; with and without the shared coarse group."""
    case = F.case(name)
    table = F.case_table(name, dtype == np.float16)
    tt = _cuda(table)
    ref = F.reference(case, table)
    out, _ = _forward(case, tt)
    worst = _ratio(out, ref["out"], ref["out_b"], f"{name} out")
    _bits(_forward(case, tt, counted=True)[0], out, "counted")
    lib_option("FOC_GRID_FUSE_SMALL", 0)
    _bits(_forward(case, tt, counted=True)[0], out, "counted, FOC_GRID_FUSE_SMALL=0")
    print(f"\n{name} {IDS[dtype == np.float16]} counted: bits of the plain call (worst error / bound {worst:.3f})")


@pytest.mark.parametrize("unit", [4, 8])
@pytest.mark.parametrize("B,L", [(1, 16), (255, 16), (257, 9), (257, 32), (255, 1)])
def test_planes_and_rows_are_exact_permutations(B, L, unit):
    """foc_grid_planes_to_rows: [L, B] units -> [B, L]; foc_grid_rows_to_planes: the inverse; bit patterns of every kind travel unchanged."""
    rng = np.random.default_rng(B * 64 + L + unit)
    words = unit // 4
    planes = rng.integers(0, 2 ** 32, (L, B, words), dtype=np.uint64).astype(np.uint32).view(np.int32)
    pt = _cuda(planes)
    rows = _Guarded((B, L, words), torch.int32, fill=-1)
    rows.flat[rows.n:] = int(FILL)
    _be().planes_to_rows(pt, rows.t, B, L, unit)
    back = _Guarded((L, B, words), torch.int32, fill=-1)
    back.flat[back.n:] = int(FILL)
    _be().rows_to_planes(rows.t, back.t, B, L, unit)
    torch.cuda.synchronize()
    assert np.array_equal(to_np(rows.t), np.transpose(planes, (1, 0, 2))) and np.array_equal(to_np(back.t), planes)
    assert rows.intact() and back.intact()


@pytest.mark.parametrize("name,otype,dtype", [("focs", "HashGrid", torch.half), ("focs", "HashGrid", torch.float), ("D3_C4_tiled", "TiledGrid", torch.float),
                                              ("D3_C4_smooth", "HashGrid", torch.half), ("D2_smooth", "HashGrid", torch.float)])
def test_tcnn_encoding_within_the_bound(name, otype, dtype):
    from focnerf_amd import tcnn
    case = F.case(name)
    D, C, L, H, lh, desired, gridtype, ac, interp = case["spec"]
    assert case["B"] == 257 and not ac and gridtype == (otype == "TiledGrid")
    pls = float(np.exp2(np.log2(desired / H) / (L - 1)))
    assert float(np.log2(pls)) == case["S"]
    enc = tcnn.Encoding(D, dict(otype=otype, n_levels=L, n_features_per_level=C, log2_hashmap_size=lh, base_resolution=H, per_level_scale=pls,
                                interpolation="Smoothstep" if interp else "Linear"), dtype=dtype).cuda()
    half = dtype == torch.half
    table = F.case_table(name, half)
    assert enc.params.numel() == table.size and np.array_equal(to_np(enc._offsets), case["off"])
    enc.params.data.copy_(_cuda(table.astype(np.float32)).reshape(-1))
    y = enc(_cuda(case["x"]))
    assert y.dtype == dtype and y.shape == (257, L * C)
    ref = F.reference(case, table)
    got = np.transpose(to_np(y.detach()).reshape(257, L, C), (1, 0, 2))
    worst = _ratio(got, ref["out"], ref["out_b"], f"tcnn {name}")
    print(f"\ntcnn.Encoding {otype} {name} {'fp16' if half else 'fp32'}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", list(F.TV_PLAN))
def test_total_variation_within_the_bound(name, dtype):
    """k_grad_tv on a zeroed gradient: every element of the gradient within the bound of its addends (ten points share one cell of the
    coarse levels, where the atomics meet); rows no cell touches, and every row under a constant table, exactly 0."""
    case = F.case(name)
    half = dtype == np.float16
    table = F.case_table(name, half)
    D, C, L, H, _, _, gridtype, ac, _ = case["spec"]
    B = case["B"]
    ref, b = F.tv_reference(case, table)
    tt = _cuda(table)
    xt = _cuda(case["x"].astype(dtype))
    grad = _Guarded(table.shape, tt.dtype, fill=0.0)
    _be().grad_total_variation(xt, tt, grad.t, _cuda(case["off"]), F.TV_WEIGHT, B, D, C, L, case["S"], H, gridtype, ac)
    torch.cuda.synchronize()
    assert grad.intact()
    got = to_np(grad.t)
    worst = _ratio(got, ref, b, f"{name} grad_tv")
    if case["kind"] == "constant":
        assert np.all(got == 0)
    else:
        assert (got != 0).sum() >= min(B, 64)
    print(f"\n{name} {IDS[half]} k_grad_tv: worst error / bound {worst:.3f}")
