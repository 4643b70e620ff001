"""GPU: the fully fused MLP (csrc/ffmlp.hip, csrc/ffmlp_wide.hip), every route a call can take, layer by layer against the float64
reference of tests/mlp_ref.py on the operands the kernel itself read, with that module's per-element bound (derivation: its docstring;
the same cases and routes as tests/test_mlp_ref.py, mlp_ref.PLAN).

Every element of forward_buffer, outputs, backward_buffer, grad_inputs and grad_weights must lie within its bound; an element without a
nonzero product, or masked by the ReLU, must be exactly zero; nothing is excluded and no share of failures is allowed; every buffer
carries a guard band past its last row that must come back untouched. Forms whose intermediates never leave the chip (inference, the
forward without forward_buffer, the planar forward, the recomputing, lean and planar backward) must give the bits of the form that
emits them, in the same test and on the same data, and their grad_weights are bounded against the float64 sum of the emitting form's
buffers. Every route runs with and without input gradients, and each test asserts that the call takes the route (`_select`).

Routes (mlp_ref.ROUTES): stored single pass, recompute, lean, planar, two-kernel (FOC_MLP_BWD_FUSED=0, or by shape), two-kernel with
FOC_DETERMINISTIC=1, hidden 256 (also deterministic), wide input. Cases: twelve shapes x ten batch sizes around the 32 / 64 / 128 / 256
row tiles; gradient scales 2^-16 .. 2^8; cancelling row pairs; totals beyond half; one inf in the gradient; and five loop-edge batches
computed from the number of compute units at which the persistent kernels' workgroups meet rows a second time.

Hidden activations 1..5 have their own file, tests/test_gpu_pointwise_reference.py (same method, on this module's helpers).
Out of scope: the colour-head and whole-field forms, performance (mlp_ref's docstring says why).

Measured on MI355X (256 CUs), worst |kernel - float64| / bound, asserted <= 1, nothing excluded. The row-wise quantities have at most
256 products per element, so nearly all of their bound is the half rounding of the result itself and a worst ratio just below 1 is what a
correct kernel gives (the oracle's k-ordered fmaf chain: fb 0.996, out 0.999, bb 0.999, grad_inputs 0.999, grad_weights 1.000).

    route (cases)                     fb     out    bb     grad_inputs  grad_weights
    stored            (batch edges)   0.999  0.999  0.998  0.999        1.000   (1.000: B = 1, one product, a tie of the half rounding)
    recompute         (batch edges)   bits   bits   bits   bits         1.000
    lean              (batch edges)   bits   bits   -      bits         1.000
    planar            (batch edges)   bits   bits   -      bits         1.000
    two-kernel        (batch edges)   0.999  0.999  0.998  0.999        1.000
    two-kernel, det.  (batch edges)   0.999  0.999  0.998  0.999        1.000
    hidden 256 (both) (batch edges)   0.988  0.905  0.994  0.915        1.000
    wide input        (batch edges)   0.995  0.996  0.995  0.996        1.000
    every route, scales 2^-16 .. 2^8  0.989  0.987  0.999  0.999        0.998   (2^-16: 0.998; 2^-8 0.988; 2^0 0.988; 2^8 0.993)
    cancellation, single pass / det.  0.986  0.988  0.994  0.984        0.006
    cancellation, two-kernel atomics  0.986  0.988  0.994  0.984        0.027
    totals beyond half (must hold)    0.983  0.983  0.996  0.980        0.999   (4008 of 7168 elements must be and are non-finite at 32 x 64 x 2)
    one inf in the gradient           -      -      bits   bits         0.996   (on the elements whose reference is finite)
    loop: fused backward, B 65 681    0.987  0.991  0.993  0.985        0.985   (stored; recompute, lean, planar: bits and 0.985)
    loop: k_mlp_dw, B 43 777          0.971  0.967  0.994  0.963        0.997
    loop: k_mlp_dw det., B 2 113      0.973  0.967  0.994  0.970        0.985
    loop: k_mlp_bwd, B 262 417        0.970  0.969  0.994  0.966        0.991
    loop: forward, B 262 289          0.986  0.986  (inference, forward_buffer-free and planar forms: bits)

"bits": identical to the emitting form in the same test. 154 tests; wall time of the file 6.7 s, the slowest test 0.6 s (the first,
which loads the library), the loop-edge tests 0.06 s each. No kernel changed: the first run had every element inside its bound.
NOTEBOOK.md, "MLP against float64", has the error model and the mutants.
"""
from collections import defaultdict

import numpy as np
import pytest
import torch

import mlp_ref as M
from util import to_np

pytestmark = pytest.mark.gpu

GUARD = 4096                  # halves past the end of every buffer the kernels write
FILL = 7.0


def _be():
    from focnerf_amd.backend import _ffmlp
    return _ffmlp


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Guarded:
    """A half buffer of `shape` in front of a guard band; everything starts as FILL (an element the kernel leaves out is outside its bound)."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.flat = torch.full((n + GUARD,), FILL, dtype=torch.float16, device="cuda")
        self.t = self.flat[:n].view(*shape)
        self.n = n

    def intact(self):
        return bool(torch.all(self.flat[self.n:] == FILL))


def _select(rname, I, H, nl, act, lib_option):
    """Put the library on route `rname` and assert that a call of this shape takes it: the option values, the wrapper's own statement of
    the selection, and the library's behaviour (only the single pass runs without a backward_buffer; only FOC_DETERMINISTIC asks for one
    workspace image per split-K workgroup)."""
    from focnerf_amd import _lib
    from focnerf_amd.ffmlp import single_pass_backward
    r = M.ROUTES[rname]
    lib_option("FOC_DETERMINISTIC", r["det"])
    lib_option("FOC_MLP_BWD_FUSED", M.fused_option(rname, I, H, nl, act))
    assert (_lib.get_option("FOC_DETERMINISTIC"), _lib.get_option("FOC_MLP_BWD_FUSED")) == (r["det"], M.fused_option(rname, I, H, nl, act))
    ks = M.kernels(rname, I, H, nl, act, True)
    assert ks is not None, f"{rname} does not serve {I} x {H} x {nl}"
    fused = ks[0].startswith("k_mlp_bwd_fused")
    assert fused == r["fused"] and single_pass_backward(I, H, nl, act) == fused
    z = lambda *s: torch.zeros(*s, dtype=torch.float16, device="cuda")
    args = (z(1, 16), z(1, I), z(M.n_params(I, H, nl)), None, 1, I, 16, H, nl, act, 6, False, None, z(1), z(M.n_params(I, H, nl)))
    if fused:
        _be().ffmlp_backward(*args)
    else:
        with pytest.raises(RuntimeError, match="backward_buffer"):
            _be().ffmlp_backward(*args)
    blob = (M.n_params(I, H, nl) + 63) // 64 * 64 * 4
    ws = int(_lib.lib.foc_ffmlp_backward_workspace_bytes(I, H, nl))
    if r["det"]:
        assert ws >= M.DW_DET_SLOTS * blob
    elif not M.single_pass(I, H, nl, M.RELU):
        assert ws == blob
    return r


def _forward(form, xt, Wt, I, H, nl, act):
    """out (and fb for 'train') of one forward form, guard bands checked."""
    be = _be()
    B = xt.shape[0] if form != "planar" else xt.shape[1]
    out = _Guarded(B, 16)
    fb = None
    if form == "train":
        fb = _Guarded(nl, B, H)
        be.ffmlp_forward(xt, Wt, B, I, 16, H, nl, act, 6, fb.t, out.t)
    elif form == "nofb":
        be.ffmlp_forward(xt, Wt, B, I, 16, H, nl, act, 6, None, out.t)
    elif form == "inference":
        scratch = torch.empty(B, H, dtype=torch.float16, device="cuda") if H > 128 else None
        be.ffmlp_inference(xt, Wt, B, I, 16, H, nl, act, 6, scratch, out.t)
    else:
        be.ffmlp_forward_planar(xt, Wt, B, I, 16, H, nl, act, 6, out.t)
    torch.cuda.synchronize()
    assert out.intact() and (fb is None or fb.intact()), f"{form} forward wrote past row B"
    return out.t, (fb.t if fb is not None else None)


def _planar(xt):
    B, I = xt.shape
    return xt.view(B, I // 2, 2).permute(1, 0, 2).contiguous()


def _backward(rname, dx, gt, xt, Wt, fbt, I, H, nl, act):
    """(bb or None, grad_inputs [B, I] or None, grad_weights) of one backward call on the route, guard bands checked."""
    be = _be()
    r = M.ROUTES[rname]
    B = gt.shape[0]
    gw = _Guarded(M.n_params(I, H, nl))
    bb = _Guarded(nl, B, H) if r["bb"] else None
    none = torch.zeros(1, dtype=torch.float16, device="cuda")
    if r["planar"]:
        gi = _Guarded(I // 2, B, 2) if dx else None
        be.ffmlp_backward_planar(gt, _planar(xt), Wt, B, I, 16, H, nl, act, 6, dx, gi.t if dx else none, gw.t)
    else:
        gi = _Guarded(B, I) if dx else None
        be.ffmlp_backward(gt, xt, Wt, fbt if r["fb"] else None, B, I, 16, H, nl, act, 6, dx, bb.t if bb else None, gi.t if dx else none, gw.t)
    torch.cuda.synchronize()
    assert gw.intact() and (bb is None or bb.intact()) and (gi is None or gi.intact()), f"{rname} backward wrote past the end of a buffer"
    git = None
    if dx:
        git = gi.t.permute(1, 0, 2).reshape(B, I).contiguous() if r["planar"] else gi.t
    return (bb.t if bb else None), git, gw.t


def _note(worst, key, v):
    worst[key] = max(worst[key], v)


def _forward_checks(c, act, xt, Wt, Ws, worst, rows=None):
    """Training forward against float64 layer by layer (on `rows` where given), then every other forward form bit for bit. Returns fb."""
    I, H, nl = c["I"], c["H"], c["nl"]
    what = f"{c['name']} act {act}"
    out, fb = _forward("train", xt, Wt, I, H, nl, act)
    sel = slice(None) if rows is None else torch.from_numpy(rows).cuda()
    xs, fbs, outs = to_np(xt[sel]), to_np(fb[:, sel]), to_np(out[sel])
    assert np.abs(fbs.astype(np.float32)).max() < M.HALF_MAX
    for l in range(nl):
        _note(worst, "fb", M.worst_ratio(fbs[l], M.forward_layer(l, xs, fbs, Ws, act), f"{what} fb[{l}]"))
    _note(worst, "out", M.worst_ratio(outs, M.output(fbs, Ws), f"{what} out"))
    forms = ["inference"] + (["nofb"] if H <= 128 else []) + (["planar"] if M.single_pass(I, H, nl, act) else [])
    for form in forms:
        o2, _ = _forward(form, _planar(xt) if form == "planar" else xt, Wt, I, H, nl, act)
        assert torch.equal(o2, out), f"{what}: the {form} forward differs from the training forward"
    return fb


def _overflow_check(gw, q, what):
    """Elements whose float64 total lies beyond the largest half by more than the bound are not finite; elements whose addends cannot
    reach it even when they all align are finite and within the bound; the rest may be either."""
    must_overflow = np.abs(q["ref"]) > M.HALF_OVER + q["bound"]
    must_hold = (q["mag"] < M.HALF_MAX - q["bound"]) & (q["count"] > 0)
    assert must_overflow.sum() >= 16 and must_hold.sum() >= 16, "degenerate overflow data"
    assert not np.isfinite(gw[must_overflow]).any(), f"{what}: a total beyond half came out finite"
    assert np.all(gw[q["count"] == 0] == 0)
    held = M.worst_ratio(gw[must_hold], {"ref": q["ref"][must_hold], "bound": q["bound"][must_hold]}, what)
    either = (q["count"] > 0) & ~must_overflow & ~must_hold
    print(f"\n{what}: {int(must_overflow.sum())} elements not finite, {int(must_hold.sum())} finite and within the bound (worst {held:.3f}), "
          f"{int(either.sum())} in between of which {int(np.isfinite(gw[either]).sum())} finite")
    return held


def _check_case(c, act, rname, worst, overflow=False):
    """One case on one route: forward, the emitting backward form against float64, then (where the route is another form) the route
    itself bit for bit and its grad_weights within the bound, with and without input gradients."""
    I, H, nl = c["I"], c["H"], c["nl"]
    what = f"{c['name']} act {act} {rname}"
    xt, Wt, gt = _cuda(c["x"]), _cuda(c["W"]), _cuda(c["grad"])
    Ws = M.split(c["W"], I, H, nl)
    fb = _forward_checks(c, act, xt, Wt, Ws, worst)
    fbn = to_np(fb)
    er = M.emitting_route(rname)
    bb_e, gi_e, gw_e = _backward(er, True, gt, xt, Wt, fb, I, H, nl, act)
    bbn = to_np(bb_e)
    for k in range(nl):
        _note(worst, "bb", M.worst_ratio(bbn[k], M.delta(k, c["grad"], fbn, bbn, Ws, act), f"{what} bb[{k}]"))
    _note(worst, "grad_inputs", M.worst_ratio(to_np(gi_e), M.grad_inputs(bbn, Ws), f"{what} grad_inputs"))
    q = M.grad_weights(c["x"], fbn, bbn, c["grad"], nl)

    def gw_check(gw, tag):
        g = to_np(gw).astype(np.float64)
        if overflow:
            _note(worst, "grad_weights", _overflow_check(g, q, f"{what} {tag}"))
        else:
            _note(worst, "grad_weights", M.worst_ratio(g, q, f"{what} grad_weights {tag}"))
    gw_check(gw_e, f"({er}, dx)")
    for dx in (True, False):
        if (rname == er and dx) or M.kernels(rname, I, H, nl, act, dx) is None:
            continue
        bb_r, gi_r, gw_r = _backward(rname, dx, gt, xt, Wt, fb, I, H, nl, act)
        if bb_r is not None:
            assert torch.equal(bb_r, bb_e), f"{what}: backward_buffer differs from the {er} form's (dx {dx})"
        if dx:
            assert torch.equal(gi_r, gi_e), f"{what}: grad_inputs differ from the {er} form's"
        gw_check(gw_r, f"({rname}, dx {dx})")


def _report(title, worst):
    print(f"\n{title}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _triples():
    out = []
    for I, H, nl in M.SHAPES:
        for rname in M.routes_for(I, H, nl, M.RELU):
            for act in M.acts_for(rname):
                if M.kernels(rname, I, H, nl, act, True) is not None:
                    out.append((I, H, nl, rname, act))
    return out


TRIPLES = _triples()


@pytest.mark.parametrize("I,H,nl,rname,act", TRIPLES, ids=[f"{M.shape_name(I, H, nl)}-{r}-act{a}" for I, H, nl, r, a in TRIPLES])
def test_every_layer_within_its_bound_at_the_batch_edges(I, H, nl, rname, act, lib_option):
    """B in {1, 31, 33, 63, 65, 127, 129, 257, 333, 1000}: around the 32-row wave tile, the 64-row dW chunk, the 128-row fused workgroup
    and the 256-row k_mlp_bwd workgroup."""
    _select(rname, I, H, nl, act, lib_option)
    worst = defaultdict(float)
    for B in M.BATCHES:
        _check_case(M.case(f"shape_{M.shape_name(I, H, nl)}_B{B}"), act, rname, worst)
    _report(f"{M.shape_name(I, H, nl)} / {rname} / act {act}", worst)


_PAIRS = [(n, r) for n in M.names("scale") + M.names("cancel") for r in M.PLAN[n]]


@pytest.mark.parametrize("name,rname", _PAIRS, ids=[f"{n}-{r}" for n, r in _PAIRS])
def test_gradient_scales_and_cancellation(name, rname, lib_option):
    """Gradients of scale 2^-16 (most deltas are subnormal halves) .. 2^8, and rows in pairs with the same x and gradients g, -g: only
    the bound applies to the latter, the order of the sum is the kernel's."""
    c = M.case(name)
    worst = defaultdict(float)
    for act in M.acts_for(rname):
        _select(rname, c["I"], c["H"], c["nl"], act, lib_option)
        _check_case(c, act, rname, worst)
    _report(f"{name} / {rname}", worst)


_OVER = [(n, r) for n in M.names("overflow") for r in M.PLAN[n]]


@pytest.mark.parametrize("name,rname", _OVER, ids=[f"{n}-{r}" for n, r in _OVER])
def test_totals_beyond_half_are_not_finite(name, rname, lib_option):
    """|g| = 60000 in one output column of every row: every delta is finite, and a grad_weights element whose float64 total lies beyond
    the largest half by more than its bound must come out inf or NaN (what the LossScaler's check looks for)."""
    c = M.case(name)
    _select(rname, c["I"], c["H"], c["nl"], M.RELU, lib_option)
    worst = defaultdict(float)
    _check_case(c, M.RELU, rname, worst, overflow=True)
    _report(f"{name} / {rname}", worst)


_NONF = [(n, r) for n in M.names("nonfinite") for r in M.PLAN[n]]


@pytest.mark.parametrize("name,rname", _NONF, ids=[f"{n}-{r}" for n, r in _NONF])
def test_one_inf_in_the_gradient(name, rname, lib_option):
    """grad[b, o] = inf: row o of dW_out is non-finite everywhere; the rows of the other samples in backward_buffer and grad_inputs are the
    bits of the run without it; nothing is NaN (or outside its bound) where the float64 reference is finite."""
    c = M.case(name)
    I, H, nl, b, o = c["I"], c["H"], c["nl"], c["inf_row"], c["inf_col"]
    _select(rname, I, H, nl, M.RELU, lib_option)
    xt, Wt = _cuda(c["x"]), _cuda(c["W"])
    _, fb = _forward("train", xt, Wt, I, H, nl, M.RELU)
    fbn = to_np(fb)
    er = M.emitting_route(rname)
    keep = torch.arange(c["B"], device="cuda") != b
    bb_i, _, _ = _backward(er, True, _cuda(c["grad"]), xt, Wt, fb, I, H, nl, M.RELU)
    with np.errstate(invalid="ignore", over="ignore"):
        q = M.grad_weights(c["x"], fbn, to_np(bb_i), c["grad"], nl)
    finite = np.isfinite(q["ref"]) & np.isfinite(q["bound"])
    assert finite.sum() > 0.25 * finite.size, "degenerate: the inf reaches nearly every weight"
    start, _, cols = M.offsets(I, H, nl)[-1]
    for dx in (True, False):
        if M.kernels(rname, I, H, nl, M.RELU, dx) is None:
            continue
        bb0, gi0, _ = _backward(rname, dx, _cuda(c["grad_finite"]), xt, Wt, fb, I, H, nl, M.RELU)
        bb1, gi1, gw1 = _backward(rname, dx, _cuda(c["grad"]), xt, Wt, fb, I, H, nl, M.RELU)
        if bb1 is not None:
            assert torch.equal(bb1[:, keep], bb0[:, keep]), "backward_buffer rows of other samples changed"
        if dx:
            assert torch.equal(gi1[keep], gi0[keep]), "grad_inputs rows of other samples changed"
        g = to_np(gw1).astype(np.float64)
        assert not np.isfinite(g[start + o * cols:start + (o + 1) * cols]).any(), f"row {o} of dW_out is not finite everywhere"
        worst = M.worst_ratio(g[finite], {"ref": q["ref"][finite], "bound": q["bound"][finite]}, f"{name} {rname} dx {dx}")
        print(f"\n{name} / {rname} / dx {dx}: {int((~np.isfinite(g)).sum())} non-finite weights, worst error / bound of the {int(finite.sum())} finite ones {worst:.3f}")


# ---------------------------------------------------------------- loop edges
def _loop_data(kind):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lc = M.loop_case(kind, cus)
    rng = np.random.default_rng(77)
    rows = M.loop_rows(lc, rng)
    B, I, H, nl = lc["B"], lc["I"], lc["H"], lc["nl"]
    gen = torch.Generator(device="cuda").manual_seed(11)
    xt = torch.randn(B, I, generator=gen, device="cuda").half()
    W = M.weights(I, H, nl, rng)
    g = (rng.standard_normal((rows.size, 16)) * 0.05).astype(np.float16)
    assert np.all(np.any(g != 0, axis=1))
    rt = torch.from_numpy(rows).cuda()
    gt = torch.zeros(B, 16, dtype=torch.float16, device="cuda")
    gt[rt] = _cuda(g)
    subset = np.union1d(rows, rng.choice(B, 2048, replace=False))
    c = dict(lc, name=f"loop_{kind}", W=W)
    return c, cus, rows, rt, g, subset, xt, _cuda(W), gt


def _loop_backward_checks(c, rname, rows, rt, g, subset, xt, Wt, gt, fb, worst, lib_option):
    I, H, nl, B = c["I"], c["H"], c["nl"], c["B"]
    _select(rname, I, H, nl, M.RELU, lib_option)
    Ws = M.split(c["W"], I, H, nl)
    er = M.emitting_route(rname)
    bb, gi, gw = _backward(er, True, gt, xt, Wt, fb, I, H, nl, M.RELU)
    zero = torch.ones(B, dtype=torch.bool, device="cuda")
    zero[rt] = False
    assert not bool(bb[:, zero].any()) and not bool(gi[zero].any()), "rows with a zero gradient have nonzero deltas or input gradients"
    st = torch.from_numpy(subset).cuda()
    gs, fbs, bbs, gis = to_np(gt[st]), to_np(fb[:, st]), to_np(bb[:, st]), to_np(gi[st])
    for k in range(nl):
        _note(worst, "bb", M.worst_ratio(bbs[k], M.delta(k, gs, fbs, bbs, Ws, M.RELU), f"{c['name']} bb[{k}]"))
    _note(worst, "grad_inputs", M.worst_ratio(gis, M.grad_inputs(bbs, Ws), f"{c['name']} grad_inputs"))
    q = M.grad_weights(to_np(xt[rt]), to_np(fb[:, rt]), to_np(bb[:, rt]), g, nl)          # every row with a nonzero gradient
    _note(worst, "grad_weights", M.worst_ratio(to_np(gw), q, f"{c['name']} grad_weights ({er})"))
    for dx in (True, False):
        if (rname == er and dx) or M.kernels(rname, I, H, nl, M.RELU, dx) is None:
            continue
        bb_r, gi_r, gw_r = _backward(rname, dx, gt, xt, Wt, fb, I, H, nl, M.RELU)
        assert bb_r is None or torch.equal(bb_r, bb)
        assert gi_r is None or torch.equal(gi_r, gi)
        _note(worst, "grad_weights", M.worst_ratio(to_np(gw_r), q, f"{c['name']} grad_weights ({rname}, dx {dx})"))


def _loop_test(kind, routes, lib_option):
    c, cus, rows, rt, g, subset, xt, Wt, gt = _loop_data(kind)
    assert c["B"] > c["grid"] * c["wg_rows"] + c["wg_rows"]
    worst = defaultdict(float)
    fb = _forward_checks(c, M.RELU, xt, Wt, M.split(c["W"], c["I"], c["H"], c["nl"]), worst, rows=subset)
    for rname in routes:
        _loop_backward_checks(c, rname, rows, rt, g, subset, xt, Wt, gt, fb, worst, lib_option)
    _report(f"loop {kind}: {cus} CUs, B = {c['B']}, {rows.size} rows with a gradient", worst)


def test_group_loop_of_the_fused_backward(lib_option):
    """B = 128 min(2 CUs, 1024) + 128 + 17: workgroups 0 and 1 of k_mlp_bwd_fused meet a second group, the last one ragged; the stored,
    recomputing, lean and planar instantiations."""
    _loop_test("fused", ("stored", "recompute", "lean", "planar"), lib_option)


def test_chunk_loop_of_the_split_k_weight_gradients(lib_option):
    """B = 64 ceil(8 CUs / ((nl + 1) GZ)) + 65: the workgroups of k_mlp_dw along x meet a second chunk."""
    _loop_test("dw", ("two_kernel",), lib_option)


def test_chunk_loop_of_the_deterministic_weight_gradients(lib_option):
    """FOC_DETERMINISTIC: 32 images, B = 64 * 32 + 65: images 0 and 1 take a second chunk, the slot images are summed in order."""
    _loop_test("dw_det", ("two_kernel_det",), lib_option)


def test_row_loop_of_the_two_kernel_backward(lib_option):
    """B = 256 * 4 CUs + 256 + 17: the workgroups of k_mlp_bwd meet a second pass (and k_mlp_dw many)."""
    _loop_test("bwd", ("two_kernel",), lib_option)


def test_row_loop_of_the_forward():
    """B = 128 * 8 CUs + 128 + 17 (8: the most 256-thread workgroups a CU can hold): k_mlp_fwd's workgroups meet a second pass in the
    training, inference, forward_buffer-free and planar forms."""
    c, cus, rows, rt, g, subset, xt, Wt, gt = _loop_data("forward")
    worst = defaultdict(float)
    _forward_checks(c, M.RELU, xt, Wt, M.split(c["W"], c["I"], c["H"], c["nl"]), worst, rows=subset)
    _report(f"loop forward: {cus} CUs, B = {c['B']}", worst)
