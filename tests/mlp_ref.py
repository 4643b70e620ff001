"""Float64 reference of the fully fused MLP (csrc/ffmlp.hip k_mlp_fwd, k_mlp_bwd, k_mlp_dw, k_mlp_bwd_fused, k_mlp_dw_reduce and the
finalize kernels; csrc/ffmlp_wide.hip k_wide_layer; csrc/mlp_common.h), ONE LAYER AT A TIME on the operands the kernel itself read, a
bound per element without a tuned constant, the cases, the route table, and a numpy fp32 model of the weight-gradient routes with
deliberately wrong variants (MUTANTS).

Why one layer at a time: every layer rounds to half once, and a pre-activation within the fp32 error of a rounding boundary or of zero
lands on the other half or on the other side of the ReLU (~0.4 % of the elements), so a float64 network that carries its own
activations cannot be compared element by element. Nothing here chains: every quantity is the exact float64 result of one matrix
product of arrays the kernel was given or wrote itself (inputs, weights, its forward_buffer `fb`, its backward_buffer `bb`, grad).

Layouts (oracle/oracle.c orc_ffmlp_forward / orc_ffmlp_backward, csrc/ffmlp.hip k_mlp_dw): the blob is
[W0: H x I | (nl - 1) x H x H | W_out: 16 x H], every matrix row-major with neuron = row; fb[l] is the post-activation output of forward
layer l; bb[k] is the delta of forward layer nl - 1 - k; planar inputs and planar input gradients are [I / 2, B, 2].

    forward layer l   s = sum_k W_l[n, k] in_l[b, k], in_0 = x, in_l = fb[l - 1];  fb[l][b, n] = act(half(s)); ReLU (0) and None (6).
                      ReLU is 1-Lipschitz: compared with max(s, 0) under the bound of s.
    output            out[b, o] = half(sum_n W_out[o, n] fb[nl - 1][b, n])
    deltas            bb[0][b, n] = [fb[nl - 1][b, n] > 0] half(sum_o grad[b, o] W_out[o, n])
                      bb[k][b, n] = [fb[nl - 1 - k][b, n] > 0] half(sum_m bb[k - 1][b, m] W[m, n]), W the matrix fb[nl - 1 - k] -> fb[nl - k];
                      the mask comes from the fb the call was given; activation None: every mask is 1
    grad_inputs       [b, i] = half(sum_n bb[nl - 1][b, n] W0[n, i])
    grad_weights      dW_j[o, i] = half(sum_b D_j[b, o] A_j[b, i]); (D, A) = (bb[nl - 1], x) for the input layer, (bb[nl - 1 - j], fb[j - 1])
                      for hidden matrix j, (grad, fb[nl - 1]) for the output matrix

The bound, per element
----------------------
Every product of two halves is exact in fp32 (22 significant bits, exponents from 2^-48), so the only errors are the fp32 additions
and the final rounding to half. U = 2^-24, m the number of NONZERO products of the element, sum|t| their absolute sum (adding an
exact zero is exact in any summation tree: rows past B, masked deltas, zero activations carry nothing):

    E     = C U max(m - 1, 0) sum|t|
    bound = E + 1/2 ulp_half(|s| + E)              ulp_half is 2^-24 below 2^-14: subnormal halves must come through unflushed

C = 1 is the any-order bound of round-to-nearest additions (each of the m - 1 additions errs by at most U times its own partial sum,
which is at most sum|t|, to first order). C = 2 covers an adder that truncates (one ulp per addition): what the matrix cores do inside
v_mfma_f32_32x32x16_f16 is not documented; depth_ref.py makes the same choice. An element with no nonzero product has bound 0 and
must be exactly 0; a masked delta likewise. NaN where the reference is finite is outside.

The bound grows with the number of rows that carry a nonzero gradient (E / (half an ulp of a sum of B random terms) ~ sqrt(B) / 2^12
times C): an fp32 emulation of the slot route has worst error / bound 0.94 at B = 333 and 0.33 at B = 4096, and a dropped row puts
>= 97 % of the elements it touches outside at B <= 1000 but only 76 - 90 % at B = 4096. The weight-gradient cases therefore keep the rows
with a nonzero gradient at or below MAX_NONZERO_ROWS; larger batches carry exact zeros everywhere else.

Forms whose intermediates never leave the chip (inference, the forward_buffer = NULL forward, the planar forward, the recomputing
backward, the lean backward, the planar backward) inherit from the form that emits them: the GPU test asserts identical bits of out,
grad_inputs and backward_buffer on the same data and bounds the form's grad_weights against the float64 sum built from the emitting
form's fb / bb.

Routes: `ROUTES`, `kernels()` restates the selection of csrc/ffmlp.hip mlp_bwd_launch / mlp_bwd_fused_launch / mlp_bwd_entry. `PLAN`
maps every case to the routes it runs on. Loop-edge batch sizes (`loop_case`) are computed from the number of compute units.

Hidden activations 1..5 (exponential, sine, sigmoid, squareplus, softplus) are measured layer by layer in the same way by
tests/pointwise_ref.py and tests/test_gpu_pointwise_reference.py, which build on this module's `product`, `delta`, `grad_inputs` and
`grad_weights`: the float64 sum names the half (or halves) the activation saw, the activation has a bound of its own.

Out of scope: the colour-head and whole-field forms (foc_color_head_*, foc_field_forward_train*, foc_nerf_field_inference*: they emit
no intermediates and existing tests pin them bit for bit, on integer data, to the plain MLP on the materialised input — which is what
is measured here; the SH half-row of the whole-field kernel is observed by test_gpu_pointwise_reference.py), and performance.
"""
import math

import numpy as np

U = 2.0 ** -24
C = 2.0
HALF_MAX = 65504.0
HALF_OVER = 65520.0                  # the first value that rounds to inf
RELU, NONE = 0, 6
MAX_NONZERO_ROWS = 1000

# csrc/ffmlp.hip: rows per workgroup and pass of the kernels, the deterministic image count, the slot cap of the fused backward
FUSED_ROWS, BWD_ROWS, FWD_ROWS, DW_CHUNK, DW_DET_SLOTS, DW_MAX_SLOTS, DW_WGS_PER_CU = 128, 256, 128, 64, 32, 1024, 8

SHAPES = [(32, 64, 2), (32, 64, 3), (16, 16, 2), (48, 32, 4), (64, 64, 1), (64, 128, 2), (32, 256, 2), (144, 32, 3), (256, 128, 2),
          (16, 16, 1), (48, 32, 1), (64, 128, 1)]                    # + one hidden layer at every width that has those kernels
BATCHES = (1, 31, 33, 63, 65, 127, 129, 257, 333, 1000)
SCALE_SHAPES = [(32, 64, 2), (64, 128, 2)]
SCALES = (-16, -8, 0, 8)


# ---------------------------------------------------------------- layout
def n_params(I, H, nl):
    return H * (I + H * (nl - 1) + 16)


def offsets(I, H, nl):
    """(start, rows, cols) of W0, the hidden matrices and W_out in the blob."""
    out, o = [(0, H, I)], H * I
    for _ in range(nl - 1):
        out.append((o, H, H)); o += H * H
    out.append((o, 16, H))
    return out


def split(W, I, H, nl):
    """The blob's matrices as float64 [rows, cols]: [W0, hidden 1 .. nl - 1, W_out]; hidden matrix j maps fb[j - 1] -> fb[j]."""
    W = np.asarray(W)
    return [W[o:o + r * c].reshape(r, c).astype(np.float64) for o, r, c in offsets(I, H, nl)]


# ---------------------------------------------------------------- the bound
def ulp_half(v):
    """Spacing of the halves around magnitude v >= 0 (2^-24 below 2^-14; the binade's own spacing above the largest half too)."""
    _, e = np.frexp(np.maximum(v, 2.0 ** -14))                      # v in [2^(e-1), 2^e)
    return np.ldexp(1.0, e - 11)


def product(A, Bm):
    """s[a, b] = sum_k A[a, k] Bm[b, k] in float64 with its bound, sum|t| and the number of nonzero products."""
    A, Bm = np.asarray(A, np.float64), np.asarray(Bm, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = A @ Bm.T
        mag = np.abs(A) @ np.abs(Bm).T
        m = (A != 0).astype(np.float64) @ (Bm != 0).astype(np.float64).T
        E = np.where(m > 1, C * U * (m - 1) * mag, 0.0)
        b = np.where(m > 0, E + 0.5 * ulp_half(np.abs(s) + E), 0.0)
    return dict(ref=s, bound=b, mag=mag, count=m)


def forward_layer(l, x, fb, Ws, act):
    """fb[l] from the kernel's own operands: x (l = 0) or fb[l - 1]."""
    q = product(x if l == 0 else fb[l - 1], Ws[l])
    if act == RELU:
        q["ref"] = np.maximum(q["ref"], 0.0)
    return q


def output(fb, Ws):
    return product(fb[-1], Ws[-1])


def delta(k, grad, fb, bb, Ws, act):
    """bb[k] from grad (k = 0) or bb[k - 1], masked by fb[nl - 1 - k] > 0 under ReLU; a masked element has bound 0."""
    nl = len(Ws) - 1
    fl = nl - 1 - k
    q = product(grad if k == 0 else bb[k - 1], Ws[-1].T if k == 0 else Ws[fl + 1].T)
    if act == RELU:
        mask = np.asarray(fb[fl], np.float64) > 0
        q = {n: np.where(mask, v, 0.0) for n, v in q.items()}
    return q


def grad_inputs(bb, Ws):
    return product(bb[len(Ws) - 2], Ws[0].T)


def dw_operands(j, x, fb, bb, grad, nl):
    """(D, A) of blob matrix j (0 input layer, 1 .. nl - 1 hidden, nl output)."""
    if j == nl:
        return grad, fb[nl - 1]
    return bb[nl - 1 - j], (x if j == 0 else fb[j - 1])


def grad_weights(x, fb, bb, grad, nl, rows=None):
    """The whole gradient blob (flat, the blob's order): ref, bound, mag, count. `rows`: the rows that may carry a nonzero delta (every
    other row of D is an exact zero and adds nothing)."""
    parts = []
    for j in range(nl + 1):
        D, A = dw_operands(j, x, fb, bb, grad, nl)
        D, A = np.asarray(D), np.asarray(A)
        if rows is not None:
            D, A = D[rows], A[rows]
        parts.append(product(D.T, A.T))
    return {n: np.concatenate([p[n].reshape(-1) for p in parts]) for n in parts[0]}


def worst_ratio(got, q, what=""):
    """max |got - ref| / bound over every element; raises where an element is outside, NaN included, or where a bound-0 element is not 0."""
    got = np.asarray(got).astype(np.float64)
    ref, bound = np.broadcast_to(q["ref"], got.shape), np.broadcast_to(q["bound"], got.shape)
    zero = bound == 0
    assert np.all(got[zero] == 0), f"{what}: {int((got[zero] != 0).sum())} elements with no nonzero product (or masked) are not exactly 0"
    sel = ~zero
    if not sel.any():
        return 0.0
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got - ref)[sel] / bound[sel]
    bad = ~(ratio <= 1.0)
    worst = float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(sel.sum())} elements outside the bound, worst error / bound {worst:.3f}"
    return worst


# ---------------------------------------------------------------- routes
ROUTES = {
    # name: fused = the call may take k_mlp_bwd_fused; det = FOC_DETERMINISTIC; fb / bb = buffers handed to the call; planar inputs
    "stored": dict(fused=True, det=0, fb=True, bb=True, planar=False),
    "recompute": dict(fused=True, det=0, fb=False, bb=True, planar=False),
    "lean": dict(fused=True, det=0, fb=False, bb=False, planar=False),
    "planar": dict(fused=True, det=0, fb=False, bb=False, planar=True),
    "two_kernel": dict(fused=False, det=0, fb=True, bb=True, planar=False),
    "two_kernel_det": dict(fused=False, det=1, fb=True, bb=True, planar=False),
    "hidden256": dict(fused=False, det=0, fb=True, bb=True, planar=False),
    "hidden256_det": dict(fused=False, det=1, fb=True, bb=True, planar=False),
    "wide_input": dict(fused=False, det=0, fb=True, bb=True, planar=False),
}
# the rows of the issue's route table -> the routes that stand for them
TABLE = {"stored, single pass": ("stored",), "recompute": ("recompute",), "lean": ("lean",), "planar": ("planar",), "two-kernel": ("two_kernel",),
         "two-kernel, deterministic": ("two_kernel_det",), "hidden 256": ("hidden256", "hidden256_det"), "wide input": ("wide_input",)}


def single_pass(I, H, nl, act):
    return H <= 64 and I <= 64 and 1 <= nl <= 4 and act in (RELU, NONE)


def fused_option(rname, I, H, nl, act):
    """Value of FOC_MLP_BWD_FUSED on the route: 0 only where the shape would otherwise take the single pass (every other route selects
    itself by its shape)."""
    return 0 if (not ROUTES[rname]["fused"] and single_pass(I, H, nl, act)) else 1


def kernels(rname, I, H, nl, act, dx):
    """The kernels a foc_ffmlp_backward / _backward_planar call launches on this route (csrc/ffmlp.hip mlp_bwd_launch and below), or None
    where the route does not serve the shape."""
    r = ROUTES[rname]
    relu = act == RELU
    if rname.startswith("hidden256"):
        return ("k_wide_layer", "k_mlp_dw<256>", "k_mlp_dw_finalize_slots" if r["det"] else "k_mlp_dw_finalize") if H == 256 and nl >= 2 else None
    if H == 256:
        return None
    if rname == "wide_input":
        return ("k_mlp_bwd", f"k_mlp_dw<{H},256>" if I > 128 else f"k_mlp_dw<{H}>", "k_mlp_dw_finalize") if I > 64 else None
    if r["fused"]:
        if not single_pass(I, H, nl, act):
            return None
        recomp = not r["fb"]
        in32 = H == 64 and recomp and relu and I <= 32
        lean = in32 and not r["bb"] and dx
        if rname == "lean" and not lean:
            return None
        if rname == "recompute" and not recomp:
            return None
        form = f"RECOMP={'true' if recomp else 'false'}, IMODE={int(r['planar'])}" + (", IN32" if in32 else "") + (", LEAN" if lean else "")
        return (f"k_mlp_bwd_fused<{H}, {nl}, {form}>", "k_mlp_dw_reduce")
    if I > 64:
        return None                                      # that is the wide-input route
    return ("k_mlp_bwd", f"k_mlp_dw<{H}>", "k_mlp_dw_finalize_slots" if r["det"] else "k_mlp_dw_finalize")


def routes_for(I, H, nl, act):
    """Every route that serves the shape and activation (with input gradients; `lean` has no form without them)."""
    return [n for n in ROUTES if kernels(n, I, H, nl, act, True) is not None]


def emitting_route(rname):
    """The route whose fb / bb a form without intermediates inherits."""
    return "stored" if rname in ("recompute", "lean", "planar") else rname


# ---------------------------------------------------------------- data
def weights(I, H, nl, rng):
    return (rng.uniform(-1, 1, n_params(I, H, nl)) * math.sqrt(3 / H)).astype(np.float16)


def make_case(name, I, H, nl, B, scale, seed, kind="random"):
    """x [B, I], W, grad [B, 16] in half. kind: 'random'; 'cancel' (rows b and b + B / 2 have the same x and gradients g, -g); 'overflow'
    (|g| = 60000 in output column 0 of every row); 'nonfinite' (one inf at grad[inf_row, inf_col]; `grad_finite` is the same without)."""
    rng = np.random.default_rng(seed)
    W = weights(I, H, nl, rng)
    x = rng.standard_normal((B, I)).astype(np.float16)
    g = (rng.standard_normal((B, 16)) * scale).astype(np.float16)
    extra = {}
    if kind == "cancel":
        assert B % 2 == 0 and (B // 2) % 128            # the two rows of a pair lie in different 64-row chunks and 128-row groups:
        x[B // 2:] = x[:B // 2]                           # their products meet as rounded partial sums, not inside one MFMA
        g[B // 2:] = -g[:B // 2]
    elif kind == "overflow":
        g[:, 0] = np.float16(60000.0)
    elif kind == "nonfinite":
        extra = dict(inf_row=B // 2 + 3, inf_col=5, grad_finite=g.copy())
        g[extra["inf_row"], extra["inf_col"]] = np.float16(np.inf)
    return dict(name=name, I=I, H=H, nl=nl, B=B, scale=scale, kind=kind, x=x, W=W, grad=g, **extra)


def shape_name(I, H, nl):
    return f"{I}x{H}x{nl}"


BUILDERS = {}
for _I, _H, _nl in SHAPES:
    for _B in BATCHES:
        BUILDERS[f"shape_{shape_name(_I, _H, _nl)}_B{_B}"] = (_I, _H, _nl, _B, 0.05, 1000 + _I + _H + _nl + _B, "random")
for _I, _H, _nl in SCALE_SHAPES:
    for _s in SCALES:
        BUILDERS[f"scale_{shape_name(_I, _H, _nl)}_2^{_s}"] = (_I, _H, _nl, 333, 2.0 ** _s, 2000 + _H + _s, "random")
    BUILDERS[f"cancel_{shape_name(_I, _H, _nl)}"] = (_I, _H, _nl, 666, 0.05, 3000 + _H, "cancel")
    BUILDERS[f"overflow_{shape_name(_I, _H, _nl)}"] = (_I, _H, _nl, 256, 0.05, 4000 + _H, "overflow")
    BUILDERS[f"nonfinite_{shape_name(_I, _H, _nl)}"] = (_I, _H, _nl, 333, 0.05, 5000 + _H, "nonfinite")
BUILDERS["overflow_32x256x2"] = (32, 256, 2, 256, 0.05, 4256, "overflow")
BUILDERS["nonfinite_32x256x2"] = (32, 256, 2, 333, 0.05, 5256, "nonfinite")
BUILDERS["nonfinite_144x32x3"] = (144, 32, 3, 333, 0.05, 5032, "nonfinite")
_BUILT = {}


def case(name):
    if name not in _BUILT:
        _BUILT[name] = make_case(name, *BUILDERS[name])
    return _BUILT[name]


def names(prefix=""):
    return [n for n in BUILDERS if n.startswith(prefix)]


def acts_for(rname):
    """Both activations go through every route that has both instantiations; the lean form is built for ReLU."""
    return (RELU,) if rname == "lean" else (RELU, NONE)


# case -> routes (both activations where acts_for says so; with and without input gradients)
PLAN = {n: tuple(routes_for(*BUILDERS[n][:3], RELU)) for n in BUILDERS}


# ---------------------------------------------------------------- loop edges
def loop_case(kind, cus):
    """Batch size, shape and route at which a persistent kernel's workgroups meet rows a second time, from the number of compute units
    (the grids of csrc/ffmlp.hip: mlp_bwd_fused_launch, mlp_dw_launch, mlp_bwd_launch, mlp_fwd_launch). `wg_rows` rows per workgroup and
    pass, `grid` workgroups, `tile` the wave tile."""
    if kind == "fused":
        I, H, nl, rname = 32, 64, 2, "stored"
        grid, wg_rows, tile = min(2 * cus, DW_MAX_SLOTS), FUSED_ROWS, 32
        B = wg_rows * grid + 128 + 17
    elif kind in ("dw", "dw_det"):
        I, H, nl = 64, 128, 2
        rname = "two_kernel" if kind == "dw" else "two_kernel_det"
        gz = (((H + 31) // 32) * ((max(H, I) + 31) // 32) + 15) // 16
        grid = -(-DW_WGS_PER_CU * cus // ((nl + 1) * gz)) if kind == "dw" else DW_DET_SLOTS
        wg_rows, tile = DW_CHUNK, 16
        B = wg_rows * grid + 65
    elif kind == "bwd":
        I, H, nl, rname = 64, 128, 2, "two_kernel"
        grid, wg_rows, tile = 4 * cus, BWD_ROWS, 64
        B = wg_rows * grid + 256 + 17
    elif kind == "forward":
        I, H, nl, rname = 32, 64, 2, None
        grid, wg_rows, tile = 8 * cus, FWD_ROWS, 32          # 8: the most 256-thread workgroups a CU can hold
        B = wg_rows * grid + 128 + 17
    else:
        raise KeyError(kind)
    return dict(kind=kind, I=I, H=H, nl=nl, route=rname, grid=grid, wg_rows=wg_rows, tile=tile, B=B)


LOOPS = ("fused", "dw", "dw_det", "bwd", "forward")


def loop_rows(lc, rng, n_random=160, budget=600):
    """Rows that carry a nonzero gradient: the first and last row, both sides of the workgroup and tile boundaries (of every workgroup
    where the grid is small, else of the first and last three of the first pass), the ragged tail, rows the workgroups meet on their
    second pass, and random rows. At most `budget`."""
    B, wg, tile, grid = lc["B"], lc["wg_rows"], lc["tile"], lc["grid"]
    rows = {0, B - 1}
    wgs = range(grid + 1) if grid <= 40 else list(range(0, 3)) + list(range(grid - 3, grid + 1))
    for w in wgs:
        for r in (w * wg - 1, w * wg, w * wg + tile - 1, w * wg + tile):
            if 0 <= r < B:
                rows.add(r)
    second = np.arange(grid * wg, B)                                 # every workgroup's second pass starts here
    tail = np.arange(B - (B % tile) - 1, B)
    rows |= set(tail.tolist())
    room = budget - len(rows) - n_random
    if second.size > room:                                           # tile edges of the second pass, then an even spread
        edges = [r for r in second if (r - grid * wg) % tile in (0, tile - 1)]
        rows |= set(edges)
        left = budget - len(rows) - n_random
        rows |= set(second[np.linspace(0, second.size - 1, max(left, 0)).astype(np.int64)].tolist()) if left > 0 else set()
    else:
        rows |= set(second.tolist())
    rows |= set(rng.choice(B, n_random, replace=False).tolist())
    rows = np.array(sorted(rows), np.int64)
    assert rows.size <= budget + 8
    return rows


# ---------------------------------------------------------------- numpy fp32 model of the weight-gradient routes
MUTANTS = ("drop_ragged_last_row", "drop_second_pass", "slot0_twice", "skip_slots_from_512", "delta_before_mask", "flush_subnormal_delta",
           "truncate_final", "fb_l_for_fb_l_minus_1")
ORDERS = ("slots", "chunks_shuffled", "images")


def _f32_outer_sum(D, A, rows):
    """sum over `rows` (in that order) of D[r]^T A[r]: fp32 products (exact) and fp32 additions, one row at a time."""
    acc = np.zeros((D.shape[1], A.shape[1]), np.float32)
    for r in rows:
        acc = acc + np.outer(D[r].astype(np.float32), A[r].astype(np.float32))
    return acc


def _round_half(v32, truncate=False):
    if not truncate:
        with np.errstate(over="ignore"):
            return v32.astype(np.float16)
    v = np.ascontiguousarray(v32, np.float32)
    with np.errstate(over="ignore"):
        h = v.astype(np.float16)
    up = np.abs(h.astype(np.float32)) > np.abs(v)                       # rounded away from zero: step back towards it
    return np.where(up, np.nextafter(h, np.float16(0)), h)


def model_dw(D, A, order, mutant=None, grid=None, seed=0):
    """dW = D^T A [OUT, IN] in half as one weight-gradient route sums it. 'slots': 128-row partials of k_mlp_bwd_fused (workgroup w takes
    the groups w, w + grid, ... into ONE slot), the slots added by k_mlp_dw_reduce (16 slices of every 16th slot, four running sums each,
    then the slices in order); 'chunks_shuffled': k_mlp_dw's 64-row chunks as fp32 atomics in a shuffled order; 'images':
    FOC_DETERMINISTIC, chunk c into image c mod 32, the images in order."""
    B = D.shape[0]
    live = np.nonzero(np.any(D != 0, axis=1))[0]
    if mutant == "drop_ragged_last_row" and B % 32:
        live = live[live != B - 1]
    if order == "slots":
        n_groups = -(-B // FUSED_ROWS)
        grid = min(n_groups, DW_MAX_SLOTS) if grid is None else min(grid, n_groups)
        slot_rows = {}
        for r in live:
            g = r // FUSED_ROWS
            if mutant == "drop_second_pass" and g >= grid:
                continue
            slot_rows.setdefault(g % grid, []).append(r)
        part = {s: _f32_outer_sum(D, A, rr) for s, rr in slot_rows.items()}
        zero = np.zeros((D.shape[1], A.shape[1]), np.float32)
        if mutant == "slot0_twice" and 0 in part:
            part[0] = part[0] + part[0]
        if mutant == "skip_slots_from_512":
            part = {s: p for s, p in part.items() if s < 512}
        slices = []
        for sl in range(16):
            a = [zero.copy() for _ in range(4)]
            g = sl
            while g + 48 < grid:
                for q in range(4):
                    if g + 16 * q in part:
                        a[q] = a[q] + part[g + 16 * q]
                g += 64
            while g < grid:
                if g in part:
                    a[0] = a[0] + part[g]
                g += 16
            slices.append((a[0] + a[1]) + (a[2] + a[3]))
        v = zero.copy()
        for s in slices:
            v = v + s
    else:
        n_chunks = -(-B // DW_CHUNK)
        by_chunk = {}
        for r in live:
            by_chunk.setdefault(r // DW_CHUNK, []).append(r)
        part = {c: _f32_outer_sum(D, A, rr) for c, rr in by_chunk.items()}
        v = np.zeros((D.shape[1], A.shape[1]), np.float32)
        if order == "chunks_shuffled":
            ids = list(part)
            np.random.default_rng(seed).shuffle(ids)
            for c in ids:
                v = v + part[c]
        else:
            gx = min(n_chunks, DW_DET_SLOTS)
            for im in range(gx):
                acc = np.zeros_like(v)
                for c in range(im, n_chunks, gx):
                    if c in part:
                        acc = acc + part[c]
                v = v + acc
    return _round_half(v, truncate=mutant == "truncate_final")


def model_delta(k, grad, fb, bb, Ws, act, mutant=None):
    """bb[k] in half from the same operands: fp32 sums in k order, rounded to half, masked."""
    nl = len(Ws) - 1
    fl = nl - 1 - k
    src = (grad if k == 0 else bb[k - 1]).astype(np.float32)
    Wm = (Ws[-1].T if k == 0 else Ws[fl + 1].T).astype(np.float32)
    acc = np.zeros((src.shape[0], Wm.shape[0]), np.float32)
    for kk in range(src.shape[1]):
        acc = acc + src[:, kk:kk + 1] * Wm[None, :, kk]
    d = _round_half(acc, truncate=mutant == "truncate_final")
    if mutant == "flush_subnormal_delta":
        d = np.where(np.abs(d.astype(np.float32)) < 2.0 ** -14, np.float16(0), d)
    if act == RELU and mutant != "delta_before_mask":
        d = np.where(fb[fl] > 0, d, np.float16(0))
    return d
