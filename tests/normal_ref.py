"""Float64 reference of the surface-normal kernel (csrc/normals.hip k_field_normals, include/focnerf.h foc_field_normals) and of
`focnerf_amd.normals.decode_normal_map`, ONE STAGE AT A TIME on operands the kernel wrote itself, a bound per element without a tuned
constant, and deliberately wrong variants (MUTANTS).

    dy_dx[b, l, d, c]  = scale_l * sum over the 4 corner pairs along d of (w_a w_b) (v_right - v_left)          (linear interpolation)
    grad_enc[b, 2l+c]  = d raw / d encoding: the gated transposed network applied to the one-hot gradient of output 0
    grad_raw[b, d]     = sum_{l, c} grad_enc[b, 2l+c] dy_dx[b, l, d, c]
    n                  = 0 where max|g| is 0 or a component is not finite, else -g / |g|;  n <- R n;  normal_rgb = 0.5 + 0.5 n
    decode             opacity = 1 - (white.r - black.r), sum w n = 2 black.rgb - opacity, normal = that sum at unit length (0 where it is 0)

The discrete decisions are the kernel's (tests/grid_backward_ref.py `level`): a point is in range when every coordinate lies in [0, 1];
the cell is the floor of the FLOAT32 position fmaf(x, scale, 0.5) with the level parameters of oracle.grid_level_params; the corner rows
come by the reference's index walk and hash. Everything behind that is float64: the in-cell fraction is the float64 position minus
that cell. A position within 2^-18 of an integer (not exactly on it) could put the two sides in different cells: `near_integer` (reused
from grid_backward_ref) must be 0 on every case, the builders redraw such points.

Bounds, counted from the rounding points csrc/normals.hip states in its header, by the magnitude rules of fixed_tail_ref.py (U = 2^-24;
an exact input carries 0; a product a b carries mag(a)|b| + |a|mag(b) + |ab|), with one refinement that keeps the bound meaningful at
the fine levels, where the one rounding of the position (U |pos|, |pos| up to 2048) is multiplied by scale^2: what the operands of a
reduction CARRY is counted once, and only the reduction's own roundings — one per product and at most T - 1 partial sums, each bounded by
the sum of the absolute terms — take the factor (T + K). bound = C U (carried + (T + K) sum|terms|) + (T + K) 2^-126, C = 2 (first order,
and an adder that truncates), K = 16:

    position   fmaf(x, scale, 0.5): one rounding, mag |pos|; the fraction f = pos - cell is then exact, u = (1 - f, f) carry mag(f) + |1 - f|, mag(f)
    dy_dx      fp32, NOT rounded to half: w = (scale u_a) u_b by the product rule (scale exact), v_right - v_left exact (two halves), the four
               terms w dv summed: mag(dy) = sum_4 mag(w)|dv| + (4 + 1) sum_4 |w dv| (the product's rounding and at most four additions)
    grad_enc   an input of the contraction (the kernel's own fp32 values, exact). Against the float64 network: mlp_ref's product bound
               E + 1/2 ulp_half(|s| + E) per layer (the deltas ARE rounded to half between layers; grad_enc itself is not, the bound's
               half-ulp term is kept as the issue sets mlp_ref's bound), chained through the layers the kernel does not emit by
               |W|^T bound(delta) (`chain_grad_enc`).
    grad_raw   32 terms: carried = sum_{l,c} |ge| mag(dy), bound C U (carried + (32 + K) sum_{l,c} |ge dy|) + (32 + K) 2^-126
    normal     from an exact g: g / m, three squares and two additions, sqrt, a division, the rotation's three products and two
               additions, the encoding's fma — fewer than K = 16 roundings of values of magnitude at most sqrt(3): C U K absolute. From a g
               with bound b: n = -g/|g| has the Jacobian -(I - n n^T)/|g|, so |dn_i| <= |dg|_2 / |g| <= sqrt(3) max_d b_d / |g| < 2 max_d b_d / |g|.
               Where that exceeds 1 the gradient is all rounding and only grad_raw is compared (`normal_bound` returns inf there).
"""
import numpy as np

import grid_backward_ref as G
import mlp_ref as M
from fixed_tail_ref import U
from ragged_ref import C as CC, K as KK, TINY

FOC14 = (3, 2, 16, 16, 14, 2048, 0, False, 0)        # the FOC grid with log2_hashmap_size 14: most levels hash, the table is small
MUTANTS = ("axis_swapped", "scale_dropped", "lc_transposed", "sign_flipped", "gates_ignored", "rotation_transposed", "wrong_norm", "oob_nonzero")


# ---------------------------------------------------------------- cases
def grid_case(name, spec, x):
    """A grid_backward_ref case for the points x [B, 3] (its gradient is not used here)."""
    x = np.ascontiguousarray(x, np.float32)
    L, C = spec[2], spec[1]
    return G.make_case(name, spec, x, np.zeros((L, x.shape[0], C), np.float16))


def settle(spec, x, redraw):
    """x with every point that has a (level, axis) within 2^-18 of an integer replaced by redraw(n) until none is left."""
    x = np.ascontiguousarray(x, np.float32).copy()
    for _ in range(40):
        bad = G.near_points(grid_case("settle", spec, x))
        if bad.size == 0:
            return x
        x[bad] = redraw(bad.size)
    raise AssertionError("settle: points near a cell boundary remain")


def points(rng, B, n_edge=True, n_out=4):
    """Uniform points, plus exact 0 and 1 on each axis, plus a few outside [0, 1] (as many as fit in B)."""
    x = rng.random((B, 3)).astype(np.float32)
    special = []
    if n_edge:
        for d in range(3):
            for v in (0.0, 1.0):
                p = rng.random(3).astype(np.float32)
                p[d] = v
                special.append(p)
    for k in range(n_out):
        p = rng.random(3).astype(np.float32)
        p[k % 3] = (-0.25, 1.5, -1e-6, 1.0000001)[k % 4]
        special.append(p)
    special = np.array(special, np.float32).reshape(-1, 3)[:max(B - 1, 0)]
    x[B - len(special):] = special
    return x, B - len(special)                                   # the points, and the number of plain uniform ones in front


# ---------------------------------------------------------------- dy_dx
def dy_dx(case, table, mutant=None):
    """float64 dy_dx [B, L, 3, 2] of `table` [rows, 2] with its magnitude (for an fp32 evaluation in the kernel's order); out-of-range points 0."""
    D, C, L, B = case["D"], case["C"], case["L"], case["B"]
    dy, mag = np.zeros((B, L, D, C)), np.zeros((B, L, D, C))
    t = np.asarray(table).astype(np.float64)
    k = np.arange(1 << D)
    for l in range(L):
        lv = G.level(case, l)
        u, mu, _ = G._axis_weights(case, lv)
        vals = t[lv["rows"] + int(case["off"][l])]                                    # [n, 8, C]
        scale = 1.0 if mutant == "scale_dropped" else float(lv["scale"])
        for d in range(D):
            a, b = [dd for dd in range(D) if dd != d]
            lo = k[((k >> d) & 1) == 0]                                              # the 4 corners with bit d clear, ascending
            ua, mua = u[:, a, :][:, (lo >> a) & 1], mu[:, a, :][:, (lo >> a) & 1]
            ub, mub = u[:, b, :][:, (lo >> b) & 1], mu[:, b, :][:, (lo >> b) & 1]
            w, mw = G._mul(scale * ua, scale * mua + np.abs(scale * ua), ub, mub)     # (scale u_a) u_b
            dv = vals[:, lo | (1 << d), :] - vals[:, lo, :]                           # [n, 4, C], exact in fp32
            terms = w[:, :, None] * dv
            dy[lv["idx"], l, d] = terms.sum(axis=1)
            mag[lv["idx"], l, d] = (mw[:, :, None] * np.abs(dv)).sum(axis=1) + 5.0 * np.abs(terms).sum(axis=1)
    if mutant == "oob_nonzero":
        out = ~np.all((case["x"] >= 0) & (case["x"] <= 1), axis=1)
        dy[out] = 1.0
    return dy, mag


# ---------------------------------------------------------------- contraction
def contract(grad_enc, dy, mag_dy, mutant=None):
    """grad_raw [B, 3] = sum_{l,c} grad_enc[b, 2l+c] dy[b, l, d, c] in float64 and its bound; grad_enc [B, 32] is an exact input."""
    ge = np.asarray(grad_enc, np.float64)
    B, L = dy.shape[0], dy.shape[1]
    g = ge.reshape(B, 2, L).transpose(0, 2, 1) if mutant == "lc_transposed" else ge.reshape(B, L, 2)
    d_ = dy[:, :, ::-1, :] if mutant == "axis_swapped" else dy
    terms = g[:, :, None, :] * d_
    with np.errstate(invalid="ignore", over="ignore"):
        gr = terms.sum(axis=(1, 3))
        T = 2 * L
        mag = (np.abs(g)[:, :, None, :] * mag_dy).sum(axis=(1, 3)) + (T + KK) * np.abs(terms).sum(axis=(1, 3))
    return gr, CC * U * mag + (T + KK) * TINY


# ---------------------------------------------------------------- normalisation, rotation, encoding
def normalise(g, mutant=None):
    """n [B, 3] float64: 0 where max|g| is 0 or a component is not finite, else -g / |g| (scaled by the largest component first)."""
    g = np.asarray(g, np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.max(np.abs(g), axis=-1, keepdims=True)
        ok = np.isfinite(g).all(axis=-1, keepdims=True) & (m > 0)
        u = g / np.where(ok, m, 1.0)
        norm = np.abs(u).sum(axis=-1, keepdims=True) if mutant == "wrong_norm" else np.sqrt((u * u).sum(axis=-1, keepdims=True))
        n = (1.0 if mutant == "sign_flipped" else -1.0) * u / np.where(ok, norm, 1.0)
    return np.where(ok, n, 0.0)


def encode(n, rotation=None, mutant=None):
    """normal_rgb = 0.5 + 0.5 (R n), R the float32 coefficients the kernel was given (exact inputs), in float64."""
    n = np.asarray(n, np.float64)
    if rotation is not None:
        R = np.asarray(rotation, np.float32).astype(np.float64).reshape(3, 3)
        n = n @ (R if mutant == "rotation_transposed" else R.T)
    return 0.5 + 0.5 * n


def normal_bound(g, bound_g):
    """Bound of every component of n for a gradient known to bound_g [B, 3] (0: exact): 2 max_d bound_g / |g| + C U K; inf where the
    first term exceeds 1 (a gradient that is all rounding) and for a zero / non-finite gradient whose bound is not 0."""
    g, bg = np.asarray(g, np.float64), np.max(np.broadcast_to(np.asarray(bound_g, np.float64), np.shape(g)), axis=-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((g * g).sum(axis=-1))
        rel = np.where(bg == 0, 0.0, 2.0 * bg / length)
    rel = np.where(np.isfinite(rel) & (rel <= 1.0), rel, np.inf)
    return (rel + CC * U * KK)[:, None] * np.ones(3)


def rgb_bound(nb):
    """normal_rgb = fma(0.5, n, 0.5): half the normal's bound and the fma's own rounding of a value in [0, 1]."""
    return 0.5 * nb + U


# ---------------------------------------------------------------- grad_enc against the float64 network, layer by layer
def chain_grad_enc(fb, W, nl, mutant=None):
    """d out[0] / d input [B, 32] of the I = 32, H = 64 network `W` (half blob) from the kernel's own forward activations fb [nl, B, 64]:
    mlp_ref's deltas for the one-hot gradient of output 0 and its grad_inputs, each layer's bound chained into the next by |W|^T bound
    (the kernel emits no delta: its half delta may be any value inside the bound). -> dict(ref, bound)."""
    Ws = M.split(W, 32, 64, nl)
    B = fb.shape[1]
    grad = np.zeros((B, 16))
    grad[:, 0] = 1.0
    act = M.NONE if mutant == "gates_ignored" else M.RELU
    q = M.delta(0, grad, fb, None, Ws, act)                                  # one product per element: exact, a half weight
    ref, carried = q["ref"], np.zeros_like(q["ref"])
    for k in range(1, nl):
        fl = nl - 1 - k
        Wm = Ws[fl + 1].T                                                    # [in, out]
        q = M.product(ref, Wm)
        extra = carried @ np.abs(Wm).T
        mask = (np.asarray(fb[fl], np.float64) > 0) if act == M.RELU else np.ones_like(q["ref"], bool)
        ref = np.where(mask, q["ref"], 0.0)
        carried = np.where(mask, q["bound"] + extra, 0.0)
    q = M.product(ref, Ws[0].T)
    return dict(ref=q["ref"], bound=q["bound"] + carried @ np.abs(Ws[0].T).T)


def network64(x, W, nl, mutant=None):
    """The chained float64 network on inputs x [B, 32] with its OWN activations and gates (for exactly representable data):
    -> raw [B] (output 0), grad_enc [B, 32]."""
    Ws = M.split(W, 32, 64, nl)
    a, acts = np.asarray(x, np.float64), []
    for l in range(nl):
        a = np.maximum(a @ Ws[l].T, 0.0)
        acts.append(a)
    raw = (a @ Ws[nl].T)[:, 0]
    d = np.broadcast_to(Ws[nl][0], a.shape) * ((acts[nl - 1] > 0) if mutant != "gates_ignored" else 1.0)
    for l in range(nl - 1, 0, -1):
        d = (d @ Ws[l]) * ((acts[l - 1] > 0) if mutant != "gates_ignored" else 1.0)
    return raw, d @ Ws[0]


# ---------------------------------------------------------------- decode, select + composite
def decode_normal_map(image4_pair):
    """focnerf_amd.normals.decode_normal_map in float64 numpy: -> normal [N, 3], opacity [N]."""
    white, black = np.asarray(image4_pair[0], np.float64), np.asarray(image4_pair[1], np.float64)
    opacity = 1.0 - (white[:, 0] - black[:, 0])
    s = 2.0 * black[:, :3] - opacity[:, None]
    length = np.sqrt((s * s).sum(axis=-1))
    ok = (opacity > 0) & (length > 0)
    return np.where(ok[:, None], s / np.where(ok, length, 1.0)[:, None], 0.0), opacity


def composite(fields4, nears, fars, bgs=(1.0, 0.0)):
    """Select + fixed-step composite of packed fields [K][N, T, 4] (float32, the kernels' own) in float64, by attribution_ref's statement
    of the combiner: the strict-'>' select in field order, the weights on oracle.composite_fixed_steps' float32 sample positions.
    -> image [len(bgs), N, 3] (not clamped), weights_sum [N], winner [N, T]."""
    import attribution_ref as A
    F = np.stack([np.asarray(f, np.float32) for f in fields4])               # [K, N, T, 4]
    win, src, merged = A.winner(F[..., 0])
    w, _ = A.weights(merged, np.asarray(nears, np.float32), np.asarray(fars, np.float32))
    rgb = np.take_along_axis(F[..., 1:].astype(np.float64), src[None, :, :, None], axis=0)[0]
    ws = w.sum(axis=1)
    acc = (w[:, :, None] * rgb).sum(axis=1)
    return np.stack([acc + (1.0 - ws)[:, None] * bg for bg in bgs]), ws, win


def composite_bound(T):
    """Bound of an fp32 composite's image channels and weights_sum against `composite`: a weight is alpha_i times i factors
    (1 - alpha_j + 1e-15), each factor two roundings and the product one, alpha an exp of a rounded argument (a e^-a U <= U / e) and a
    subtraction: relative (3 i + K) U at most, so sum_i |dw_i| <= (3 T + K) U sum w <= (3 T + K) U; colours lie in [0, 1] and the sums'
    own roundings are covered by C. The decoded sum 2 black - opacity carries 2 + 2 of these."""
    return CC * U * (3 * T + KK)
