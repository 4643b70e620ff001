"""Float64 reference of the background model (csrc/background.hip), the per-element error bounds its tolerances need, and the cases the
CPU and GPU tests share.

    bg = sigmoid(W1 . relu(W0 . [SH16(d) | grid8((coords + 1) / 2)]))          W0 [64,24], W1 [3,64], no biases

The operation
-------------
Where a sample lies is fp32 by definition (gridencoder.cu:100-135): u = (c + 1) / 2, p = fmaf(u, scale, 0.5), floor, the fraction and the
four corner weights w = 1 * (fx | 1 - fx) * (fy | 1 - fy) are formed here with the same single correctly rounded fp32 operations (numpy
float32; fmaf(a, b, c) = float32(float64(a) * float64(b) + float64(c))). At level 3 an fp32 position resolves 2^-13 of a cell: a float64
position is another sample. The level scale is exp2f(l * S) * H - 1 and the resolution ceil(scale) + 1 (gridencoder.cu:138-139). A
corner's row follows gridencoder.cu:50-84: index = sum p_d * stride_d while stride_d <= size (stride_0 = 1, stride_{d+1} = stride_d *
(resolution + 1)); if the last stride overran the size, index = px ^ py * 2654435761 in uint32; then index % size. A point with u or v
outside [0,1] has a zero grid part and takes no table gradient.

Everything after that is float64 — the corner sums, the SH polynomials, both layers, the sigmoid, every backward product and sum — with a
rounding to fp16 exactly where the operation has one under fp16 autocast: table values on load, the SH values, each level's pair, each
layer's output (ReLU on the rounded value), the sigmoid, g2 = g (1 - y) y, gz = [a > 0] half(W1^T g2), and the grid columns of the input
gradient W0[:,16:]^T gz. `half=False, pos32=False` switches every rounding off (the smooth chain that autograd can differentiate).

The error model (`bounds()`)
----------------------------
E(q) bounds |q_kernel - q_reference| and is carried through the chain to first order (second-order terms are added where a factor's own
E can reach an fp16 ulp). U = 2^-24.

  * An fp32 fma chain over n products: n U sum |products| (any order of association). n = 4 (corner sum), 24 (layer 0), 64 (layer 1),
    3 (W1^T g2), 64 (the grid columns), and for dW: the rays a workgroup sums (64 per chunk, chunk after chunk) plus the G workgroup
    partials that k_bg_dw_reduce adds: (64 ceil(chunks / G) + G) U sum |products|.
  * An SH value: at most 7 fp32 roundings (the literal, the squares, the sums, the products), each relative to the sum of the
    polynomial's absolute terms: 8 U mag.
  * The sigmoid in fp32: expf within 1 ulp (2 U relative on e / (1 + e) <= 1), the sum and the quotient one rounding each: 4 U s; an
    input error e moves it by at most s (1 - s) e exp(e).
  * A rounding point q = half(p): if p lies further than E(p) from both neighbouring rounding boundaries of fp16, the kernel's p rounds
    to the same fp16 value and E(q) = 0. Otherwise it may land on the other side: E(q) = E(p) + ulp16(|p| + E(p)), half an ulp for each
    of the two roundings plus the distance. E(p) is a few U relative while an fp16 ulp is 2^-10 relative, so about 2^-10 of the roundings
    can flip at all; downstream of a possible flip E is an fp16 ulp of that input times the weights. This keeps the bound of a ray that
    has no rounding near a boundary at fp32 size, where a wrong weight, index or column shows, and makes most rgb values exact.
  * The ReLU gate is a discontinuity of the backward. A (ray, neuron) pair is `undecided` when |z| <= E(z) (`err_z`), or when half(z)
    itself may flip across 0: the kernel's gate may then differ and E(gz) = |half(s)| + E(half(s)), the neuron's whole contribution,
    which the chain carries into dW0[m,:], dW1[:,m] (through E(a)) and the eight grid gradients, hence the table rows. The tests cap
    the share of undecided pairs at 1 % per case, on the reference alone.
  * A table row in default mode: its addends w * gg (one fp32 rounding each, U |v|) arrive as fp32 atomics in any order: count U
    (|base| + sum |v|). Under FOC_DETERMINISTIC each addend is rounded to 2^-40 (2^-41 each), the total is converted to fp32 and added
    to the row once: count 2^-41 + 2 U (|base| + sum |v|). `base` is what grad_embeddings held before the call.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
LEVELS, HIDDEN, IN, OUT = 4, 64, 24, 3
RAYS, MAX_WG = 64, 2048                  # background.hip BG_RAYS, BG_MAX_WG
BLOB = HIDDEN * 32 + 16 * HIDDEN


def spacing16(v):
    """Spacing of fp16 at |v| (2^-24 below 2^-14)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) - 10)


def _round(p, Ep, half=True):
    """q = half(p) (as the dtype of p) and E(q) (module docstring: a rounding point)."""
    if not half:
        return p, Ep
    with np.errstate(over="ignore", invalid="ignore"):
        q16 = p.astype(np.float16)
        q = q16.astype(np.float64)
        lo = np.nextafter(q16, np.float16(-np.inf)).astype(np.float64)
        hi = np.nextafter(q16, np.float16(np.inf)).astype(np.float64)
        p64 = p.astype(np.float64)
        dist = np.minimum(p64 - (q + lo) / 2, (q + hi) / 2 - p64)
        Eq = np.where(dist > Ep, 0.0, Ep + spacing16(np.abs(p64) + Ep))
    return q.astype(p.dtype), Eq


def levels(log2_scale, base_resolution):
    """[(scale fp32, resolution)] per level: exp2f((float)l * S) * (float)H - 1.0f, ceil(scale) + 1."""
    S = np.float32(log2_scale)
    out = []
    for l in range(LEVELS):
        e = np.float32(np.exp2(np.float64(np.float32(l) * S)))
        sc = np.float32(e * np.float32(base_resolution)) - np.float32(1.0)
        out.append((sc, int(math.ceil(float(sc))) + 1))
    return out


def grid_index(size, resolution, px, py):
    """gridencoder.cu:50-84 for D = 2, align_corners = false, gridtype hash; px, py uint64 arrays holding uint32 values."""
    stride, index = 1, np.zeros_like(px)
    for p in (px, py):
        if stride <= size:
            index = index + p * np.uint64(stride)
            stride *= resolution + 1
    if stride > size:
        index = px ^ ((py * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF))
    return index % np.uint64(size)


def sh16(d):
    """Degree-4 real spherical harmonics (shencoder.cu's constants) of d [N,3] in d's dtype, and the sum of each one's absolute terms."""
    t = d.dtype.type
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    c = lambda v: t(v)
    sh = np.stack([np.full_like(x, c(0.28209479177387814)), c(-0.48860251190291987) * y, c(0.48860251190291987) * z, c(-0.48860251190291987) * x,
                   c(1.0925484305920792) * xy, c(-1.0925484305920792) * yz, c(0.94617469575755997) * z2 - c(0.31539156525251999),
                   c(-1.0925484305920792) * xz, c(0.54627421529603959) * x2 - c(0.54627421529603959) * y2,
                   c(0.59004358992664352) * y * (c(-3.0) * x2 + y2), c(2.8906114426405538) * xy * z, c(0.45704579946446572) * y * (c(1.0) - c(5.0) * z2),
                   c(0.3731763325901154) * z * (c(5.0) * z2 - c(3.0)), c(0.45704579946446572) * x * (c(1.0) - c(5.0) * z2),
                   c(1.4453057213202769) * z * (x2 - y2), c(0.59004358992664352) * x * (-x2 + c(3.0) * y2)], -1)
    ax, ay, az = np.abs(x).astype(np.float64), np.abs(y).astype(np.float64), np.abs(z).astype(np.float64)
    x2, y2, z2 = ax * ax, ay * ay, az * az
    mag = np.stack([np.zeros_like(ax), 0.48860251190291987 * ay, 0.48860251190291987 * az, 0.48860251190291987 * ax,
                    1.0925484305920792 * ax * ay, 1.0925484305920792 * ay * az, 0.94617469575755997 * z2 + 0.31539156525251999,
                    1.0925484305920792 * ax * az, 0.54627421529603959 * (x2 + y2), 0.59004358992664352 * ay * (3 * x2 + y2),
                    2.8906114426405538 * ax * ay * az, 0.45704579946446572 * ay * (1 + 5 * z2), 0.3731763325901154 * az * (5 * z2 + 3),
                    0.45704579946446572 * ax * (1 + 5 * z2), 1.4453057213202769 * az * (x2 + y2), 0.59004358992664352 * ax * (x2 + 3 * y2)], -1)
    return sh, mag


def forward(coords, rays_d, emb, offsets, log2_scale, base_resolution, W0, W1, half=True, pos32=True, dtype=np.float64):
    """coords [N,2] fp32, rays_d [N,3] fp32, emb [rows,2] fp32, offsets [5], W0 [64,24] and W1 [3,64] (fp16 values) -> a dict with `rgb`
    [N,3], the intermediates and their error bounds (E_*), `err_z` and `undecided` [N,64]. dtype=np.float32 evaluates the same
    expressions in fp32 (the bound's own test)."""
    ft = dtype
    coords = np.asarray(coords, np.float32)
    N = coords.shape[0]
    offsets = [int(v) for v in offsets]
    W0, W1 = np.asarray(W0).astype(ft), np.asarray(W1).astype(ft)
    with np.errstate(over="ignore"):
        embh = np.asarray(emb, np.float32).astype(np.float16).astype(ft) if half else np.asarray(emb).astype(ft)
    if pos32:
        uv = (coords + np.float32(1.0)) / np.float32(2.0)
    else:
        uv = (coords.astype(np.float64) + 1.0) / 2.0
    inside = ~((uv < 0) | (uv > 1)).any(1)
    uvc = np.where(inside[:, None], uv, uv.dtype.type(0.5))
    rows = np.zeros((N, LEVELS, 4), np.int64)
    wts = np.zeros((N, LEVELS, 4), uv.dtype)
    grid = np.zeros((N, 8), ft)
    E_grid = np.zeros((N, 8))
    one = uv.dtype.type(1.0)
    for l, (sc, res) in enumerate(levels(log2_scale, base_resolution)):
        p = uvc.astype(np.float64) * np.float64(sc) + 0.5
        if pos32:
            p = p.astype(np.float32)
        g = np.floor(p)
        f = p - g
        gi = g.astype(np.uint64)
        size = offsets[l + 1] - offsets[l]
        for idx in range(4):
            w = one * (f[:, 0] if idx & 1 else one - f[:, 0])
            w = w * (f[:, 1] if idx & 2 else one - f[:, 1])
            rows[:, l, idx] = offsets[l] + grid_index(size, res, gi[:, 0] + np.uint64(idx & 1), gi[:, 1] + np.uint64((idx >> 1) & 1)).astype(np.int64)
            wts[:, l, idx] = np.where(inside, w, 0)
        e = embh[rows[:, l]]                                                      # [N,4,2]
        prod = wts[:, l, :, None].astype(ft) * e
        grid[:, 2 * l:2 * l + 2] = prod.sum(1, dtype=ft)
        E_grid[:, 2 * l:2 * l + 2] = 4 * U * np.abs(prod).astype(np.float64).sum(1)
    sh, sh_mag = sh16(np.asarray(rays_d, np.float32).astype(ft))
    pre_x = np.concatenate([sh, grid], 1)
    x, E_x = _round(pre_x, np.concatenate([8 * U * sh_mag, E_grid], 1), half)
    aW0, aW1 = np.abs(W0).astype(np.float64), np.abs(W1).astype(np.float64)
    z = x @ W0.T
    E_z = E_x @ aW0.T + IN * U * (np.abs(x).astype(np.float64) @ aW0.T)
    hz, E_hz = _round(z, E_z, half)
    a = np.maximum(hz, 0)
    undecided = (np.abs(z) <= E_z) | ((E_hz > 0) & (np.abs(hz) <= E_hz))
    o = a @ W1.T
    E_o = E_hz @ aW1.T + HIDDEN * U * (np.abs(a).astype(np.float64) @ aW1.T)
    oh, E_oh = _round(o, E_o, half)
    with np.errstate(over="ignore"):
        s = (ft(1.0) / (ft(1.0) + np.exp(-oh))).astype(ft)
        s64 = s.astype(np.float64)
        E_s = s64 / (1.0 + np.exp(oh.astype(np.float64))) * E_oh * np.exp(np.minimum(E_oh, 50.0)) + 4 * U * s64
    y, E_y = _round(s, E_s, half)
    return dict(N=N, rgb=y, E_rgb=E_y, inside=inside, rows=rows, wts=wts, x=x, E_x=E_x, z=z, err_z=E_z, undecided=undecided, a=a, E_a=E_hz,
                o=oh, y=y, E_y=E_y, W0=W0, W1=W1, n_rows=offsets[LEVELS], half=half, dtype=ft)


def dw_chain(N):
    """(rays one workgroup sums in a row, workgroups) of foc_background_backward's dW sums."""
    chunks = -(-N // RAYS)
    G = min(chunks, MAX_WG)
    return (RAYS * -(-chunks // G), G) if N else (0, 0)


def _scatter(fwd, t):
    """t [N,4 levels,4 corners,2] -> [rows,2]: the float64 sum of the inside rays' entries per table row."""
    keep = np.broadcast_to(fwd["inside"][:, None, None], fwd["rows"].shape).ravel()
    r = fwd["rows"].ravel()[keep]
    return np.stack([np.bincount(r, weights=t[..., c].ravel()[keep], minlength=fwd["n_rows"]) for c in (0, 1)], 1)


def backward(fwd, grad_rgb):
    """grad_rgb [N,3] (fp16 values) -> grad_embeddings [rows,2], dW0 [64,24], dW1 [3,64] and what bounds() needs. In fp32 mode the dW
    sums run as the kernel's: per 64-ray chunk, then over the chunks."""
    ft, half, N = fwd["dtype"], fwd["half"], fwd["N"]
    W0, W1, y, a, x = fwd["W0"], fwd["W1"], fwd["y"], fwd["a"], fwd["x"]
    aW0, aW1 = np.abs(W0).astype(np.float64), np.abs(W1).astype(np.float64)
    g = np.asarray(grad_rgb).astype(ft)
    ag = np.abs(g).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pre = g * (ft(1.0) - y) * y
        E_pre = 2 * U * np.abs(pre).astype(np.float64) + ag * (np.abs(1 - 2 * y.astype(np.float64)) * fwd["E_y"] + fwd["E_y"] ** 2)
        g2, E_g2 = _round(pre, E_pre, half)
        s = g2 @ W1
        E_s = E_g2 @ aW1 + OUT * U * (np.abs(g2).astype(np.float64) @ aW1)
        hs, E_hs = _round(s, E_s, half)
        gz = np.where(a > 0, hs, ft(0.0))
        E_gz = np.where(fwd["undecided"], np.abs(hs).astype(np.float64) + E_hs, np.where(a > 0, E_hs, 0.0))
        W0g = W0[:, 16:]
        gx = gz @ W0g
        E_gx = E_gz @ aW0[:, 16:] + HIDDEN * U * (np.abs(gz).astype(np.float64) @ aW0[:, 16:])
        gg, E_gg = _round(gx, E_gx, half)
        # the table: addend (ray, level, corner, channel) = w * gg[2 l + c]
        wts = fwd["wts"].astype(np.float64)
        ggl = gg.astype(np.float64).reshape(N, LEVELS, 1, 2)
        v = wts[..., None] * ggl
        if ft == np.float32:
            v = v.astype(np.float32).astype(np.float64)
        E_v = wts[..., None] * E_gg.reshape(N, LEVELS, 1, 2) + U * np.abs(v)
        grad_emb, sum_E, sum_abs = _scatter(fwd, v), _scatter(fwd, E_v), _scatter(fwd, np.abs(v))
        count = _scatter(fwd, np.ones_like(v))[:, 0]
        # dW
        ax, aa = np.abs(x).astype(np.float64), np.abs(a).astype(np.float64)
        agz, ag2 = np.abs(gz).astype(np.float64), np.abs(g2).astype(np.float64)
        if ft == np.float32:
            pad = -N % RAYS
            ch = lambda t: np.concatenate([t, np.zeros((pad, t.shape[1]), t.dtype)]).reshape(-1, RAYS, t.shape[1])
            dW0 = np.einsum("cnm,cnj->cmj", ch(gz), ch(x)).sum(0, dtype=np.float32)
            dW1 = np.einsum("cnk,cnm->ckm", ch(g2), ch(a)).sum(0, dtype=np.float32)
        else:
            dW0, dW1 = gz.T @ x, g2.T @ a
        n, G = dw_chain(N)
        E_dW0 = E_gz.T @ ax + agz.T @ fwd["E_x"] + E_gz.T @ fwd["E_x"] + (n + G) * U * (agz.T @ ax)
        E_dW1 = E_g2.T @ aa + ag2.T @ fwd["E_a"] + E_g2.T @ fwd["E_a"] + (n + G) * U * (ag2.T @ aa)
    return dict(grad_embeddings=grad_emb, dW0=dW0, dW1=dW1, E_dW0=E_dW0, E_dW1=E_dW1, sum_E=sum_E, sum_abs=sum_abs, count=count, g2=g2, gz=gz)


def table_gradient(fwd, gg):
    """The grid stage's backward alone: gg [N,8] (the gradient of each level's pair) -> grad_embeddings [rows,2], float64 sums."""
    return _scatter(fwd, fwd["wts"].astype(np.float64)[..., None] * np.asarray(gg, np.float64).reshape(fwd["N"], LEVELS, 1, 2))


def bounds(fwd, bwd=None, deterministic=False, base=None):
    """Per-element bounds on |kernel - reference| (module docstring): rgb [N,3]; with bwd, grad_embeddings [rows,2], dW0, dW1. `base`
    [rows,2]: what grad_embeddings held before the call (the gradient is added to it)."""
    out = dict(rgb=fwd["E_rgb"])
    if bwd is not None:
        mag = bwd["sum_abs"] + (np.abs(np.asarray(base, np.float64)) if base is not None else 0.0)
        cnt = bwd["count"][:, None]
        order = cnt * 2.0 ** -41 + 2 * U * mag if deterministic else cnt * U * mag
        out.update(grad_embeddings=bwd["sum_E"] + np.where(cnt > 0, order, 0.0), dW0=bwd["E_dW0"], dW1=bwd["E_dW1"])
    return out


def pack_blob(W0, W1):
    """W0 [64,24], W1 [3,64] -> the FFMLP blob of bg_net: W0 padded to [64,32], W1 padded to [16,64] (fp16)."""
    blob = np.zeros(BLOB, np.float16)
    blob[:HIDDEN * 32].reshape(HIDDEN, 32)[:, :IN] = W0
    blob[HIDDEN * 32:].reshape(16, HIDDEN)[:OUT] = W1
    return blob


def unpack_blob(blob):
    """A blob-shaped array -> (W0 part [64,24], W1 part [3,64], the padding entries)."""
    blob = np.asarray(blob)
    w0, w1 = blob[:HIDDEN * 32].reshape(HIDDEN, 32), blob[HIDDEN * 32:].reshape(16, HIDDEN)
    return w0[:, :IN], w1[:OUT], np.concatenate([w0[:, IN:].ravel(), w1[OUT:].ravel()])


# ---------------------------------------------------------------------------------------------------------------- the shared cases
LOG2_SCALE = float(np.log2(2048 / 16) / 3)          # encoder_bg: 4 levels from 16 to 2048
BASE_RESOLUTION = 16
GRIDS = {"a": [0, 296, 7024, 173488, 697776],       # encoder_bg's own layout: levels 0-2 dense, level 3 hashed into 2^19 rows (`&`)
         "b": [0, 296, 360, 424, 488],              # 64 rows on levels 1-3: hashed, every row shared by N / 16 rays (`&`)
         "c": [0, 296, 1296, 2296, 3296]}           # 1000 rows on levels 1-3: hashed, not a power of two (`%`)
SIZES = [1, 2, 63, 64, 65, 129, 4097]
BIG = MAX_WG * RAYS + 65                            # 131 137: workgroups 0 and 1 take a second chunk, the last one ragged
MAGS = [0.5, 2048.0, 2.0 ** -20]
CAP = 0.01                                          # share of undecided (ray, neuron) pairs a case may have


def cases():
    """name -> (N, grid, weights 'lin' | 'sat', table amplitude, |grad_rgb| scale, seed)."""
    out = {}
    for j, N in enumerate(SIZES):
        for gi, g in enumerate("abc"):
            mag = MAGS[(j + gi) % 3]
            # 2^-20-scaled gradients get past g2 only through the 128x weights; 2048-scaled ones would leave fp16's range through them
            sat = mag == MAGS[2] or ((j + gi) % 4 == 3 and mag != 2048.0)
            out[f"{N}-{g}"] = (N, g, "sat" if sat else "lin", 0.5, mag, 10 * j + gi)
    out["4097-b-sat"] = (4097, "b", "sat", 0.5, 0.5, 100)
    out["4097-a-subnormal-table"] = (4097, "a", "lin", 1e-4, 0.5, 101)
    out[f"{BIG}-b"] = (BIG, "b", "lin", 0.5, 0.5, 102)
    return out


@functools.lru_cache(maxsize=None)
def table(grid, amplitude):
    rng = np.random.default_rng(7)
    return rng.uniform(-amplitude, amplitude, (GRIDS[grid][-1], 2)).astype(np.float32)


def weights(kind, seed=3):
    """nn.Linear's scale (uniform in +-1/sqrt(fan_in)); 'sat': W1 times 128, so that some logits saturate the fp16 sigmoid (y = 1 exactly,
    g2 = 0) and some give a subnormal y, with |z| and |o| far below fp16's range."""
    rng = np.random.default_rng(seed)
    W0 = rng.uniform(-1, 1, (HIDDEN, IN)) / math.sqrt(IN)
    W1 = rng.uniform(-1, 1, (OUT, HIDDEN)) / math.sqrt(HIDDEN) * (128.0 if kind == "sat" else 1.0)
    return W0.astype(np.float16), W1.astype(np.float16)


def _special_coords():
    f = np.float32
    # The first fp32 values whose u = (c + 1) / 2 leaves [0,1]: below -1 the next one down (u = -2^-25); above +1 the SECOND one up,
    # 1 + 2^-22 (u = 1 + 2^-23) — for the next one up, 1 + 2^-23, the sum c + 1 is a tie that rounds to 2: u = 1 exactly, inside.
    out_hi, out_lo, in_hi = f(1 + 2.0 ** -22), np.nextafter(f(-1), f(-2)), np.nextafter(f(1), f(2))
    edge = [(-1, -1), (1, 1), (-1, 1), (1, -1), (0.3, 1), (-1, -0.7), (in_hi, 0.1), (0.25, in_hi)]        # u, v = 0 or 1: inside
    out = [(out_hi, 0.2), (0.4, out_hi), (out_lo, -0.3), (-0.6, out_lo), (out_hi, out_lo), (3.0, 0.0)]    # outside
    cell = []
    for k in (1, 7, 15):                                   # level 0 (scale 15): p = 15 u + 0.5 an integer, and its fp32 neighbours
        c = f(2 * (k - 0.5) / 15 - 1)
        cell += [(c, 0.37), (np.nextafter(c, f(2)), c), (-0.2, np.nextafter(c, f(-2)))]
    s = [t[i] for i in range(9) for t in (edge, out, cell) if i < len(t)]          # interleaved: any 16 in a row hold all three kinds
    return np.array(s, np.float32)


def rays(N, seed):
    """coords [N,2] and rays_d [N,3] fp32 mixing, at every N that has room for them: interior points, points on the edge of the square,
    points just outside it, points on level 0's cell boundaries, repeated coordinates; unit directions, the six axes, lengths 0.5 and 2."""
    rng = np.random.default_rng(1000 + seed)
    coords = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    sp = _special_coords()
    k = np.concatenate([np.arange(1, min(N, 2 * len(sp)), 2), np.arange(2 * len(sp) + 1, N, 4)])      # every special once by ray 46
    coords[k] = sp[(np.arange(len(k)) + seed) % len(sp)]
    coords[6::8] = coords[5::8][:len(coords[6::8])]
    d = rng.normal(0, 1, (N, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    k = np.arange(5, N, 16)
    d[k] = axes[(k // 16) % 6]
    d[9::16] *= 0.5
    d[13::16] *= 2.0
    return coords, d.astype(np.float32)


def grad_rgb(N, mag, seed):
    """[N,3] fp16 of scale `mag`; every eighth ray (from ray 2) exactly zero."""
    rng = np.random.default_rng(2000 + seed)
    g = (rng.uniform(-1, 1, (N, 3)) * mag).astype(np.float16)
    g[2::8] = 0
    return g


COMBOS = [(0,), (1,), (2,), (0, 1, 2)]                     # each channel of grad_rgb alone, then all three


def only(g, channels):
    out = np.zeros_like(g)
    out[:, list(channels)] = g[:, list(channels)]
    return out


def make_case(name):
    """The inputs of a case and its float64 forward."""
    N, grid, kind, amplitude, mag, seed = cases()[name]
    coords, d = rays(N, seed)
    W0, W1 = weights(kind)
    emb = table(grid, amplitude)
    fwd = forward(coords, d, emb, GRIDS[grid], LOG2_SCALE, BASE_RESOLUTION, W0, W1)
    return dict(name=name, N=N, grid=grid, offsets=np.array(GRIDS[grid], np.int32), coords=coords, rays_d=d, W0=W0, W1=W1, emb=emb,
                grad_rgb=grad_rgb(N, mag, seed), fwd=fwd)
