"""Reference statements of focnerf_amd.batch (csrc/batch.hip): the Philox draw and the integer pixel and jitter maps, an fp32 statement
of the blend, the per-ray loss, the gradient and the error map's EMA with one numpy fp32 operation per kernel operation, a float64
statement of the rays, the 'linear' conversion, the loss and the gradient, and the bounds the GPU tests hold the kernels to. numpy only.

Checked by tests/test_batch_ref.py against known answers, synthetic.get_rays, the torch lines of the reference's train_step,
torch.nn.MSELoss / HuberLoss with autograd, and torch's gather / scatter.

THE BOUNDS, counted from roundings (U = 2^-24: one correctly rounded fp32 operation has relative error <= U; sqrt and division are
correctly rounded in the kernels, which build with contraction off).

  rays_d   x = ((col + 0.5) - cx) / fx: col + 0.5 is exact below 2^23, the subtraction and the division round: 2 U, the same for y.
           n = sqrt((x x + y y) + 1): the squares 2 U (input) + U each, two sums U each, all terms positive: <= 5 U under the root,
           halved by it, + U of its own: 3.5 U. d = (x, y, 1) / n: 2 U + 3.5 U + U = 6.5 U relative, |d| <= 1.
           The rotation (R0 dx + R1 dy) + R2 dz: each product U, the first sum U on a partial sum, the second U on the result: below
           3 U * sum_k |R_k d_k|, and the inputs' 6.5 U times the same sum. sum_k |R_k d_k| <= |R row| |d| = 1 for a rotation (rows of
           unit length, by Cauchy-Schwarz). Total <= 9.5 U + O(U^2) per component: RAY_BOUND = 16 U holds with room, for a pose whose
           3 x 3 is a rotation. A half-pixel slip at 800 px moves a direction by about 6e-4 = 10^4 U.
  rays_o   the pose's translation, bit for bit.
  gt_rgb   'srgb': bit-equal to the fp32 statement. 'linear': the conversion is taken in double and rounded once, so the converted
           pixel is within one fp32 ulp of the float64 statement (half an ulp from the rounding, the rest for the device's double pow,
           whose error is ~2^-52 relative). Through the blend t1 = rgb a, om = 1 - a, t2 = bg om, gt = t1 + t2 (four roundings, om's
           acting on t2): |gt - ref| <= ulp(rgb) a + U (|t1| + 2 |t2| + |gt|).
  ray_loss, grad, error map: bit-equal to the fp32 statement.
  loss     MSE per component: d = p - g rounds (U, so 2 U on d d), the square U; ((l0 + l1) + l2) / 3: 2 U + U; all terms are
           non-negative, so relative errors do not grow in the sums: 6 U per ray. The sum over the rays is taken in double (2^-53 per
           addition: nothing at this scale), divided by N in double and rounded to fp32 once: U. Total 7 U: LOSS_BOUND['mse'] = 8 U * ref.
           Huber, |d| <= delta: 0.5 (d d), the same count (the 0.5 is exact): 7 U. |d| > delta: delta * (|d| - 0.5 delta): d's U is an
           absolute U |d| on a difference that is >= |d| / 2 (0.5 delta < |d| / 2): 2 U; the subtraction U, the product U: 4 U, the sums
           and the division 3 U, the final rounding U: 8 U. A component whose fp32 d falls on the other side of delta than the float64 d
           changes the branch where the two meet with equal value and slope: second order. LOSS_BOUND['huber'] = 10 U * ref.
  grad     MSE: g = (2 d) / float(3 N): d rounds (U |d|), the doubling is exact, the division rounds (U); float(3 N) is exact for
           3 N < 2^24 and carries U beyond: <= 3 U |ref| in all. The bound of the feature's specification,
           (2 / (3 N)) U max(|p|, |g|) + 2 U |ref|, is at least that wherever |d| <= max(|p|, |g|), i.e. wherever p and g have one sign
           (colours): U |ref| = (2 / (3 N)) U |d|. It is kept as specified.
           Huber: |d| <= delta: g = d / float(3 N), the same two or three roundings on half the value: (1 / (3 N)) U max(|p|, |g|) +
           2 U |ref|. |d| > delta: +-delta / float(3 N): fp32(delta) is the kernel's own input, so one or two roundings: inside
           2 U |ref|. A component within U max(|p|, |g|) of delta may take the other branch; there the two gradients differ by at most
           that rounding of d, which the first term already holds.
Nothing here is fitted to an output."""
import numpy as np

U = 2.0 ** -24
M32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
CELL = 128

RAY_BOUND = 16.0 * U


# ---------------------------------------------------------------- Philox4x32-10
def philox(ctr, key):
    """Philox4x32-10 on Python integers: ctr 4 words, key 2 words -> 4 words."""
    c = [int(v) & M32 for v in ctr]
    k = [int(v) & M32 for v in key]
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c[0], PHILOX_M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + PHILOX_W0) & M32, (k[1] + PHILOX_W1) & M32]
    return c


def philox_rays(seed, step, n, stream):
    """The four words of every ray r < n: uint64 array [n,4] (values < 2^32). Counter (r, step lo, step hi, stream), key (seed lo, seed hi)."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    m = np.uint64(M32)
    c0 = np.arange(n, dtype=np.uint64)
    c1 = np.full(n, step & M32, dtype=np.uint64)
    c2 = np.full(n, step >> 32, dtype=np.uint64)
    c3 = np.full(n, int(stream), dtype=np.uint64)
    k0, k1 = seed & M32, seed >> 32
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2          # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def uniform(w):
    """(w >> 8) * 2^-24 as fp32, exact, in [0, 1)."""
    return ((np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * U).astype(np.float32)


def pixel_inds(seed, step, n, H, W):
    """The uniform route: inds = (uint64(word 0 of stream 0) * (H * W)) >> 32, int64 [n]."""
    w = philox_rays(seed, step, n, 0)[:, 0]
    return ((w * np.uint64(H * W)) >> np.uint64(32)).astype(np.int64)


def coarse_pixels(seed, step, inds_coarse, H, W):
    """The error-map route (nerf/utils.py:104-110) in fp32: -> rows, cols int64 [n]."""
    c = np.asarray(inds_coarse, dtype=np.int64).reshape(-1)
    q = philox_rays(seed, step, c.shape[0], 0)
    u1, u2 = uniform(q[:, 1]), uniform(q[:, 2])
    sx, sy = np.float32(H) / np.float32(128), np.float32(W) / np.float32(128)
    rows = ((c // CELL).astype(np.float32) * sx + u1 * sx).astype(np.int64)
    cols = ((c % CELL).astype(np.float32) * sy + u2 * sy).astype(np.int64)
    return np.minimum(rows, H - 1), np.minimum(cols, W - 1)


def bg_colors(seed, step, n):
    """The pixel-wise random background: words 0..2 of stream 1 as uniform floats, fp32 [n,3]."""
    return uniform(philox_rays(seed, step, n, 1)[:, :3])


def view_of(order, step):
    return int(np.asarray(order)[int(step) % len(order)])


# ---------------------------------------------------------------- pixels, colour space, blend
def pixel_values(pixels):
    """uint8 -> float(v) / 255.f in fp32; fp16 widened exactly; fp32 as it is."""
    pixels = np.asarray(pixels)
    if pixels.dtype == np.uint8:
        return pixels.astype(np.float32) / np.float32(255)
    return pixels.astype(np.float32)


def srgb_to_linear64(x):
    """nerf/utils.py:52-53 in float64."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x < 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)


def blend32(rgb, a, bg):
    """gt = rgb * a + bg * (1 - a), four fp32 operations (nerf/utils.py:856). rgb [n,3], a [n,1], bg [n,3] or a scalar."""
    rgb, a, bg = np.asarray(rgb, dtype=np.float32), np.asarray(a, dtype=np.float32), np.asarray(bg, dtype=np.float32)
    t1 = rgb * a
    om = np.float32(1) - a
    t2 = bg * om
    return t1 + t2


def blend64(rgb, a, bg, drop_one_minus=False):
    rgb, a, bg = (np.asarray(v, dtype=np.float64) for v in (rgb, a, bg))
    return rgb * a + bg * (a if drop_one_minus else 1.0 - a)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def linear_gt_bound(rgb64, a, bg):
    """|gt - blend64| allowed on the 'linear' route (module docstring); with a = None (C = 3) the conversion's one ulp alone."""
    if a is None:
        return ulp32(rgb64)
    a, bg = np.asarray(a, dtype=np.float64), np.asarray(bg, dtype=np.float64)
    t1, t2 = np.abs(rgb64 * a), np.abs(bg * (1.0 - a))
    return ulp32(rgb64) * a + U * (t1 + 2.0 * t2 + (t1 + t2))


# ---------------------------------------------------------------- rays
def rays64(pose, intrinsics, rows, cols, half=0.5, swap=False, transpose=False):
    """get_rays (nerf/utils.py:131-139) in float64 for one pose [4,4]: -> rays_o [n,3], rays_d [n,3]. The keywords are the mutants the
    bound must reject: no + 0.5, rows and columns swapped, the rotation transposed."""
    pose = np.asarray(pose, dtype=np.float64)
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics)                  # the kernel's inputs are fp32
    rows, cols = np.asarray(rows, dtype=np.float64), np.asarray(cols, dtype=np.float64)
    if swap:
        rows, cols = cols, rows
    x = (cols + half - cx) / fx
    y = (rows + half - cy) / fy
    d = np.stack([x, y, np.ones_like(x)], axis=-1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    R = pose[:3, :3]
    rays_d = d @ (R if transpose else R.T)
    rays_o = np.broadcast_to(pose[:3, 3], rays_d.shape).copy()
    return rays_o, rays_d


# ---------------------------------------------------------------- loss
def loss32(pred, gt, kind="mse", delta=0.1):
    """The kernel's fp32 operations in its order: -> ray_loss [n], grad [n,3] (fp32). pred, gt [n,3]; fp16 pred is widened exactly."""
    p, g = np.asarray(pred).astype(np.float32), np.asarray(gt, dtype=np.float32)
    n = p.shape[0]
    n3 = np.float32(3.0 * n)
    d = p - g
    if kind == "mse":
        l = d * d
        gr = np.float32(2) * d
    else:
        dl = np.float32(delta)
        quad = np.abs(d) <= dl
        l = np.where(quad, np.float32(0.5) * (d * d), dl * (np.abs(d) - np.float32(0.5) * dl))
        gr = np.where(quad, d, np.where(d < 0, -dl, dl))
    ray_loss = ((l[:, 0] + l[:, 1]) + l[:, 2]) / np.float32(3)
    return ray_loss.astype(np.float32), (gr / n3).astype(np.float32)


def loss64(pred, gt, kind="mse", delta=0.1, channels=3):
    """float64: -> ray_loss [n], grad [n,3] = d(loss) / d(pred), loss. `delta` is taken as the kernel gets it (fp32). `channels=2` is the
    mutant that averages over two of the three channels."""
    p, g = np.asarray(pred).astype(np.float64), np.asarray(gt).astype(np.float64)
    n = p.shape[0]
    d = p - g
    if kind == "mse":
        l, gr = d * d, 2.0 * d
    else:
        dl = float(np.float32(delta))
        quad = np.abs(d) <= dl
        l = np.where(quad, 0.5 * d * d, dl * (np.abs(d) - 0.5 * dl))
        gr = np.where(quad, d, dl * np.sign(d))
    ray_loss = l[:, :channels].sum(-1) / channels
    grad = gr / (channels * n)
    grad[:, channels:] = 0.0
    return ray_loss, grad, float(ray_loss.mean())


LOSS_BOUND = {"mse": 8.0 * U, "huber": 10.0 * U}         # times the float64 loss (module docstring)


def loss_bound(ref_loss, kind="mse"):
    return LOSS_BOUND[kind] * abs(float(ref_loss))


def grad_bound(ref_grad, pred, gt, kind="mse"):
    """(2 / (3 N)) U max(|p|, |g|) + 2 U |ref| for MSE, (1 / (3 N)) U max(|p|, |g|) + 2 U |ref| for Huber (module docstring)."""
    p, g = np.abs(np.asarray(pred).astype(np.float64)), np.abs(np.asarray(gt).astype(np.float64))
    n = p.shape[0]
    lead = 2.0 if kind == "mse" else 1.0
    return lead / (3.0 * n) * U * np.maximum(p, g) + 2.0 * U * np.abs(ref_grad)


def ema32(old, ray_loss):
    """error_map[view, c] = 0.1f * old + 0.9f * ray_loss: three fp32 operations."""
    return np.float32(0.1) * np.asarray(old, dtype=np.float32) + np.float32(0.9) * np.asarray(ray_loss, dtype=np.float32)


def ema64(old, ray_loss, swapped=False):
    a, b = (0.9, 0.1) if swapped else (0.1, 0.9)
    return a * np.asarray(old, dtype=np.float64) + b * np.asarray(ray_loss, dtype=np.float64)


def error_map_update32(error_map, view, inds_coarse, ray_loss):
    """The updated map (a copy): row `view`, cells `inds_coarse` (distinct), fp32."""
    out = np.array(error_map, dtype=np.float32, copy=True)
    c = np.asarray(inds_coarse, dtype=np.int64).reshape(-1)
    out[view, c] = ema32(out[view, c], ray_loss)
    return out


# ---------------------------------------------------------------- a whole batch
def sample(images, poses, intrinsics, order, seed, step, n, random_bg=True, linear=False, inds_coarse=None, clamp=True):
    """What RaySampler.next() must produce at `step`: a dict with view, inds, rows, cols, bg (fp32 [n,3]), rays_o, rays_d (float64),
    and gt: for 'srgb' the fp32 statement `gt` (bit-equal); for 'linear' `gt64` and `gt_bound`. `clamp`: n <= H * W as the reference
    has it (nerf/utils.py:73); RaySampler(clamp=False) keeps a larger n, and pixels then repeat."""
    images, poses = np.asarray(images), np.asarray(poses)
    V, H, W, C = images.shape
    n = min(int(n), H * W) if clamp else int(n)
    v = view_of(order, step)
    if inds_coarse is None:
        inds = pixel_inds(seed, step, n, H, W)
        rows, cols = inds // W, inds % W
    else:
        rows, cols = coarse_pixels(seed, step, inds_coarse, H, W)
        inds = rows * W + cols
    rnd = C == 4 and random_bg
    bg = bg_colors(seed, step, n) if rnd else np.ones((n, 3), dtype=np.float32)
    px = pixel_values(images[v].reshape(H * W, C)[inds])
    rays_o, rays_d = rays64(poses[v], intrinsics, rows, cols)
    out = {"view": v, "inds": inds, "rows": rows, "cols": cols, "bg": bg, "rays_o": rays_o, "rays_d": rays_d}
    a = px[:, 3:4] if C == 4 else None
    if not linear:
        out["gt"] = blend32(px[:, :3], a, bg) if C == 4 else px[:, :3]
    else:
        rgb64 = srgb_to_linear64(px[:, :3])
        out["gt64"] = blend64(rgb64, a, bg) if C == 4 else rgb64
        out["gt_bound"] = linear_gt_bound(rgb64, a, bg)
    return out
