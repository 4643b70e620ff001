"""GPU: the fixed-step tail kernels (csrc/fixedstep.hip) against the float64 reference of run()'s compositing (tests/fixed_tail_ref.py),
through the raw ABI so that no MLP noise enters: the one-kernel training tail (foc_fixed_tail_forward / _backward), the three-node chain
(foc_fixed_head_* + foc_fixed_composite_*) and the inference forms (foc_fixed_render_inference, foc_fixed_field_pack).

Every call mixes rays that are transparent (h0 <= -8), typical (h0 ~ N(0, 2)), opaque within a few samples (h0 up to 16.5), at trunc_exp's
clamp (h0 = +-14.5, +-15, +-15.0078125, on short rays where such a density still leaves a gradient), and rays that miss the box
(near = far = FLT_MAX); colour logits at +7 and +-12 among N(0, 2) ones; noise draws of exactly 0 and 0.99999994 at the first and last
sample. The sample depths and deltas are formed with the device torch expressions of run() (test_gpu_fixedstep.py pins fs_z to them).

Bound per element: |kernel - float64| <= C * 2^-24 * (T + K) * mag (+ half an fp16 ulp on fp16 outputs, + (T + K) * 2^-126 on fp32
forward outputs for subnormal transmittance), mag from fixed_tail_ref.magnitudes(). C = 2: the device's expf is within 1 ulp (2^-23
relative) and every other operation of the kernels is correctly rounded, its 2^-24 already inside mag; K = 16 covers the second-order
terms the first-order magnitudes drop and the few roundings outside the T-long reductions that mag counts once (the kernels' wave
reductions, the transmittance carried across 64-sample chunks). The same C and K hold an fp32 torch evaluation of the reference's
expressions on the CPU (test_fixed_tail_ref.py).
Measured on MI355X over every case of this file: worst ratio |kernel - float64| / (2^-24 (T + K) mag) = 0.047 (sigma at T = 2; weights
0.032, grad_h0 0.011, grad_c 0.0065, grad_w 0.0067); asserted C = 2, a margin of 40x.

The `w > thresh` decision is taken from the kernel's weights after those have been checked (fixed_tail_ref.py); the inference forms,
which return no weights, report it through their masked colour, and the decision must match float64 wherever the float64 weight is
clear of the threshold by more than the bound.
"""
import numpy as np
import pytest
import torch

from fixed_tail_ref import U, clear_of_half_midpoints, magnitudes, tail, tail_backward
from util import half_ulp, to_np

pytestmark = pytest.mark.gpu

C, K = 2.0, 16
FMAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 2), (3, 63), (4, 64), (5, 65), (7, 127), (9, 128), (33, 129), (64, 512), (17, 1024)]
WORST = {}          # name -> worst measured ratio (read by whoever runs this module to record it)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(name, got, want, mag, T, half=False):
    """got (kernel) against want (float64) within the bound; non-finite values exactly where want (rounded to fp16 for fp16 outputs) has
    them. Returns the worst ratio and records it in WORST."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    mag = np.nan_to_num(np.asarray(mag, np.float64), nan=0.0, posinf=np.inf)
    scale = U * (T + K) * mag
    if half:
        with np.errstate(over="ignore"):
            want16 = want.astype(np.float16).astype(np.float64)
        border = np.isfinite(want) & (np.abs(np.abs(want) - 65520.0) <= C * scale + 32.0)    # float64 within the bound of fp16's overflow
        fin = np.isfinite(want16)
    else:
        want16, border, fin = want, np.zeros(want.shape, bool), np.isfinite(want)
    placed = (np.isfinite(got) == fin) | border
    assert placed.all(), f"{name}: non-finite values at other places than float64's: {np.argwhere(~placed)[:6].tolist()}, " \
                         f"got {got[~placed][:6]}, want {want[~placed][:6]}"
    over = np.isfinite(want) & ~fin & ~border                        # float64 finite, beyond fp16: the kernel must give the same inf
    assert np.array_equal(got[over], want16[over]), f"{name}: fp16 overflow"
    both = fin & np.isfinite(got)
    err = np.abs(got - want)[both]
    extra = 0.5 * half_ulp(np.maximum(np.abs(got), np.abs(want))[both].astype(np.float32)) if half else (T + K) * 2.0 ** -126
    s = scale[both]
    bad = err > C * s + extra
    r = float((np.maximum(err - extra, 0) / np.where(s > 0, s, np.inf)).max(initial=0.0))
    WORST[name] = max(WORST.get(name, 0.0), r)
    assert not bad.any(), f"{name}: {bad.sum()} / {bad.size} beyond the bound; worst ratio {r:.3g}; first at " \
                          f"{np.argwhere(both)[np.argmax(bad)].tolist()}: got {err[bad][:1] + 0} off, bound {(C * s + extra)[bad][:1]}"
    return r


def _z_delta(nears, fars, noise, T):
    """run()'s z_vals and deltas, as the device torch ops form them (fp32)."""
    N = nears.shape[0]
    z = torch.linspace(0.0, 1.0, T, device="cuda").unsqueeze(0).expand(N, T)
    z = nears[:, None] + (fars - nears)[:, None] * z
    sd = (fars - nears) / T
    if noise is not None:
        z = z + (noise.view(N, T) - 0.5) * sd[:, None]
    delta = torch.cat([z[:, 1:] - z[:, :-1], sd[:, None] * torch.ones_like(z[:, :1])], -1)
    return to_np(z), to_np(delta)


def _draw(N, T, seed):
    """Rays in the regimes of the module docstring: ray r has regime (r + seed) % 5."""
    rng = np.random.default_rng(seed)
    h0 = rng.normal(0, 2, (N, T))
    near = rng.uniform(0.2, 0.6, N)
    far = near + rng.uniform(0.5, 2.5, N)
    regime = (np.arange(N) + seed) % 5
    for r in range(N):
        if regime[r] == 0:                                                       # transparent
            h0[r] = rng.uniform(-16, -8, T)
        elif regime[r] == 2:                                                     # opaque from a random sample on
            p = int(rng.integers(0, T))
            h0[r, p:] = rng.uniform(4, 16.5, T - p)
        elif regime[r] == 3:                                                     # at trunc_exp's clamp, on a short ray
            h0[r] = rng.choice([14.5, -14.5, 15.0, -15.0, 15.0078125, -15.0078125, 0.5, -1.0], T)
            far[r] = near[r] + rng.uniform(1e-4, 1e-2) * T / 512
        elif regime[r] == 4:                                                     # misses the box
            near[r] = far[r] = FMAX
    c = (rng.normal(0, 2, (N, T, 3))).astype(np.float16)
    special = rng.random((N, T, 3)) < 0.15
    c[special] = rng.choice(np.array([7.0, 12.0, -12.0], np.float16), int(special.sum()))
    c = clear_of_half_midpoints(c)
    noise = rng.random((N, T)).astype(np.float32)
    even = (np.arange(N) % 2 == 0)
    noise[:, 0] = np.where(even, 0.0, np.float32(0.99999994))
    noise[:, -1] = np.where(even, np.float32(0.99999994), 0.0)
    grads = dict(grad_image=rng.normal(0, 1, (N, 3)), grad_ws=rng.normal(0, 0.05, N), grad_depth=rng.normal(0, 0.1, N),
                 grad_sumsq=rng.normal(0, 1, N) * 10.0 ** rng.uniform(-10, -3, N))
    return dict(h0=h0.astype(np.float16), c=c, near=near.astype(np.float32), far=far.astype(np.float32), noise=noise,
                bg=rng.random((N, 3)).astype(np.float32), grads={k: v.astype(np.float32) for k, v in grads.items()}, rng=rng,
                missed=regime == 4)


TERMS = ("grad_image", "grad_ws", "grad_depth", "grad_sumsq")


def _combos(with_sumsq):
    """One incoming gradient term at a time, then all of them together."""
    terms = TERMS if with_sumsq else TERMS[:3]
    return [(t,) for t in terms] + [terms]


def _grads_of(d, on):
    """The incoming gradients with only the terms in `on`: an absent term is None (NULL), except grad_image (zeros: always read). In the
    all-terms case grad_depth is 0 on every other ray that misses the box: such a ray keeps finite rows (the gdp == 0 rule)."""
    g = {k: (d["grads"][k] if k in on else None) for k in TERMS}
    if g["grad_image"] is None:
        g["grad_image"] = np.zeros_like(d["grads"]["grad_image"])
    if len(on) > 1 and g["grad_depth"] is not None:
        g["grad_depth"] = g["grad_depth"].copy()
        g["grad_depth"][np.nonzero(d["missed"])[0][::2]] = 0.0
    return g


def _tail_fwd(d, N, T, c_width, noise, sumsq, bg_ray, ds, thresh):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    M = N * T
    h = torch.randn(M, 16, device="cuda").half()                        # columns 1..15 are not the tail's to read
    h[:, 0] = _cuda(d["h0"].reshape(-1))
    c = (torch.randn(M, c_width, device="cuda") * 30).half()             # pad columns: whatever the colour network left there
    c[:, :3] = _cuda(d["c"].reshape(-1, 3))
    t = dict(h=h, c=c, near=_cuda(d["near"]), far=_cuda(d["far"]), noise=_cuda(d["noise"].reshape(-1)) if noise else None,
             bg=_cuda(d["bg"]) if bg_ray else None)
    out = {k: torch.full((M,), float("nan"), device="cuda") for k in ("sigma", "trans", "weights")}
    out.update({k: torch.full((N,), float("nan"), device="cuda") for k in ("weights_sum", "depth")})
    out["image"] = torch.full((N, 3), float("nan"), device="cuda")
    out["sumsq"] = torch.full((N,), float("nan"), device="cuda") if sumsq else None
    check(lib.foc_fixed_tail_forward(ptr(h), ptr(c), ptr(t["near"]), ptr(t["far"]), ptr(t["noise"]), ptr(t["bg"]), 0.7, N, T, float(ds),
                                     float(thresh), ptr(out["sigma"]), ptr(out["trans"]), ptr(out["weights"]), ptr(out["weights_sum"]),
                                     ptr(out["depth"]), ptr(out["image"]), c_width, ptr(out["sumsq"]), stream_of(h)), "fixed_tail_forward")
    return t, out


def _tail_bwd(t, out, g, N, T, c_width, ds, thresh):
    from focnerf_amd._lib import lib, ptr, stream_of, check
    M = N * T
    gt = {k: (_cuda(v) if v is not None else None) for k, v in g.items()}
    grad_c = torch.full((M, c_width), float("nan"), dtype=torch.float16, device="cuda")
    grad_h0 = torch.full((M,), float("nan"), dtype=torch.float16, device="cuda")
    check(lib.foc_fixed_tail_backward(ptr(gt["grad_image"]), ptr(gt["grad_ws"]), ptr(gt["grad_depth"]), ptr(t["c"]), ptr(out["sigma"]),
                                      ptr(out["trans"]), ptr(out["weights"]), ptr(t["near"]), ptr(t["far"]), ptr(t["noise"]), ptr(t["bg"]), 0.7,
                                      N, T, float(ds), float(thresh), ptr(grad_c), ptr(grad_h0), c_width, ptr(gt["grad_sumsq"]),
                                      stream_of(grad_c)), "fixed_tail_backward")
    return grad_c, grad_h0


def _reference(d, t, N, T, ds, mask, bg_ray):
    z, delta = _z_delta(t["near"], t["far"], t["noise"], T)
    bg = d["bg"] if bg_ray else np.full((N, 3), 0.7, np.float32)
    return tail(z, delta, d["near"], d["far"], bg, ds, mask, h0=d["h0"], c=d["c"])


def _check_forward(tag, ref, out, N, T, sumsq=True, trans=True):
    m = magnitudes(ref)
    v = lambda k: ref[k].detach().numpy()
    for k in ("sigma",) + (("trans",) if trans else ()) + ("weights",):
        if k in out and out[k] is not None:
            _check(f"{tag}.{k}", to_np(out[k]).reshape(N, T), v(k), m[k] if m[k] is not None else np.zeros((N, T)), T)
    for k in ("weights_sum", "image") + (("sumsq",) if sumsq else ()):
        if out.get(k) is not None:
            _check(f"{tag}.{k}", to_np(out[k]), v(k), m[k], T)
    if out.get("depth") is not None:
        _check(f"{tag}.depth", to_np(out["depth"]), v("depth"), m["depth"], T)    # NaN on rays that miss the box, in both


@pytest.mark.parametrize("cfg", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_tail_kernels_against_float64(shape, cfg):
    """foc_fixed_tail_forward / _backward: forward outputs, then grad_h0 and grad_c for each incoming gradient term alone and all of
    them together; pad columns of grad_c exactly 0; rows of missed rays finite zeros when grad_depth is 0 or NULL; two backward calls
    give the same bits. Configurations alternate c_width 4 / 16, noise and the outside-mask sums on / off, a per-ray or a scalar
    background, density_scale 1 / 3 and thresh 0 / 1e-10 / 1e-4 across the shapes."""
    N, T = shape
    j = SHAPES.index(shape)
    on = cfg == 0
    c_width = (4, 16)[(j + cfg) % 2]
    ds = (1.0, 3.0)[(j + cfg) % 2]
    thresh = (0.0, 1e-10, 1e-4)[(j + 2 * cfg) % 3]
    d = _draw(N, T, 100 * j + cfg)
    t, out = _tail_fwd(d, N, T, c_width, noise=on, sumsq=on, bg_ray=on, ds=ds, thresh=thresh)
    tag = f"tail[{N}x{T},{cfg}]"
    mask = to_np(out["weights"]).reshape(N, T) > thresh
    ref = _reference(d, t, N, T, ds, mask, bg_ray=on)
    _check_forward(tag, ref, out, N, T, sumsq=on)
    for combo in _combos(on):
        g = _grads_of(d, combo)
        grad_c, grad_h0 = _tail_bwd(t, out, g, N, T, c_width, ds, thresh)
        want = tail_backward(ref, **g)
        m = magnitudes(ref, **g)
        gc = to_np(grad_c).astype(np.float64)
        _check(f"{tag}.grad_h0", to_np(grad_h0).astype(np.float64).reshape(N, T), want["grad_h0"].numpy(), m["grad_h0"], T, half=True)
        _check(f"{tag}.grad_c", gc[:, :3].reshape(N, T, 3), want["grad_c"].numpy(), m["grad_c"], T, half=True)
        assert (gc[:, 3:] == 0).all(), "pad columns of grad_c"
        # a ray that misses the box has finite rows when its grad_depth is 0 or NULL — zeros, unless the outside-mask term is on
        quiet = d["missed"] & ((g["grad_depth"] == 0) if g["grad_depth"] is not None else True)
        assert np.isfinite(to_np(grad_h0).reshape(N, T)[quiet]).all() and (gc.reshape(N, T, -1)[quiet] == 0).all()
        if g["grad_sumsq"] is None:
            assert (to_np(grad_h0).reshape(N, T)[quiet] == 0).all()
    grad_c2, grad_h02 = _tail_bwd(t, out, g, N, T, c_width, ds, thresh)
    assert torch.equal(grad_c.view(torch.int16), grad_c2.view(torch.int16)) and torch.equal(grad_h0.view(torch.int16), grad_h02.view(torch.int16))


def test_tail_kernels_against_float64_at_the_headline_size():
    """The training step's shape: 4096 rays x 512 samples, jittered depths, a per-ray background, the outside-mask sums, mask 1e-10."""
    N, T = 4096, 512
    d = _draw(N, T, 7)
    t, out = _tail_fwd(d, N, T, 4, noise=True, sumsq=True, bg_ray=True, ds=1.0, thresh=1e-10)
    mask = to_np(out["weights"]).reshape(N, T) > 1e-10
    ref = _reference(d, t, N, T, 1.0, mask, bg_ray=True)
    _check_forward("headline", ref, out, N, T)
    for combo in (("grad_depth",), TERMS):
        g = _grads_of(d, combo)
        grad_c, grad_h0 = _tail_bwd(t, out, g, N, T, 4, 1.0, 1e-10)
        want = tail_backward(ref, **g)
        m = magnitudes(ref, **g)
        _check("headline.grad_h0", to_np(grad_h0).astype(np.float64).reshape(N, T), want["grad_h0"].numpy(), m["grad_h0"], T, half=True)
        _check("headline.grad_c", to_np(grad_c)[:, :3].astype(np.float64).reshape(N, T, 3), want["grad_c"].numpy(), m["grad_c"], T, half=True)
        assert (to_np(grad_c)[:, 3] == 0).all()


def _sh16(d):
    """Degree-4 real spherical harmonics of unit directions [N,3], float64 (shencoder.py's constants)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    return np.stack([np.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                     1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.94617469575755997 * z2 - 0.31539156525251999,
                     -1.0925484305920792 * xz, 0.54627421529603959 * x2 - 0.54627421529603959 * y2,
                     0.59004358992664352 * y * (-3.0 * x2 + y2), 2.8906114426405538 * xy * z, 0.45704579946446572 * y * (1.0 - 5.0 * z2),
                     0.3731763325901154 * z * (5.0 * z2 - 3.0), 0.45704579946446572 * x * (1.0 - 5.0 * z2), 1.4453057213202769 * z * (x2 - y2),
                     0.59004358992664352 * x * (-x2 + 3.0 * y2)], -1)


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_three_node_chain_against_float64(shape):
    """foc_fixed_head_forward / _backward + foc_fixed_composite_forward / _backward: the head's outputs and the colour-net input rows
    (SH of the direction, h[:,1:16], the pad column 31 = obj[0] or 0, for 48 wide obj[1:16] and a zero), the composite's image, grad_c
    (pad columns 0) and grad_w, and grad_h: column 0 against float64, columns 1..15 = grad_cin[:, 16:31] bit for bit; each incoming term
    alone, then together; two backward calls give the same bits. cin_width 32 / 48 (with and without the object feature)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N, T = shape
    j = SHAPES.index(shape)
    width, with_obj = ((32, False), (48, True), (32, False), (48, False))[j % 4]
    noise, bg_ray = j % 2 == 0, j % 3 != 0
    ds, thresh = (3.0, 1.0)[j % 2], (1e-4, 0.0, 1e-10)[j % 3]
    d = _draw(N, T, 1000 + j)
    M = N * T
    rng = d["rng"]
    h = torch.from_numpy(rng.normal(0, 1, (M, 16)).astype(np.float16)).cuda()
    h[:, 0] = _cuda(d["h0"].reshape(-1))
    dirs = rng.normal(0, 1, (N, 3))
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    obj = _cuda(rng.normal(0, 1, 16).astype(np.float16)) if with_obj else None
    nt, ft, dt = _cuda(d["near"]), _cuda(d["far"]), _cuda(dirs)
    zt = _cuda(d["noise"].reshape(-1)) if noise else None
    bt = _cuda(d["bg"]) if bg_ray else None
    sigma, trans, weights = (torch.full((M,), float("nan"), device="cuda") for _ in range(3))
    ws, depth = torch.full((N,), float("nan"), device="cuda"), torch.full((N,), float("nan"), device="cuda")
    cin = torch.full((M, width), float("nan"), dtype=torch.float16, device="cuda")
    check(lib.foc_fixed_head_forward(ptr(h), ptr(dt), ptr(nt), ptr(ft), ptr(zt), N, T, ds, ptr(sigma), ptr(trans), ptr(weights), ptr(ws),
                                     ptr(depth), ptr(cin), ptr(obj), width, stream_of(h)), "fixed_head_forward")
    c = torch.from_numpy((rng.normal(0, 1, (M, 16)) * 30).astype(np.float16)).cuda()
    c[:, :3] = _cuda(d["c"].reshape(-1, 3))
    image = torch.full((N, 3), float("nan"), device="cuda")
    check(lib.foc_fixed_composite_forward(ptr(c), ptr(weights), ptr(bt), 0.7, N, T, thresh, ptr(image), stream_of(c)), "fixed_composite_forward")
    tag = f"chain[{N}x{T}]"
    mask = to_np(weights).reshape(N, T) > thresh
    t = dict(near=nt, far=ft, noise=zt)
    ref = _reference(d, t, N, T, ds, mask, bg_ray)
    _check_forward(tag, ref, dict(sigma=sigma, trans=trans, weights=weights, weights_sum=ws, depth=depth, image=image), N, T, sumsq=False)
    # the colour-net input rows
    ci = to_np(cin)
    sh = _sh16(dirs.astype(np.float64))
    assert (np.abs(ci[:, :16].reshape(N, T, 16).astype(np.float64) - sh[:, None, :]) <= half_ulp(sh.astype(np.float32))[:, None, :]).all()
    assert np.array_equal(ci[:, 16:31].view(np.uint16), to_np(h)[:, 1:16].view(np.uint16))
    o = to_np(obj).view(np.uint16) if with_obj else np.zeros(16, np.uint16)
    assert (ci[:, 31].view(np.uint16) == o[0]).all()
    if width == 48:
        assert (ci[:, 32:47].view(np.uint16) == o[1:]).all() and (ci[:, 47] == 0).all()
    for combo in _combos(False):
        g = _grads_of(d, combo)
        gi, gws, gdp = (_cuda(g[k]) if g[k] is not None else None for k in TERMS[:3])
        grad_c = torch.full((M, 16), float("nan"), dtype=torch.float16, device="cuda")
        grad_w = torch.full((M,), float("nan"), device="cuda")
        check(lib.foc_fixed_composite_backward(ptr(gi), ptr(c), ptr(weights), ptr(bt), 0.7, N, T, thresh, ptr(grad_c), ptr(grad_w), stream_of(c)),
              "fixed_composite_backward")
        grad_cin = torch.from_numpy(rng.normal(0, 1e-2, (M, width)).astype(np.float16)).cuda()
        grad_h = torch.full((M, 16), float("nan"), dtype=torch.float16, device="cuda")
        gw_in = grad_w if "grad_image" in combo else None
        check(lib.foc_fixed_head_backward(ptr(h), ptr(sigma), ptr(trans), ptr(nt), ptr(ft), ptr(zt), ptr(gw_in), ptr(gws), ptr(gdp), ptr(grad_cin),
                                          N, T, ds, ptr(grad_h), width, stream_of(h)), "fixed_head_backward")
        want = tail_backward(ref, **{**g, "grad_sumsq": None})
        m = magnitudes(ref, **{**g, "grad_sumsq": None})
        gc = to_np(grad_c).astype(np.float64)
        _check(f"{tag}.grad_c", gc[:, :3].reshape(N, T, 3), want["grad_c"].numpy(), m["grad_c"], T, half=True)
        assert (gc[:, 3:] == 0).all(), "pad columns of grad_c"
        _check(f"{tag}.grad_w", to_np(grad_w).reshape(N, T), want["grad_w"].numpy(), m["grad_w"], T)
        _check(f"{tag}.grad_h0", to_np(grad_h)[:, 0].astype(np.float64).reshape(N, T), want["grad_h0"].numpy(), m["grad_h0"], T, half=True)
        assert np.array_equal(to_np(grad_h)[:, 1:].view(np.uint16), to_np(grad_cin)[:, 16:31].view(np.uint16))
    grad_h2 = torch.empty_like(grad_h)
    check(lib.foc_fixed_head_backward(ptr(h), ptr(sigma), ptr(trans), ptr(nt), ptr(ft), ptr(zt), ptr(gw_in), ptr(gws), ptr(gdp), ptr(grad_cin),
                                      N, T, ds, ptr(grad_h2), width, stream_of(h)), "fixed_head_backward")
    assert torch.equal(grad_h.view(torch.int16), grad_h2.view(torch.int16))


def _blocked_rows(N, T, block=64):
    """Ray-major row of every row of the block-interleaved order (include/focnerf.h; the last block padded with ray N-1)."""
    nb = -(-N // block)
    n = torch.arange(nb * block).clamp(max=N - 1).view(nb, 1, block)
    return (n * T + torch.arange(T).view(1, T, 1)).reshape(-1)


@pytest.mark.parametrize("ray_block", [0, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{n}x{t}" for n, t in SHAPES])
def test_inference_forms_against_float64(shape, ray_block):
    """foc_fixed_render_inference and foc_fixed_field_pack (forward only) on fp32 sigma / rgb, ray-major and in 64-ray blocks: image,
    depth, weights_sum against float64; the masked colour and the packed field are the inputs where w > thresh and 0 elsewhere, with
    the decision matching float64 wherever the float64 weight is clear of the threshold by more than the bound."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N, T = shape
    j = SHAPES.index(shape)
    noise, bg_ray = (j + ray_block) % 2 == 0, j % 2 == 1
    ds, thresh = (1.0, 3.0)[j % 2], (1e-10, 1e-4, 0.0)[j % 3]
    d = _draw(N, T, 2000 + j + ray_block)
    M = N * T
    sig = np.exp(d["h0"].astype(np.float32))
    rgb = d["rng"].uniform(0.01, 1.0, (N, T, 3)).astype(np.float32)
    st, rt = _cuda(sig.reshape(-1)), _cuda(rgb.reshape(-1, 3))
    if ray_block:
        rows = _blocked_rows(N, T).cuda()
        st, rt = st[rows].contiguous(), rt[rows].contiguous()
    nt, ft = _cuda(d["near"]), _cuda(d["far"])
    zt = _cuda(d["noise"].reshape(-1)) if noise else None
    bt = _cuda(d["bg"]) if bg_ray else None
    out = dict(image=torch.full((N, 3), float("nan"), device="cuda"), depth=torch.full((N,), float("nan"), device="cuda"),
               weights_sum=torch.full((N,), float("nan"), device="cuda"))
    masked = torch.full((M, 3), float("nan"), device="cuda")
    sig_rm = torch.full((M,), float("nan"), device="cuda") if ray_block else None
    check(lib.foc_fixed_render_inference(ptr(st), ptr(rt), ptr(nt), ptr(ft), ptr(zt), ptr(bt), 0.7, N, T, ds, thresh, ptr(out["image"]),
                                         ptr(out["depth"]), ptr(out["weights_sum"]), ptr(masked), ray_block, ptr(sig_rm), stream_of(st)),
          "fixed_render_inference")
    kept = (to_np(masked).reshape(N, T, 3) != 0).any(-1)
    assert np.array_equal(to_np(masked).reshape(N, T, 3), np.where(kept[..., None], rgb, 0))
    if ray_block:
        assert np.array_equal(to_np(sig_rm), sig.reshape(-1))
    t = dict(near=nt, far=ft, noise=zt)
    z, delta = _z_delta(nt, ft, zt, T)
    ref = tail(z, delta, d["near"], d["far"], d["bg"] if bg_ray else np.full((N, 3), 0.7), ds, kept, sigma=sig, rgb=rgb)
    w = ref["weights"].detach().numpy()
    wb = C * U * (T + K) * magnitudes(ref)["weights"].numpy() + (T + K) * 2.0 ** -126
    assert not (kept != (w > thresh))[np.abs(w - thresh) > wb].any(), "the w > thresh decision where float64 is clear of it"
    tag = f"infer[{N}x{T},{ray_block}]"
    _check_forward(tag, ref, out, N, T, sumsq=False)
    f4 = torch.full((M, 4), float("nan"), device="cuda")
    out2 = {k: torch.full_like(v, float("nan")) for k, v in out.items()}
    check(lib.foc_fixed_field_pack(ptr(st), ptr(rt), ptr(nt), ptr(ft), ptr(zt), ptr(bt), 0.7, N, T, ds, thresh, ptr(out2["image"]),
                                   ptr(out2["depth"]), ptr(out2["weights_sum"]), ptr(f4), ray_block, stream_of(st)), "fixed_field_pack")
    _check_forward(tag + ".pack", ref, out2, N, T, sumsq=False)
    assert np.array_equal(to_np(f4)[:, 0], sig.reshape(-1)) and np.array_equal(to_np(f4)[:, 1:], to_np(masked))


@pytest.mark.parametrize("form", ["tail", "chain"])
def test_non_finite_incoming_gradient_poisons_its_own_ray(form):
    """NaN in one ray's grad_image, inf in another's: non-finite values exactly where float64 has them (NaN exactly where it has NaN on
    the NaN ray), every other element within the bound (_check); 129 samples (a partial third chunk), 8 rays (two workgroups)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    N, T = 8, 129
    d = _draw(N, T, 77)
    d["grads"]["grad_image"][4, 1] = np.nan                          # a typical ray
    d["grads"]["grad_image"][5, 0] = np.inf                          # a ray that turns opaque
    t, out = _tail_fwd(d, N, T, 16, noise=True, sumsq=True, bg_ray=True, ds=1.0, thresh=1e-10)
    mask = to_np(out["weights"]).reshape(N, T) > 1e-10
    ref = _reference(d, t, N, T, 1.0, mask, bg_ray=True)
    g = _grads_of(d, TERMS if form == "tail" else TERMS[:3])
    want = tail_backward(ref, **g)
    m = magnitudes(ref, **g)
    if form == "tail":
        grad_c, grad_h0 = _tail_bwd(t, out, g, N, T, 16, 1.0, 1e-10)
        gh0 = to_np(grad_h0).astype(np.float64).reshape(N, T)
    else:
        gi, gws, gdp = (_cuda(g[k]) for k in TERMS[:3])
        M = N * T
        grad_c = torch.empty(M, 16, dtype=torch.float16, device="cuda")
        grad_w = torch.empty(M, device="cuda")
        check(lib.foc_fixed_composite_backward(ptr(gi), ptr(t["c"]), ptr(out["weights"]), ptr(t["bg"]), 0.7, N, T, 1e-10, ptr(grad_c), ptr(grad_w),
                                               stream_of(grad_c)), "fixed_composite_backward")
        grad_h = torch.empty(M, 16, dtype=torch.float16, device="cuda")
        check(lib.foc_fixed_head_backward(ptr(t["h"]), ptr(out["sigma"]), ptr(out["trans"]), ptr(t["near"]), ptr(t["far"]), ptr(t["noise"]),
                                          ptr(grad_w), ptr(gws), ptr(gdp), None, N, T, 1.0, ptr(grad_h), 32, stream_of(grad_h)), "fixed_head_backward")
        gh0 = to_np(grad_h)[:, 0].astype(np.float64).reshape(N, T)
        assert (to_np(grad_h)[:, 1:] == 0).all()
    gc = to_np(grad_c)[:, :3].astype(np.float64).reshape(N, T, 3)
    w_h0, w_c = want["grad_h0"].numpy(), want["grad_c"].numpy()
    assert np.array_equal(np.isnan(gh0[4]), np.isnan(w_h0[4])) and np.isnan(gh0[4]).any()
    assert np.array_equal(np.isnan(gc[4]), np.isnan(w_c[4])) and np.isnan(gc[4]).any()
    assert not np.isfinite(gh0[5]).all()
    _check(f"nonfinite.{form}.grad_h0", gh0, w_h0, m["grad_h0"], T, half=True)
    _check(f"nonfinite.{form}.grad_c", gc, w_c, m["grad_c"], T, half=True)


def test_render_fixed_steps_refuses_one_step():
    """num_steps = 1 has no delta between samples: the library refuses it (T must be >= 2) rather than dividing by T - 1 = 0."""
    from focnerf_amd import synthetic
    from focnerf_amd.fixedstep import render_fixed_steps
    from focnerf_amd.network import NeRFNetwork
    m = NeRFNetwork(bound=1, cuda_ray=False).cuda()
    o, d = synthetic.make_view_rays(4, 4, 1, 1, seed=0, device="cuda", radius=2.0)
    m.train()
    with pytest.raises(RuntimeError, match="T must be >= 2"), torch.autocast("cuda", dtype=torch.float16):
        render_fixed_steps(m, o, d, num_steps=1, perturb=True)
