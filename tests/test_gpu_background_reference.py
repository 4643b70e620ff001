"""GPU: the background kernels (csrc/background.hip: foc_background_forward / _backward) against the float64 reference of the operation
(tests/background_ref.py), through the raw ABI, so that no packing, autograd or scratch logic sits in between; in the default mode and
under FOC_DETERMINISTIC.

Every call mixes (background_ref.rays) interior points, points exactly on the edge of the square (inside), points one fp32 step outside it
(zero grid part, no table gradient, SH still feeds dW0), points on level 0's cell boundaries and repeated coordinates; unit directions,
the six axes, directions of length 0.5 and 2. N in {1, 2, 63, 64, 65, 129, 4097} on three hand-made grids — encoder_bg's own layout, 64
rows per hashed level (every row shared by N / 16 rays), 1000 rows per hashed level (the `%` wrap) — with a table uniform in +-0.5, one
case with the +-1e-4 initial table (fp16-subnormal features), one with W1 scaled until the fp16 sigmoid saturates (y = 1, g2 = 0) or
turns subnormal, and one at N = 131 137 = 2048 * 64 + 65, where workgroups take a second 64-ray chunk and the last chunk is ragged.
grad_rgb is fed one channel at a time and then whole, at scales 0.5, 2048 and 2^-20, with whole rays exactly zero.

The assertion is |kernel - float64| <= bounds() element by element — rgb, every channel of every table row, every entry of dW0 and dW1 —
with the bound derived in background_ref.py (a value whose bound is 0 must be exact). The share of undecided ReLU gates is capped on the
reference alone before the kernel is looked at.
Measured on MI355X over every test of this file, worst |kernel - float64| / bound: rgb 0.99975 in both modes; grad_embeddings 0.989
(default) and 0.99978 (FOC_DETERMINISTIC); dW0 0.890 and dW1 0.979 in both modes. The ratios near 1 are single values whose pre-rounding
value lies within E of an fp16 rounding boundary and lands on its other side: the error is one fp16 ulp against a bound of one ulp + E.
Away from such flips the bound is of fp32 size, and 92 % of the rgb values carry a bound of 0 and match bit for bit. Undecided ReLU
gates: at most 0.025 % of the pairs of a case (63-a: one pair), 0.001-0.002 % at N >= 4097, against the cap of 1 %.
"""
import numpy as np
import pytest
import torch

import background_ref as br
from util import to_np

pytestmark = pytest.mark.gpu

OPT = "FOC_DETERMINISTIC"
MODES = (("default", 0), ("deterministic", 1))
FOC_E_INVALID = 1
WORST = {}          # "<output>.<mode>" -> worst measured |kernel - float64| / bound (read by whoever runs this module to record it)
SHARES = {}         # case -> share of undecided (ray, neuron) pairs


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(name, got, want, bound, where=None):
    """|got - want| <= bound element by element (over `where`); records the worst ratio in WORST."""
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    if where is not None:
        got, want, bound = got[where], want[where], bound[where]
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.isfinite(bound).all(), f"{name}: non-finite values"
    err = np.abs(got - want)
    exact = bound == 0
    assert not (err[exact] > 0).any(), f"{name}: {int((err[exact] > 0).sum())} values with a zero bound differ, first at " \
                                       f"{np.argwhere(exact & (err > 0))[0].tolist()}: got {got[exact & (err > 0)][0]!r}, want {want[exact & (err > 0)][0]!r}"
    r = float((err[~exact] / bound[~exact]).max(initial=0.0))
    key = name.split("/")[0]
    WORST[key] = max(WORST.get(key, 0.0), r)
    bad = err > bound
    assert not bad.any(), f"{name}: {int(bad.sum())} / {bad.size} beyond the bound, worst ratio {r:.4g}, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"off by {err[bad][0]:.4g}, bound {bound[bad][0]:.4g}, want {want[bad][0]!r}"


class _Device:
    """A case's inputs on the device and the two raw calls."""

    def __init__(self, c, rays_o=None, radius=0.0):
        self.N = c["N"]
        self.d, self.emb, self.off = _cuda(c["rays_d"]), _cuda(c["emb"]), _cuda(c["offsets"])
        self.coords = _cuda(c["coords"]) if rays_o is None else None
        self.rays_o, self.radius = (_cuda(rays_o) if rays_o is not None else None), float(radius)
        self.blob = _cuda(br.pack_blob(c["W0"], c["W1"]))
        self.rows = int(c["offsets"][-1])

    def forward(self):
        from focnerf_amd._lib import lib, ptr, stream_of, check
        rgb = torch.full((self.N, 3), float("nan"), dtype=torch.float16, device="cuda")
        check(lib.foc_background_forward(ptr(self.rays_o), ptr(self.d), ptr(self.coords), self.radius, self.N, ptr(self.emb), ptr(self.off),
                                         br.LOG2_SCALE, br.BASE_RESOLUTION, ptr(self.blob), ptr(rgb), stream_of(self.d)), "background_forward")
        return rgb

    def workspace(self, fill=0):
        from focnerf_amd._lib import lib
        return torch.full((int(lib.foc_background_backward_workspace_bytes(self.N)),), fill, dtype=torch.uint8, device="cuda")

    def backward_rc(self, g, grad_emb, grad_w, ws, ws_bytes=None):
        from focnerf_amd._lib import lib, ptr, stream_of
        g = _cuda(g) if isinstance(g, np.ndarray) else g
        return lib.foc_background_backward(ptr(g), ptr(self.rays_o), ptr(self.d), ptr(self.coords), self.radius, self.N, ptr(self.emb), ptr(self.off),
                                           br.LOG2_SCALE, br.BASE_RESOLUTION, ptr(self.blob), ptr(grad_emb), ptr(grad_w), ptr(ws),
                                           ws.numel() if ws_bytes is None else ws_bytes, stream_of(self.d))

    def backward(self, g, base=None, ws_fill=0):
        """-> grad_embeddings [rows,2] (started from `base` or zeros) and grad_weights [3072], as numpy."""
        from focnerf_amd._lib import check
        grad_emb = _cuda(base) if base is not None else torch.zeros(self.rows, 2, device="cuda")
        grad_w = torch.full((br.BLOB,), float("nan"), device="cuda")
        check(self.backward_rc(g, grad_emb, grad_w, self.workspace(ws_fill)), "background_backward")
        return to_np(grad_emb), to_np(grad_w)


def _check_backward(tag, mode, c, bwd, got_emb, got_w, deterministic, base=None):
    bd = br.bounds(c["fwd"], bwd, deterministic=deterministic, base=base)
    w0, w1, pad = br.unpack_blob(got_w)
    assert (pad.view(np.uint32) == 0).all(), f"{tag}: padding entries of grad_weights"
    want = bwd["grad_embeddings"] + (base.astype(np.float64) if base is not None else 0.0)
    _check(f"grad_embeddings.{mode}/{tag}", got_emb, want, bd["grad_embeddings"])
    _check(f"dW0.{mode}/{tag}", w0, bwd["dW0"], bd["dW0"])
    _check(f"dW1.{mode}/{tag}", w1, bwd["dW1"], bd["dW1"])


def _assert_cap(c):
    share = float(c["fwd"]["undecided"].mean())
    SHARES[c["name"]] = share
    assert share <= br.CAP, f"{c['name']}: {100 * share:.3g} % of the (ray, neuron) pairs are undecided"


@pytest.mark.parametrize("name", list(br.cases()))
def test_background_kernels_against_float64(name, lib_option):
    """rgb, then grad_embeddings row by row and channel by channel, dW0 and dW1 entry by entry, for each channel of grad_rgb alone and all
    three, in both modes; the padding entries of grad_weights exactly 0."""
    c = br.make_case(name)
    _assert_cap(c)
    dev = _Device(c)
    refs = [(combo, br.backward(c["fwd"], br.only(c["grad_rgb"], combo))) for combo in br.COMBOS]
    for mode, det in MODES:
        lib_option(OPT, det)
        _check(f"rgb.{mode}/{name}", to_np(dev.forward()), c["fwd"]["rgb"], c["fwd"]["E_rgb"])
        for combo, bwd in refs:
            got_emb, got_w = dev.backward(br.only(c["grad_rgb"], combo))
            _check_backward(f"{name}{list(combo)}", mode, c, bwd, got_emb, got_w, bool(det))


@pytest.fixture(scope="module")
def case_b():
    """N = 4097 on the grid with 64 rows per hashed level: the case of the contract tests, its all-channels backward included."""
    c = br.make_case("4097-b")
    c["bwd"] = br.backward(c["fwd"], c["grad_rgb"])
    return c


def test_grad_embeddings_is_added_to(case_b, lib_option):
    """A pre-filled grad_embeddings: touched rows are the pattern plus the gradient within the bound, untouched rows keep their bits."""
    c = case_b
    base = np.random.default_rng(5).normal(0, 1, (int(c["offsets"][-1]), 2)).astype(np.float32)
    untouched = c["bwd"]["count"] == 0
    assert 0 < untouched.sum() < untouched.size
    dev = _Device(c)
    for mode, det in MODES:
        lib_option(OPT, det)
        got_emb, got_w = dev.backward(c["grad_rgb"], base=base)
        assert np.array_equal(got_emb[untouched].view(np.uint32), base[untouched].view(np.uint32)), f"{mode}: untouched rows"
        _check_backward("added-to", mode, c, c["bwd"], got_emb, got_w, bool(det), base=base)


def test_workspace_needs_no_zero_fill(case_b, lib_option):
    """A workspace of 0xFF bytes gives the bits of a zeroed one: dW in the default mode, dW and the table under the option."""
    dev = _Device(case_b)
    for mode, det in MODES:
        lib_option(OPT, det)
        emb0, w0 = dev.backward(case_b["grad_rgb"], ws_fill=0)
        emb1, w1 = dev.backward(case_b["grad_rgb"], ws_fill=0xFF)
        assert np.array_equal(w0.view(np.uint32), w1.view(np.uint32)), f"{mode}: grad_weights"
        if det:
            assert np.array_equal(emb0.view(np.uint32), emb1.view(np.uint32)), "deterministic: grad_embeddings"


def test_short_workspace_is_refused(case_b, lib_option):
    dev = _Device(case_b)
    g = _cuda(case_b["grad_rgb"])
    for mode, det in MODES:
        lib_option(OPT, det)
        ws = dev.workspace()
        grad_emb, grad_w = torch.zeros(dev.rows, 2, device="cuda"), torch.zeros(br.BLOB, device="cuda")
        assert dev.backward_rc(g, grad_emb, grad_w, ws, ws_bytes=ws.numel() - 1) == FOC_E_INVALID, mode
        assert dev.backward_rc(g, grad_emb, grad_w, ws) == 0, mode
    torch.cuda.synchronize()


def test_deterministic_mode_repeats_and_ignores_the_ray_order(case_b, lib_option):
    """Under the option two runs give the same bits, and a permutation of the rays gives the same table gradient (N rays on 64 rows per
    level: the heaviest contention the row table sees); N = 1 (the 1024-entry minimum table) repeats too."""
    lib_option(OPT, 1)
    c = case_b
    dev = _Device(c)
    emb0, w0 = dev.backward(c["grad_rgb"])
    emb1, w1 = dev.backward(c["grad_rgb"])
    assert np.array_equal(emb0.view(np.uint32), emb1.view(np.uint32)) and np.array_equal(w0.view(np.uint32), w1.view(np.uint32))
    perm = np.random.default_rng(9).permutation(c["N"])
    emb2, _ = _Device(dict(c, coords=c["coords"][perm], rays_d=c["rays_d"][perm])).backward(c["grad_rgb"][perm])
    assert np.array_equal(emb0.view(np.uint32), emb2.view(np.uint32)), "a permutation of the rays changed the table gradient"
    assert np.abs(emb0).max() > 0
    one = br.make_case("1-a")
    d1 = _Device(one)
    a, b = d1.backward(one["grad_rgb"]), d1.backward(one["grad_rgb"])
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.abs(a[0]).max() > 0


def test_non_finite_incoming_gradient_poisons_its_own_rows(case_b, lib_option):
    """inf and NaN in one ray's grad_rgb: that ray's table rows become non-finite exactly where float64's do, in the same places in both
    modes; every other row stays within its bound; dW is non-finite only where float64, fed the same values, is (or where the ray's
    gate is undecided)."""
    c = case_b
    f = c["fwd"]
    g = c["grad_rgb"].copy()
    p = int(np.nonzero(f["inside"] & (np.abs(g.astype(np.float32)).min(1) > 0))[0][3])
    g[p] = [np.inf, 0.25, np.nan]
    bwd = br.backward(f, g)
    ref_bad = ~np.isfinite(bwd["grad_embeddings"])
    assert ref_bad.any() and set(np.nonzero(ref_bad.any(1))[0]) <= set(f["rows"][p].ravel().tolist())
    dev = _Device(c)
    places = []
    for mode, det in MODES:
        lib_option(OPT, det)
        got_emb, got_w = dev.backward(g)
        bad = ~np.isfinite(got_emb)
        assert np.array_equal(bad, ref_bad), f"{mode}: non-finite table entries at other places than float64's"
        places.append(bad)
        bd = br.bounds(f, bwd, deterministic=bool(det))
        _check(f"grad_embeddings.{mode}/non-finite", got_emb, bwd["grad_embeddings"], bd["grad_embeddings"], where=~ref_bad)
        w0, w1, pad = br.unpack_blob(got_w)
        assert (pad.view(np.uint32) == 0).all()
        for key, got, allowed in (("dW0", w0, ~np.isfinite(bwd["dW0"]) | f["undecided"][p][:, None]), ("dW1", w1, ~np.isfinite(bwd["dW1"]))):
            assert not (~np.isfinite(got) & ~allowed).any(), f"{mode}: {key} non-finite where float64 is finite"
            fin = np.isfinite(bwd[key]) & np.isfinite(got)
            assert fin.any()
            _check(f"{key}.{mode}/non-finite", got, bwd[key], bd[key], where=fin)
        assert (~np.isfinite(w0)).any() and (~np.isfinite(w1)).any()
    assert np.array_equal(places[0], places[1])


def test_rays_form_is_the_coordinates_form(case_b, lib_option):
    """coords = NULL with rays_o and a radius: the bits of the coordinates form fed with raymarching.sph_from_ray's output — rgb, dW in
    both modes and the table gradient under the option; in the default mode the table gradient within the row bound of the float64
    reference at those coordinates."""
    from focnerf_amd import raymarching
    c = dict(case_b)
    rng = np.random.default_rng(11)
    o = (rng.uniform(-1, 1, (c["N"], 3)) * 0.9).astype(np.float32)
    d = c["rays_d"] / np.linalg.norm(c["rays_d"], axis=1, keepdims=True).astype(np.float32)
    coords = to_np(raymarching.sph_from_ray(_cuda(o), _cuda(d), 32.0))
    c.update(coords=coords, rays_d=d)
    c["fwd"] = br.forward(coords, d, c["emb"], c["offsets"], br.LOG2_SCALE, br.BASE_RESOLUTION, c["W0"], c["W1"])
    bwd = br.backward(c["fwd"], c["grad_rgb"])
    via_coords, via_rays = _Device(c), _Device(c, rays_o=o, radius=32.0)
    for mode, det in MODES:
        lib_option(OPT, det)
        assert torch.equal(via_coords.forward().view(torch.int16), via_rays.forward().view(torch.int16)), mode
        emb_c, w_c = via_coords.backward(c["grad_rgb"])
        emb_r, w_r = via_rays.backward(c["grad_rgb"])
        assert np.array_equal(w_c.view(np.uint32), w_r.view(np.uint32)), f"{mode}: grad_weights"
        if det:
            assert np.array_equal(emb_c.view(np.uint32), emb_r.view(np.uint32)), "deterministic: grad_embeddings"
        _check_backward("rays-form", mode, c, bwd, emb_r, w_r, bool(det))


def test_no_rays(lib_option):
    """N = 0: the forward returns FOC_OK and touches nothing; the backward writes grad_weights as zeros and leaves grad_embeddings alone."""
    from focnerf_amd._lib import lib, ptr, stream_of
    c = br.make_case("1-b")
    dev = _Device(c)
    for mode, det in MODES:
        lib_option(OPT, det)
        rgb = torch.full((4, 3), 7.0, dtype=torch.float16, device="cuda")
        rc = lib.foc_background_forward(None, ptr(dev.d), ptr(dev.coords), 0.0, 0, ptr(dev.emb), ptr(dev.off), br.LOG2_SCALE, br.BASE_RESOLUTION,
                                        ptr(dev.blob), ptr(rgb), stream_of(dev.d))
        assert rc == 0 and (rgb == 7.0).all()
        grad_emb = torch.full((dev.rows, 2), 3.0, device="cuda")
        grad_w = torch.full((br.BLOB,), float("nan"), device="cuda")
        dev.N = 0
        assert dev.backward_rc(_cuda(c["grad_rgb"]), grad_emb, grad_w, torch.zeros(16, dtype=torch.uint8, device="cuda"), ws_bytes=0) == 0, mode
        dev.N = 1
        assert (to_np(grad_w).view(np.uint32) == 0).all() and (grad_emb == 3.0).all(), mode
