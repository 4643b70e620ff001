"""GPU: near_far_from_aabb, sph_from_ray, march_rays_train (wave, lane + scan, fused-range forms) and march_rays (serial, row, and the forms of
foc_march_rays_two_phase) against the float64 definition of tests/march_ref.py, through the backend and the raw ABI. The asserted bound is
the derived one (error / bound <= 1, march_ref's docstring). check_train / check_burst re-synchronise on the kernel's own samples, so what
they leave undecided (a sample within the band of a cell face, a gap whose walk meets a band) depends on that output: every test therefore
asserts the caps test_march_ref.py holds on the oracle — at most 2 % of the gaps and 1 % of the samples left out, and a strict minority —
so that a kernel cannot pass by making its output undecidable. Every output buffer starts at a fill value with a guard band behind it,
which must come back untouched. Each test prints its worst ratios.

Measured on the MI355X (worst error / bound over all cases, asserted <= 1; `pytest -s` prints them per test with the shares left out):
    form                                       deltas0   xyzs     next_sample_t   t_below_far   gaps / samples left out (worst case)
    march_rays_train  wave                     0.025     0.026    0.090           0             0.0112 / 0.0004
    march_rays_train  lane + scan              0.025     0.026    0.090           0             0.0112 / 0.0004
    march_rays_train  fused range (field)      0.023     0.049    0.090           0             0.0106 / 0.0008   (xyzs: the normalised enc_in)
    march_rays        row and serial           0.025     0.026    0.090           0             0.0198 / 0.0018
    two_phase  two / row / lane / staged / ""  0.025     0.049    0.090           0             0.0198 / 0.0025   (each form the same figures)
    near_far_from_aabb 0.059 (the fused range's nears / fars included), sph_from_ray 0.0042.
    With too little room (caps not asserted there, see the test): 0.0144 of the gaps.
The file's 301 tests take 10.2 s in all; the slowest (blob-b2, 257 rays, 6 200 samples) 0.20 s.
"""
import numpy as np
import pytest
import torch

import march_ref as R
from util import to_np

pytestmark = pytest.mark.gpu

FILL, GUARD = 7.5, 64
TRAIN_CASES = list(R.PLAN)
_FIELDS = {}


def _fields(name):
    if name not in _FIELDS:
        _FIELDS[name] = R.fields(name)
    return _FIELDS[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _buffers(rows, fill=FILL):
    return [torch.full((rows + GUARD, k), fill, device="cuda") for k in (3, 3, 2)]


def _guard_ok(bufs, rows):
    return all(bool((b[rows:] == FILL).all()) for b in bufs)


def _train_form(N):
    """The form foc_march_rays_train takes (raymarching.hip: FOC_MARCH_SERIAL forces one, else a wave per ray up to 16 384 rays)."""
    from focnerf_amd import _lib
    forced = _lib.get_option("FOC_MARCH_SERIAL")
    return "lane+scan" if (forced != 0 if forced >= 0 else N > 16384) else "wave"


def _run_train(f, M, counter0=(0, 0)):
    from focnerf_amd.backend import _raymarching as be
    N = f["N"]
    xyzs, dirs, deltas = _buffers(M)
    rays = torch.full((N, 3), -7, dtype=torch.int32, device="cuda")
    counter = torch.tensor(list(counter0), dtype=torch.int32, device="cuda")
    be.march_rays_train(_dev(f["o"]), _dev(f["d"]), _dev(f["bits"]), f["bound"], f["dt_gamma"], f["max_steps"], N, f["C"], f["H"], M, _dev(f["near"]),
                        _dev(f["far"]), xyzs, dirs, deltas, rays, counter, _dev(f["noise"]))
    assert _guard_ok((xyzs, dirs, deltas), M), "the guard band behind the sample arrays was written"
    return to_np(xyzs[:M]), to_np(dirs[:M]), to_np(deltas[:M]), to_np(rays), to_np(counter)


def _assert_caps(res, what, caps=True):
    """What the definition leaves undecided on this output: a strict minority, and within the caps of test_march_ref.py."""
    assert 2 * res["gaps_left_out"] < max(res["gaps"], 1) and 2 * res["samples_left_out"] < max(res["samples"], 1), (what, res["gaps_left_out"], res["samples_left_out"])
    if caps:
        assert res.gap_share <= 0.02 and res.sample_share <= 0.01, (what, res.gap_share, res.sample_share, res["left_out_by"])


def _assert_train(f, out, what, caps=True):
    res = R.check_train(f, *out)
    print(f"\n{what}: worst error / bound {({k: round(v, 4) for k, v in res['ratio'].items()})}, gaps left out {res.gap_share:.4f}, samples {res.sample_share:.4f}")
    assert res.ok, (what, res["ratio"], res["fail"])
    _assert_caps(res, what, caps)
    assert (res["samples"] > 0) == ("s" in R.MEANT[f["name"]])
    for a in (out[0], out[1], out[2]):
        if a is not None:
            assert (a[~res["written"]] == FILL).all(), f"{what}: a row outside the rays that fit was written"
    return res


@pytest.mark.parametrize("name", list(R.near_far_cases()))
def test_near_far_from_aabb(name):
    from focnerf_amd.backend import _raymarching as be
    o, d, aabb, min_near = R.near_far_cases()[name]
    N = len(o)
    nears, fars = torch.full((N + GUARD,), FILL, device="cuda"), torch.full((N + GUARD,), FILL, device="cuda")
    be.near_far_from_aabb(_dev(o), _dev(d), _dev(aabb), N, float(min_near), nears, fars)
    assert bool((nears[N:] == FILL).all()) and bool((fars[N:] == FILL).all())
    r, decided = R.near_far_ratio(to_np(nears[:N]), to_np(fars[:N]), o, d, aabb, min_near)
    print(f"\nnear_far {name}: worst error / bound {r.max():.4f}, undecided {(~decided).sum()} of {N}")
    assert r.max() <= 1.0


def test_sph_from_ray():
    from focnerf_amd.backend import _raymarching as be
    o, d, radius = R.sph_cases()
    N = len(o)
    coords = torch.full((N + GUARD, 2), FILL, device="cuda")
    be.sph_from_ray(_dev(o), _dev(d), radius, N, coords)
    assert bool((coords[N:] == FILL).all())
    r, decided = R.sph_ratio(to_np(coords[:N]), o, d, radius)
    print(f"\nsph_from_ray: worst error / bound {r.max():.4f}")
    assert decided.all() and r.max() <= 1.0


@pytest.mark.parametrize("serial", [None, 1], ids=["wave", "lane+scan"])
@pytest.mark.parametrize("name", TRAIN_CASES)
def test_march_rays_train(name, serial, lib_option):
    f = _fields(name)
    if serial is not None:
        lib_option("FOC_MARCH_SERIAL", serial)
    assert _train_form(f["N"]) == ("wave" if serial is None else "lane+scan")
    _assert_train(f, _run_train(f, f["M"]), f"march_rays_train {name} {_train_form(f['N'])}")


@pytest.mark.parametrize("serial", [None, 1], ids=["wave", "lane+scan"])
@pytest.mark.parametrize("name", ["blob-b1", "rand90-b2-cap", "rand50-b1.5"])
def test_march_rays_train_counter_base_and_too_little_room(name, serial, lib_option):
    """A counter that does not start at zero; an M that drops the rays behind it: they write nothing and their counts are the definition's."""
    if serial is not None:
        lib_option("FOC_MARCH_SERIAL", serial)
    f = _fields(name)
    total = int(_run_train(f, f["M"])[4][0])
    M = 37 + total // 2
    g = {k: v for k, v in f.items() if k != "_cfg"}
    g.update(M=M, counter0=(37, 5))
    out = _run_train(g, M, counter0=(37, 5))
    # (a dropped ray is one gap, counted by a walk over its whole length, which is undecided more often than a gap between two samples:
    # the caps are held where every ray fits, test_march_rays_train; here what is left out must be a strict minority)
    _assert_train(g, out, f"march_rays_train {name} base 37, M {M}", caps=False)
    assert (out[3][:, 1] + out[3][:, 2] > M).any()


@pytest.mark.parametrize("name", ["blob-b2", "rand50-b4-g.3", "rand50-b1.5", "rand10-b2", "empty-b2"])
def test_march_rays_train_fused_range(name):
    """foc_march_rays_train_field with aabb: the march performs the slab test itself (nears / fars are outputs, held to near_far's bound) and
    stores the encoder's coordinates; every row of enc_in / deltas up to M is written (zeros outside the rays)."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    f = _fields(name)
    N, M = f["N"], f["M"]
    o, d = _dev(f["o"]), _dev(f["d"])
    enc, _, deltas = _buffers(M)
    sh = torch.zeros(M + GUARD, 16, dtype=torch.float16, device="cuda")
    nears, fars = torch.full((N + GUARD,), FILL, device="cuda"), torch.full((N + GUARD,), FILL, device="cuda")
    rays = torch.full((N, 3), -7, dtype=torch.int32, device="cuda")
    counter = torch.zeros(2, dtype=torch.int32, device="cuda")
    scratch = torch.zeros(int(lib.foc_march_rays_train_scratch_bytes(N, f["max_steps"])) // 4 + 16, dtype=torch.int32, device="cuda")
    bits, noise, aabb = _dev(f["bits"]), _dev(f["noise"]), _dev(f["aabb"])
    check(lib.foc_march_rays_train_field(ptr(o), ptr(d), ptr(bits), f["bound"], f["dt_gamma"], f["max_steps"], N, f["C"], f["H"], M, ptr(nears), ptr(fars),
                                         ptr(enc), ptr(sh), ptr(deltas), ptr(rays), ptr(counter), ptr(noise), ptr(scratch), 0, ptr(aabb),
                                         f["min_near"], stream_of(o)), "march_rays_train_field")
    assert _guard_ok((enc, deltas), M) and bool((nears[N:] == FILL).all()) and bool((fars[N:] == FILL).all())
    r, _ = R.near_far_ratio(to_np(nears[:N]), to_np(fars[:N]), f["o"], f["d"], f["aabb"], np.float32(f["min_near"]))
    assert r.max() <= 1.0
    g = {k: v for k, v in f.items() if k != "_cfg"}
    g.update(near=to_np(nears[:N]), far=to_np(fars[:N]), normalised=True)                   # the march's own range, checked above
    out = (to_np(enc[:M]), None, to_np(deltas[:M]), to_np(rays), to_np(counter))
    res = R.check_train(g, *out)
    print(f"\nfused range {name}: worst error / bound {({k: round(v, 4) for k, v in res['ratio'].items()})}, gaps left out {res.gap_share:.4f}, samples {res.sample_share:.4f}")
    assert res.ok, (res["ratio"], res["fail"])
    _assert_caps(res, name)
    assert not out[0][~res["written"]].any() and not out[2][~res["written"]].any()


def _run_burst(b, how, flags=0):
    """how "single": foc_march_rays (zeroed slots, as its callers hand them over); "two": foc_march_rays_two_phase (NaN where it fills).
    Returns the slot arrays and, for "two", the form taken as the library's own queries and the worklist tell it: "staged" honours the
    sample-major flag, "row" fills every slot without it, "two" leaves the length of its worklist in scratch[0], "lane" leaves it zero."""
    from focnerf_amd._lib import lib, ptr, stream_of, check
    from focnerf_amd.backend import _raymarching as be
    n, s = len(b["rays_alive"]), b["n_step"]
    rows = n * s
    fills = how == "two" and bool(lib.foc_march_rays_two_phase_fills(s, flags))
    bufs = _buffers(rows)
    for a in bufs:
        a[:rows] = float("nan") if fills else 0.0
    args = (_dev(b["rays_alive"]), _dev(b["rays_t"]), _dev(b["o"]), _dev(b["d"]))
    tail = (_dev(b["bits"]), _dev(b["near"]), _dev(b["far"]))
    noise = _dev(b["noise"])
    taken = None
    if how == "single":
        be.march_rays(n, s, *args, b["bound"], b["dt_gamma"], b["max_steps"], b["C"], b["H"], *tail, *bufs, noise)
    else:
        scratch = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
        check(lib.foc_march_rays_two_phase(n, s, *(ptr(a) for a in args), float(b["bound"]), b["dt_gamma"], b["max_steps"], b["C"], b["H"], *(ptr(a) for a in tail),
                                           *(ptr(a) for a in bufs), ptr(noise), ptr(scratch), flags, stream_of(args[2])), "march_rays_two_phase")
        walkers = int(scratch[0])
        taken = "staged" if lib.foc_march_rays_two_phase_sample_major(n, s, flags | 4) else "row" if fills else ("two", walkers)
    assert _guard_ok(bufs, rows), "the guard band behind the slot arrays was written"
    return [to_np(a[:rows]) for a in bufs], taken


def _assert_burst(b, out, what, first=True):
    res = R.check_burst(b, *out)
    print(f"\n{what}: worst error / bound {({k: round(v, 4) for k, v in res['ratio'].items()})}, gaps left out {res.gap_share:.4f}, samples {res.sample_share:.4f}")
    assert res.ok, (what, res["ratio"], res["fail"])
    _assert_caps(res, what)
    assert (res["samples"] > 0) == ("s" in R.MEANT[b["name"]])
    if first:
        assert b["N"] < 3 or ((b["rays_alive"] < 0).any() and (b["rays_t"] == b["far"])[b["near"] < b["far"]].any())


def _march_rays_form(n_alive, n_step):
    """The kernel foc_march_rays takes (raymarching.hip: 16 lanes per ray up to FOC_MARCH_RAYS_ROW_MAX rays and 16 slots)."""
    from focnerf_amd import _lib
    return "row" if n_alive <= _lib.get_option("FOC_MARCH_RAYS_ROW_MAX") and n_step <= 16 else "serial"


@pytest.mark.parametrize("row_max,form", [(1000000000, "row"), (0, "serial")], ids=["row", "serial"])
@pytest.mark.parametrize("name,n_step", [c[:2] for c in R.BURSTS])
def test_march_rays(name, n_step, row_max, form, lib_option):
    """foc_march_rays in both forms on every case at n_step 1, 4, 8: a list with dead entries and a ray at its far, then a second burst
    continued from the first one's rays_t as composite_rays hands it on."""
    lib_option("FOC_MARCH_RAYS_ROW_MAX", row_max)
    b = R.burst_fields(_fields(name), n_step)
    assert _march_rays_form(len(b["rays_alive"]), n_step) == form
    out, _ = _run_burst(b, "single")
    _assert_burst(b, out, f"march_rays[{form}] {name} n_step {n_step} first")
    b2 = R.next_burst(b, out[2])
    assert (b2["rays_alive"] >= 0).any() == ("s" in R.MEANT[name]), "the second burst has no live ray"
    _assert_burst(b2, _run_burst(b2, "single")[0], f"march_rays[{form}] {name} n_step {n_step} second", first=False)


@pytest.mark.parametrize("form", ["two", "row", "lane", "staged", ""])
@pytest.mark.parametrize("name,n_step", [c[:2] for c in R.BURSTS])
def test_march_rays_two_phase(name, n_step, form, lib_option):
    """foc_march_rays_two_phase on every case in every form, both output forms; the two phases with their walkers 16 lanes per ray and one
    ray per lane (FOC_MARCH_RAYS_ROW_MAX both ways). The form taken is observed (_run_burst), not restated."""
    lib_option("FOC_OCC_MARCH_FORM", form)
    want = form or ("two" if n_step <= 2 else "staged")
    met_empty = R.PLAN[name]["occ"] != "full" and R.PLAN[name]["N"] >= 64       # (the two or three marching rays of a 5-ray case may all start in occupied cells)
    for row_max in ((1000000000, 0) if want == "two" else (None,)):
        if row_max is not None:
            lib_option("FOC_MARCH_RAYS_ROW_MAX", row_max)
        for norm in (False, True):
            b = R.burst_fields(_fields(name), n_step, normalised=norm)
            out, taken = _run_burst(b, "two", flags=int(norm))
            if want in ("two", "lane"):
                assert taken[0] == "two" and (taken[1] == 0 if want == "lane" else taken[1] > 0 or not met_empty), f"asked for {want}, the call left {taken}"
            else:
                assert taken == want, f"asked for {want}, the call took {taken}"
            _assert_burst(b, out, f"two_phase[{form or 'auto'}] {name} n_step {n_step} normalised {norm} row_max {row_max}")
