"""CPU: the C oracle's near_far_from_aabb, sph_from_ray, march_rays_train and march_rays against the float64 definition of tests/march_ref.py
(the oracle and the kernels were written by one hand from raymarching.cu and are compared bit for bit with each other only); the same checks
on an fp32 walker written apart from the oracle; and each deliberately wrong walker (march_ref.MUTANTS) rejected on a named case.

Caps on what the definition leaves undecided, per case, from the inputs and the oracle's outputs alone: gaps <= 2 %, samples <= 1 %,
near / far decisions <= 1 % of the rays. Measured on the oracle (share of gaps / of samples left out; near / far: 0 on every case but
"constructed", whose ray through an edge of the box is undecided by construction; that case is not capped):
    blob-b1 0.0065 / 0.0004  blob-b2 0.0101 / 0.0002   blob-b4 0.0112 / 0       one-ray 0 / 0            rand10-b2 0.0106 / 0
    rand50-b1 0.0012 / 0     rand50-b4-g.3 0 / 0       rand90-b2-cap 0.0029 / 0 rand50-b1.5 0.0024 / 0   full-b4-cap 0.0007 / 0
    full-b1-g.3 0 / 0        empty-b2 0.0104 / -
Bursts (march_ref.BURSTS: every case at n_step 1, 4, 8, first and continued): at most 0.02 of the gaps (blob-b2, n_step 1: 4 of 203), no
sample. The blob cases' bursts start shortly before the blob (burst_fields): from the box they would cross 150 .. 570 lattice steps of
0.0034 first, and that one gap was undecided for 20 of 42 rays of blob-b1. The seeds of PLAN are those under which every cap holds.
Worst error / bound of the oracle over all cases (asserted <= 1): deltas0 0.025, xyzs 0.026, next_sample_t 0.090, t_below_far 0;
near / far 0.059, sph 0.005 (each test prints its own: `pytest -s`).

Mutants, each applied to the fp32 walker and rejected on the case named in CAUGHT_BY, where the unmutated walker passes in the same
configuration (and on every case: first 64 rays of the two cases with 257):
skip_ignores_sign, dt_unclamped, skip_one_step_less on rand50-b4-g.3 (a skip's exit face, steps beyond dt_max, and a lookup one lattice point
early at a coarser level); level_from_pos_only, noise_scales_dt_min on blob-b4, burst_keeps_stale_slot on its burst; index_rounds,
delta1_is_dt, skip_one_step_more on blob-b1; morton_axes_swapped on rand10-b2; mip_bound_unclamped on rand50-b1.5 (the only bound below
2^(C-1)); far_inclusive on full-b4-cap's burst, whose list holds a ray with rays_t == far: `t <= far` differs from `t < far` at equality
only, which float64 can tell from an fp32 march only where the inputs make it exact. The definition and the oracle disagree nowhere: no
kernel or oracle change came out of this.
"""
import numpy as np
import pytest

import march_ref as R
import oracle

NAMES = list(R.PLAN)
_FIELDS = {}


def _fields(name):
    if name not in _FIELDS:
        _FIELDS[name] = R.fields(name)
    return _FIELDS[name]


def _oracle_train(f, M=None, counter=None):
    return oracle.march_rays_train(f["o"], f["d"], f["bits"], f["bound"], f["dt_gamma"], f["max_steps"], f["C"], f["H"], f["M"] if M is None else M,
                                   f["near"], f["far"], f["noise"], counter=counter)


def _oracle_burst(b):
    """oracle.march_rays on the live entries (it does not skip entries < 0), scattered back into the list's slots."""
    live = np.nonzero(b["rays_alive"] >= 0)[0]
    n, s = len(b["rays_alive"]), b["n_step"]
    x, d, l = oracle.march_rays(len(live), s, b["rays_alive"][live], b["rays_t"], b["o"], b["d"], b["bound"], b["dt_gamma"], b["max_steps"], b["C"], b["H"],
                                b["bits"], b["near"], b["far"], b["noise"][live])
    out = [np.zeros((n, s, k), np.float32) for k in (3, 3, 2)]
    for a, v in zip(out, (x, d, l)):
        a[live] = v[:len(live) * s].reshape(len(live), s, a.shape[-1])
    return [a.reshape(n * s, -1) for a in out]


def _assert_ok(res, what):
    assert res.ok, (what, res["ratio"], res["fail"])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_training_march_meets_the_definition(name):
    """Every rule of check_train within its bound, the caps on what is left out, and the case shows what it is meant to (march_ref.MEANT)."""
    f = _fields(name)
    out = _oracle_train(f)
    res = R.check_train(f, *out)
    print(f"\n{name}: gaps left out {res.gap_share:.4f} of {res['gaps']} {res['left_out_by']}, samples {res.sample_share:.4f} of {res['samples']}, "
          f"longest gap {res['longest_gap']} steps, rays at the cap {res['capped']}, worst ratios {res['ratio']}")
    _assert_ok(res, name)
    assert res.gap_share <= 0.02 and res.sample_share <= 0.01
    meant = R.MEANT[name]
    assert (res["samples"] > 0) == ("s" in meant) and ("g" not in meant or res["long_gaps"] > 0) and (res["capped"] > 0) == ("c" in meant)
    assert res["gaps"] > 0 and 2 * res["gaps_left_out"] < res["gaps"] and (res["samples"] == 0 or 2 * res["samples_left_out"] < res["samples"])
    assert not out[0][~res["written"]].any() and not out[2][~res["written"]].any()


@pytest.mark.parametrize("name", ["blob-b1", "rand90-b2-cap"])
def test_oracle_training_march_with_a_counter_and_too_little_room(name):
    """A sample counter that does not start at zero (the ray counter indexes the oracle's rays rows: :406, :411), and an M that drops the rays behind it: their counts are still the definition's."""
    f = dict(_fields(name), counter0=(37, 0))
    total = int(_oracle_train(f)[4][0])
    M = 37 + total // 2
    f = dict(f, M=M)
    f.pop("_cfg", None)
    out = _oracle_train(f, M=M, counter=np.array([37, 0], np.int32))
    res = R.check_train(f, *out)
    _assert_ok(res, name)
    assert (out[3][:, 1] + out[3][:, 2] > M).any() and not out[0][~res["written"]].any()


@pytest.mark.parametrize("name,n_step,normalised", R.BURSTS)
def test_oracle_burst_meets_the_definition(name, n_step, normalised):
    """march_rays from rays_t = near with dead list entries, and a second burst continued from the first one's rays_t."""
    f = _fields(name)
    b = R.burst_fields(f, n_step)
    out = _oracle_burst(b)
    if normalised:                                                     # the form foc_march_rays_two_phase stores: (x + bound) * (1 / (2 bound)) in fp32
        bb = np.float32(f["bound"])
        out[0] = np.where(out[2][:, :1] != 0, (out[0] + bb) * (np.float32(1) / (np.float32(2) * bb)), 0).astype(np.float32)
        b = dict(b, normalised=True)
    res = R.check_burst(b, *out)
    _assert_ok(res, (name, "first"))
    assert res.gap_share <= 0.02 and res.sample_share <= 0.01
    # not vacuous: slots are filled where the case has samples, some ray fills its burst and marches on, a dead entry and a ray at its far exist
    samples = "s" in R.MEANT[name]
    assert res["gaps"] > 0 and 2 * res["gaps_left_out"] < res["gaps"] and (res["samples"] > 0) == samples
    assert f["N"] < 3 or ((b["rays_alive"] < 0).any() and (b["rays_t"] == f["far"])[f["near"] < f["far"]].any())
    b2 = R.next_burst(b, out[2])
    assert (b2["rays_alive"] >= 0).any() == samples
    if not normalised:
        res2 = R.check_burst(b2, *_oracle_burst(b2))
        _assert_ok(res2, (name, "second"))
        assert res2.gap_share <= 0.02 and res2.sample_share <= 0.01 and (res2["samples"] > 0) == samples


@pytest.mark.parametrize("name", list(R.near_far_cases()))
def test_oracle_near_far_meets_the_definition(name):
    o, d, aabb, min_near = R.near_far_cases()[name]
    n, f = oracle.near_far_from_aabb(o, d, aabb, min_near)
    r, decided = R.near_far_ratio(n, f, o, d, aabb, min_near)
    print(f"\n{name}: worst ratio {r.max():.3f}, undecided {(~decided).mean():.4f}")
    assert r.max() <= 1.0
    if name == "constructed":
        want = R.near_far(o, d, aabb, min_near)
        assert (want[0] == R.FLT_MAX).sum() >= 4 and (want[0] < 1).sum() >= 2 and np.array_equal(n == np.float32(R.FLT_MAX), want[0] == R.FLT_MAX)
        assert not decided[13] and decided[:13].all()
        assert np.array_equal(np.isnan(n), np.isnan(want[0])) and np.array_equal(np.isnan(f), np.isnan(want[1]))
    else:
        assert (~decided).mean() <= 0.01 and (n == np.float32(R.FLT_MAX)).any() == ("miss" in R.PLAN[name]["kinds"])


def test_oracle_sph_from_ray_meets_the_definition():
    o, d, radius = R.sph_cases()
    got = oracle.sph_from_ray(o, d, radius)
    r, decided = R.sph_ratio(got, o, d, radius)
    want, mag, _ = R.sph_from_ray(o, d, radius)
    print(f"\nsph_from_ray: worst ratio {r.max():.3f}, undecided {(~decided).sum()}")
    assert r.max() <= 1.0 and decided.all()
    assert np.isnan(want[-3:-1]).all() and np.isnan(got[-3:-1]).all() and np.isfinite(want[:-3]).all() and np.isfinite(want[-1]).all()
    # the cases are what they claim: poles (theta = 0, pi), phi = +-pi
    assert want[0, 0] == -1.0 and want[1, 0] == 1.0 and abs(want[2, 1]) == 1.0 and want[3, 1] > 0.999999 and want[4, 1] < -0.999999


def test_morton_by_its_definition_is_the_oracles():
    c = np.random.default_rng(0).integers(0, 1024, (4096, 3)).astype(np.int32)
    assert np.array_equal(R.morton(c[:, 0], c[:, 1], c[:, 2]), oracle.morton3D(c).astype(np.int64))


def test_scalar_lookup_is_the_vectorised_one():
    """walk()'s Python-float lookup against level / cell / index / occupied on random points."""
    f = _fields("rand50-b4-g.3")
    cfg = R._cfg(f)
    rng = np.random.default_rng(3)
    seen = 0
    for _ in range(400):
        o, d, t = rng.uniform(-1, 1, 3), R._unit(rng.normal(size=3)), rng.uniform(0.05, 6.0)
        look = R.lookup(cfg, list(o), list(d), t, 0.0)
        if look is None:
            continue
        occ, x, dt, lev, n, mb, _ = look
        l2, _ = R.level(np.array(x), dt, cfg)
        n2, _ = R.cell(np.array(x), l2, cfg)
        assert lev == int(l2) and n == n2.tolist() and occ == bool(R.occupied(R.index(l2, n2, cfg), cfg["bits"])[0])
        seen += 1
    assert seen > 300


def _walker_case(name):
    """The case as the fp32 walker takes it: its first 64 rays."""
    f = _fields(name)
    if f["N"] <= 64:
        return f
    if name + "/64" not in _FIELDS:
        _FIELDS[name + "/64"] = R.first_rays(f, 64)
    return _FIELDS[name + "/64"]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_walker_meets_the_definition(name):
    f = _walker_case(name)
    _assert_ok(R.check_train(f, *R.walker_train(f)), name)
    for n_step, normalised in ((1, False), (4, False), (4, True), (8, False)):
        b = R.burst_fields(f, n_step, normalised=normalised)
        _assert_ok(R.check_burst(b, *R.walker_burst(b)), (name, n_step))


CAUGHT_BY = {"skip_ignores_sign": ("rand50-b4-g.3", "train"), "level_from_pos_only": ("blob-b4", "train"), "index_rounds": ("blob-b1", "train"),
             "far_inclusive": ("full-b4-cap", "burst"), "delta1_is_dt": ("blob-b1", "train"), "dt_unclamped": ("rand50-b4-g.3", "train"),
             "noise_scales_dt_min": ("blob-b4", "train"), "skip_one_step_more": ("blob-b1", "train"), "skip_one_step_less": ("rand50-b4-g.3", "train"),
             "morton_axes_swapped": ("rand10-b2", "train"), "mip_bound_unclamped": ("rand50-b1.5", "train"), "burst_keeps_stale_slot": ("blob-b4", "burst")}


def _walk_it(f, how, mutant):
    if how == "burst":
        b = R.burst_fields(f, 4)
        return R.check_burst(b, *R.walker_burst(b, mutant))
    return R.check_train(f, *R.walker_train(f, mutant))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_checks_reject_the_mutant(mutant):
    """On its named case the mutated walker breaks a rule or leaves a bound; the unmutated one passes in the very same configuration."""
    assert set(CAUGHT_BY) == set(R.MUTANTS)
    name, how = CAUGHT_BY[mutant]
    f = _walker_case(name)
    _assert_ok(_walk_it(f, how, None), (name, how))
    res = _walk_it(f, how, mutant)
    print(f"\n{mutant} on {name} ({how}): {res['ratio']} {res['fail'][:2]}")
    assert not res.ok
