"""CPU: the references of the pointwise kernels (tests/pointwise_ref.py). The SH basis from its definition against the polynomial form,
its Gram matrix on the sphere by quadrature, and every copy of the basis in the tree; the numpy fp32 model of each kernel within the
bounds on the exact inputs the GPU tests draw (worst ratio <= 1, share of elements left to the looser half check <= 1 %); and every
mutant of the issue outside the bounds on those inputs.

The GPU comparison is tests/test_gpu_pointwise_reference.py; it draws the same inputs."""
import numpy as np
import pytest
import torch

import mlp_ref as M
import pointwise_ref as P

F16, F32, F64 = np.float16, np.float32, np.float64


def _unit(n, seed):
    d = np.random.default_rng(seed).standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


# ---------------------------------------------------------------- the basis
def test_definition_and_polynomial_form_agree_on_unit_vectors():
    d = _unit(100_000, 1)
    a, b, c = P.sh16(d), P.sh16_poly(d), P.sh16(d, angles=True)
    print(f"\ndefinition vs polynomial {np.abs(a - b).max():.2e}, textbook angles vs (x + iy)^m {np.abs(a - c).max():.2e}")
    assert np.abs(a - b).max() <= 1e-13 and np.abs(a - c).max() <= 1e-13


def test_gram_matrix_is_the_identity():
    """Gauss-Legendre in z (8 nodes) times 16 equal steps in phi: exact for the degree-6 products of two degree-3 harmonics."""
    z, wz = np.polynomial.legendre.leggauss(8)
    phi = 2 * np.pi * np.arange(16) / 16
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    rho = np.sqrt(1 - zz ** 2)
    d = np.stack([rho * np.cos(pp), rho * np.sin(pp), zz], -1).reshape(-1, 3)
    w = (wz[:, None] * np.full_like(pp, 2 * np.pi / 16)).reshape(-1)
    for Y in (P.sh16(d, angles=True), P.sh16(d), P.sh16_poly(d)):
        G = (Y * w[:, None]).T @ Y
        assert np.abs(G - np.eye(16)).max() <= 1e-12
    for m in P.SH_MUTANTS:
        Y = P.sh16_poly(d, mutant=m)
        G = (Y * w[:, None]).T @ Y
        off = np.abs(P.sh16_poly(d) - Y).max()
        assert off > 1e-7, m                                   # orthonormality alone misses a swap and a sign: the definition does not
        print(f"\n{m}: Gram - I {np.abs(G - np.eye(16)).max():.2e}, basis off by {off:.2e}")


def _test_directions():
    d = P.directions(4096, 3).astype(F64)
    assert np.linalg.norm(d, axis=1).max() > 3 and (d[7] == 0).all() and np.abs(d[1:7]).sum() == 6
    return d


def test_every_copy_of_the_basis_agrees_with_the_polynomial_form():
    """focnerf_amd.shencoder, oracle.torch_cpu_nerf, background_ref and the fixed-tail test's _sh16: in float64 to 1e-14 of the terms'
    magnitude, in float32 (where the copy evaluates in its input's type) within sh16_bound; on and off the sphere."""
    import background_ref
    import test_gpu_fixed_tail_reference as ft
    from focnerf_amd.shencoder import sh_encode_deg4
    from oracle import torch_cpu_nerf
    d = _test_directions()
    want, mag, bound = P.sh16_poly(d), P.sh16_mag(d), P.sh16_bound(d)
    assert np.abs(P.sh16(d) - want).max() <= 1e-13 * mag.max()
    copies = {"shencoder": lambda a: sh_encode_deg4(torch.from_numpy(a)).numpy(), "oracle": lambda a: torch_cpu_nerf.sh_encode_deg4(torch.from_numpy(a)).numpy(),
              "background_ref": lambda a: background_ref.sh16(a)[0], "fixed_tail_test": ft._sh16}
    for name, fn in copies.items():
        got = fn(d.copy())
        assert got.dtype == F64 and np.all(np.abs(got - want) <= 1e-14 * mag), name
        if name != "fixed_tail_test":
            got32 = fn(d.astype(F32))
            assert got32.dtype == F32, name
            assert np.all(np.abs(got32.astype(F64) - want) <= bound), name
    assert np.allclose(background_ref.sh16(d)[1][:, 1:], mag[:, 1:], rtol=1e-14, atol=0)


# ---------------------------------------------------------------- models within the bounds
def _sh_run(n, seed, mutant=None):
    d = P.directions(n, seed)
    ref, bound = P.sh16(d.astype(F64)), P.sh16_bound(d)
    got = P.sh16_poly(d, F32, mutant)
    r32 = P.f32_check("model sh fp32", got, ref, bound)
    r16 = P.half_check("model sh half", P.to_half(got), ref, bound)
    return r32, r16


@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_sh_model_within_the_bound(n):
    r32, r16 = _sh_run(n, 10 + n % 97)
    print(f"\nSH model, n = {n}: fp32 {r32:.3f}, half {r16:.3f}")
    assert r32 <= 1 and r16 <= 1


def _head_run(n, mutant=None):
    c = P.head_case(n, 20 + n % 97)
    h0, gs = c["h"][:, 0], c["grad_sigma"]
    sig = P.expf(h0)
    out = {"sigma": P.f32_check("model sigma", sig, *P.head_sigma(h0)),
           "grad_h0": P.half_check("model grad_h0", P.model_head_grad_h0(h0, gs, mutant), *P.head_grad_h0(h0, gs))}
    sh = P.sh16_poly(c["dirs"], F32)
    out["cin SH"] = P.half_check("model cin SH", P.to_half(sh), P.sh16(c["dirs"].astype(F64)), P.sh16_bound(c["dirs"]))
    rgb = P.model_sigmoid_h(c["c"][:, :3], mutant)
    out["rgb"] = P.rgb_check("model rgb", rgb, c["c"][:, :3])
    out["grad_c"] = P.half_check("model grad_c", P.model_rgb_grad(c["grad_rgb"], rgb, mutant), *P.rgb_grad(c["grad_rgb"], rgb))
    return out


@pytest.mark.parametrize("n", P.HEAD_SIZES)
def test_head_models_within_the_bounds(n):
    out = _head_run(n)
    print(f"\nhead models, n = {n}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert max(out.values()) <= 1


def test_head_specials_are_what_the_issue_lists():
    c = P.head_case(257, 1)
    rgb = P.model_sigmoid_h(np.array([-17.0, -17.328125, -17.34375, -18.0], F16))
    assert rgb.tolist() == [2.0 ** -24, 2.0 ** -24, 0.0, 0.0]                 # just above 2^-25 the smallest subnormal, below it 0
    g = P.to_half(np.array([1e5, 2.0 ** -26], F32))
    assert np.isinf(g[0]) and g[1] == 0
    h0 = c["h"][:, 0]
    assert np.isnan(h0).any() and np.isinf(h0).sum() >= 2 and (np.abs(h0.astype(F64)) == 15.0078125).sum() >= 2
    assert ((h0 != 0) & (np.abs(h0.astype(F64)) < 2.0 ** -14)).any()


def _freq_run(deg, D, B, mutant=None):
    x = P.freq_inputs(B, D, 30 + deg + D + B % 89)
    out = P.model_freq_forward(x, deg, mutant)
    r = {"forward": P.f32_check("model freq forward", out, *P.freq_forward(x, deg))}
    assert np.array_equal(out[:, :D].view(np.uint32), x.view(np.uint32))
    g = np.random.default_rng(B + D).standard_normal(out.shape).astype(F32)
    clean = P.model_freq_forward(x, deg)
    r["backward"] = P.f32_check("model freq backward", P.model_freq_backward(g, clean, D, deg, mutant), *P.freq_backward(g, clean, D, deg))
    return r


@pytest.mark.parametrize("deg,D", P.FREQ_CASES)
def test_freq_models_within_the_bounds(deg, D):
    for B in P.FREQ_BATCHES:
        r = _freq_run(deg, D, B)
        assert max(r.values()) <= 1
    print(f"\nfreq models deg {deg} D {D}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))


def test_freq_model_within_the_bounds_at_the_loop_size():
    deg, D, B = P.FREQ_LOOP
    assert max(_freq_run(deg, D, B).values()) <= 1


def test_the_argument_of_the_sine_is_exact_up_to_one_addition():
    """scalbnf is exact, so the sine columns' arguments are 2^f x itself; the cosine columns' differ from 2^f x + fl32(pi/2) by one rounding."""
    x = P.freq_inputs(257, 3, 5)
    a = P.freq_args(x, 30).astype(F64)
    for f in range(30):
        assert np.array_equal(a[:, 2 * f], x.astype(F64) * 2.0 ** f)
        exact = x.astype(F64) * 2.0 ** f + float(P.HALF_PI32)
        assert np.all(np.abs(a[:, 2 * f + 1] - exact) <= 0.5 * P.ulp32(exact))
    assert float(P.HALF_PI32) == float(F32(np.pi / 2))


def _model_layer(src, Wm, act):
    """fp32 sums in k order, rounded to half, through the fp32 model of the activation."""
    acc = np.zeros((src.shape[0], Wm.shape[0]), F32)
    for k in range(src.shape[1]):
        acc = acc + src[:, k:k + 1].astype(F32) * Wm[None, :, k].astype(F32)
    pre = P.to_half(acc)
    return pre, (P.model_act_forward(act, pre) if act is not None else pre)


def _act_run(c, act, mutant=None):
    I, H, nl = c["I"], c["H"], c["nl"]
    Ws = M.split(c["W"], I, H, nl)
    fb, src = [], c["x"]
    r = {"fb": 0.0, "bb undecided": 0.0}
    for l in range(nl):
        _, a = _model_layer(src, Ws[l], act)
        fb.append(a)
        src = a
    fb = np.stack(fb)
    for l in range(nl):
        r["fb"] = max(r["fb"], P.act_forward_check(f"model fb act {act}", fb[l], M.forward_layer(l, c["x"], fb, Ws, act), act))
    bb = []
    for k in range(nl):
        fl = nl - 1 - k
        pre, _ = _model_layer(c["grad"] if k == 0 else bb[k - 1], Ws[-1].T if k == 0 else Ws[fl + 1].T, None)
        bb.append(P.act_backward_candidates(act, pre, fb[fl], mutant)[0])
    for k in range(nl):
        q = M.delta(k, c["grad"], fb, bb, Ws, act)
        r["bb undecided"] = max(r["bb undecided"], P.act_delta_check(f"model bb act {act}", bb[k], q, fb[nl - 1 - k], act))
    return r


@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("I,H,nl", P.ACT_SHAPES)
def test_activation_models_within_the_bounds(I, H, nl, act):
    for B in P.ACT_BATCHES:
        r = _act_run(P.act_case(I, H, nl, B, 40 + B, act=act), act)
        assert r["fb"] <= 1
    print(f"\nactivation {P.ACT_NAMES[act]} {I}x{H}x{nl}: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))


@pytest.mark.parametrize("act", P.ACTS)
def test_activation_models_over_gradient_scales(act):
    for s in M.SCALES:
        assert _act_run(P.act_case(32, 64, 2, 333, 60 + s, scale=2.0 ** s, act=act), act)["fb"] <= 1


@pytest.mark.parametrize("act", P.ACTS)
def test_activation_models_on_every_half(act):
    """The sweep of the GPU test on the model: every finite half through the function, against float64."""
    x = P.all_halves()
    got = P.model_act_forward(act, x)
    r = P.through_half(f"model sweep act {act}", got, x.astype(F64), 0.0, lambda v: P.act_ref(act, v), max_loose=None)
    print(f"\nevery half through {P.ACT_NAMES[act]}: worst {r:.3f}")
    assert r <= 1
    c = P.sweep_case()
    Ws = M.split(c["W"], c["I"], c["H"], c["nl"])
    assert np.array_equal(M.forward_layer(0, c["x"], None, Ws, M.NONE)["ref"][:, :16], x.astype(F64))
    fb = np.zeros((1, c["B"], 64), F16)
    fb[0, :, :16] = got
    q = M.delta(0, c["grad"], fb, None, Ws, M.NONE)
    assert np.array_equal(q["ref"][:, :16], c["grad"].astype(F64)) and q["count"].max() == 1
    assert len(P.act_backward_candidates(act, c["grad"], got)) == (2 if act == P.SOFTPLUS else 1)


# ---------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", P.SH_MUTANTS)
def test_sh_mutants_fall_outside(mutant):
    with pytest.raises(AssertionError, match="outside"):
        _sh_run(257, 11, mutant)


@pytest.mark.parametrize("mutant", P.HEAD_MUTANTS)
def test_head_mutants_fall_outside(mutant):
    with pytest.raises(AssertionError, match="outside|not halves"):
        _head_run(257, mutant)


@pytest.mark.parametrize("mutant", P.FREQ_MUTANTS)
def test_freq_mutants_fall_outside(mutant):
    with pytest.raises(AssertionError, match="outside"):
        _freq_run(10, 3, 257, mutant)


@pytest.mark.parametrize("mutant,act", [("squareplus_factor_in_half", P.SQUAREPLUS), ("sigmoid_factor_in_fp32", P.SIGMOID)])
def test_activation_mutants_fall_outside(mutant, act):
    with pytest.raises(AssertionError, match="none of the candidates"):
        _act_run(P.act_case(32, 64, 2, 333, 40 + 333, act=act), act, mutant)


def test_mutant_lists_are_the_issue_s():
    assert len(P.SH_MUTANTS) + len(P.HEAD_MUTANTS) + len(P.FREQ_MUTANTS) + len(P.ACT_MUTANTS) == 11
