"""CPU: tests/normal_ref.py pinned on its own, before a GPU sees it.

1. dy_dx and the contracted gradient against an independent float64 torch restatement of the hash-grid interpolation under
   torch.autograd, and against central differences inside a cell;   2. the normalisation's edge cases;   3. the decode_normal_map
identity on synthetic weights (reference and package);   4. the layer chain against torch.autograd on exact data;
5. MUTANTS: each deliberately wrong variant lands outside the bound on the stated cases."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as MR        # noqa: E402
import normal_ref as R      # noqa: E402

B = 200


def _case(seed=1, n=B):
    rng = np.random.default_rng(seed)
    x, _ = R.points(rng, n)
    fresh = np.random.default_rng(seed + 50)
    x = R.settle(R.FOC14, x, lambda k: fresh.random((k, 3)).astype(np.float32))
    case = R.grid_case(f"ref{seed}", R.FOC14, x)
    table = rng.uniform(-0.5, 0.5, (int(case["off"][-1]), 2)).astype(np.float16)
    return case, table, rng


def _torch_features(case, table, x64):
    """Independent restatement: features [B, 32] of float64 positions x64 (a torch tensor that may require grad), trilinear interpolation
    written corner by corner; the cell and the rows of every (point, level) are the case's (the discrete decisions)."""
    t = torch.from_numpy(table.astype(np.float64))
    cols = []
    for l in range(case["L"]):
        lv = R.G.level(case, l)
        idx = torch.from_numpy(lv["idx"])
        cell = torch.from_numpy(lv["cell"].astype(np.float64))
        f = x64[idx] * float(lv["scale"]) + 0.5 - cell                                  # [n, 3]
        out = torch.zeros(x64.shape[0], 2, dtype=torch.float64)
        acc = torch.zeros(len(idx), 2, dtype=torch.float64)
        for k in range(8):
            w = torch.ones(len(idx), dtype=torch.float64)
            for d in range(3):
                w = w * (f[:, d] if (k >> d) & 1 else 1.0 - f[:, d])
            acc = acc + w[:, None] * t[torch.from_numpy(lv["rows"][:, k] + int(case["off"][l]))]
        out = out.index_add(0, idx, acc)
        cols.append(out)
    return torch.cat(cols, dim=1)


def test_dy_dx_and_the_contraction_equal_autograd_through_an_independent_interpolation():
    case, table, rng = _case()
    dy, mag = R.dy_dx(case, table)
    dy_g, _ = R.G.forward64(case, table)[1], None                                        # grid_backward_ref's own statement agrees too
    assert np.abs(dy - dy_g).max() <= 1e-9 * np.abs(dy).max()
    ge = rng.standard_normal((case["B"], 32))
    x64 = torch.from_numpy(case["x"].astype(np.float64)).requires_grad_(True)
    feats = _torch_features(case, table, x64)
    (feats * torch.from_numpy(ge)).sum().backward()
    gr, bound = R.contract(ge, dy, mag)
    inside = np.all((case["x"] >= 0) & (case["x"] <= 1), axis=1)
    assert (~inside).any() and (gr[~inside] == 0).all() and (x64.grad.numpy()[~inside] == 0).all()
    assert np.abs(gr - x64.grad.numpy()).max() <= 1e-11 * np.abs(gr).max()
    assert (bound > 0).all() and (bound[inside] < 1e-3 * np.abs(gr[inside]).max()).all()   # a bound that means something
    # every single derivative, one one-hot gradient at a time on a few points
    for b_, f_ in [(0, 0), (3, 7), (17, 30), (50, 31)]:
        x1 = torch.from_numpy(case["x"].astype(np.float64)).requires_grad_(True)
        _torch_features(case, table, x1)[b_, f_].backward()
        assert np.abs(x1.grad.numpy()[b_] - dy[b_, f_ // 2, :, f_ % 2]).max() <= 1e-11 * max(1.0, np.abs(dy[b_, f_ // 2]).max())


def test_dy_dx_equals_central_differences_inside_a_cell():
    case, table, _ = _case(seed=2)
    dy, _ = R.dy_dx(case, table)
    x = case["x"].astype(np.float64)
    eps = 2.0 ** -30                                                # far below the 2^-18 the case keeps from every cell wall
    with torch.no_grad():
        for d in range(3):
            e = np.zeros(3)
            e[d] = eps
            hi = _torch_features(case, table, torch.from_numpy(x + e)).numpy()
            lo = _torch_features(case, table, torch.from_numpy(x - e)).numpy()
            cd = ((hi - lo) / (2 * eps)).reshape(-1, 16, 2)
            want = dy[:, :, d, :]
            # linear in x_d inside the cell: the difference quotient is the derivative up to float64 cancellation (|f| / eps * 2^-53)
            assert np.abs(cd - want).max() <= 2.0 ** -20 * max(1.0, np.abs(want).max())


def test_normalisation_edge_cases():
    g = np.array([[0, 0, 0], [0, -3, 0], [1e30, -2e30, 2e30], [1e-40, 0, -1e-40], [np.inf, 1, 0], [np.nan, 0, 0], [1, 2, 2], [3e38, 3e38, 3e38], [5e-324, 0, 0]])
    n = R.normalise(g)
    assert (n[0] == 0).all() and np.array_equal(n[1], [0, 1, 0])
    assert np.allclose(n[2], [-1 / 3, 2 / 3, -2 / 3], atol=1e-15) and np.allclose(n[3], [-np.sqrt(0.5), 0, np.sqrt(0.5)], atol=1e-15)
    assert (n[4] == 0).all() and (n[5] == 0).all() and np.allclose(n[6], [-1 / 3, -2 / 3, -2 / 3], atol=1e-15)
    assert np.allclose(n[7], -np.ones(3) / np.sqrt(3), atol=1e-15) and np.array_equal(n[8], [-1, 0, 0])
    length = np.linalg.norm(n, axis=1)
    assert np.all((np.abs(length - 1) < 1e-15) | (length == 0))
    assert (R.encode(n[:1]) == 0.5).all() and np.array_equal(R.encode(n[1:2]), [[0.5, 1.0, 0.5]])
    nb = R.normal_bound(g, 0.0)
    assert np.allclose(nb, R.CC * R.U * R.KK)
    nb = R.normal_bound(np.array([[1.0, 0, 0], [1e-9, 0, 0]]), np.array([[1e-3] * 3, [1e-8] * 3]))
    assert np.isclose(nb[0, 0], 2e-3 + R.CC * R.U * R.KK) and np.isinf(nb[1]).all()          # all rounding: only grad_raw is compared
    # the package's own mesh helper agrees (fp32)
    from focnerf_amd.mesh import unit_normals
    ok = np.isfinite(g).all(axis=1) & (np.abs(g).max(axis=1) < 3e38) & ((np.abs(g).max(axis=1) > 1e-37) | (np.abs(g).max(axis=1) == 0))
    got = unit_normals(torch.from_numpy(g[ok].astype(np.float32))).numpy()
    assert np.abs(got - R.normalise(g[ok].astype(np.float32))).max() <= R.CC * R.U * R.KK
    assert (unit_normals(torch.tensor([[float("inf"), 1.0, 0.0], [float("nan"), 0.0, 0.0]])) == 0).all()


def test_decode_identity_on_synthetic_weights():
    rng = np.random.default_rng(3)
    N, T = 40, 12
    w = rng.random((N, T)) * rng.random((N, 1)) / T
    w[5] = 0                                                         # an empty ray
    n = rng.standard_normal((N, T, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[7] = n[7, :1]                                                  # one normal along a whole ray
    ws = w.sum(axis=1)
    acc = (w[:, :, None] * (0.5 + 0.5 * n)).sum(axis=1)
    pair = np.stack([acc + (1 - ws)[:, None], acc])
    normal, opacity = R.decode_normal_map(pair)
    s = (w[:, :, None] * n).sum(axis=1)
    want = s / np.where(ws > 0, np.linalg.norm(s, axis=1), 1)[:, None]
    assert np.abs(opacity - ws).max() < 1e-15 and (normal[5] == 0).all() and opacity[5] == 0
    keep = ws > 0
    assert np.abs(normal[keep] - want[keep]).max() < 1e-12 and np.abs(normal[7] - n[7, 0]).max() < 1e-12
    from focnerf_amd.normals import decode_normal_map
    image4 = torch.from_numpy(np.concatenate([pair, np.zeros((2, N, 1))], axis=-1).astype(np.float32))
    got_n, got_op = decode_normal_map(image4)
    assert np.abs(got_op.numpy() - ws).max() < 1e-6
    big = ws > 0.05
    assert np.abs(got_n.numpy()[big] - want[big]).max() < 1e-5 and (got_n.numpy()[5] == 0).all()


@pytest.mark.parametrize("nl", [1, 2, 3])
def test_layer_chain_equals_autograd_and_the_chained_network(nl):
    """chain_grad_enc on the float64 network's own (half-representable) activations: small-integer data, where every layer is exact and the
    layer-by-layer form, the chained form and torch.autograd must give the same numbers."""
    rng = np.random.default_rng(40 + nl)
    W = np.concatenate([rng.integers(-1, 2, 64 * 32), rng.integers(-1, 2, 64 * 64 * (nl - 1)), rng.integers(-1, 2, 16 * 64)]).astype(np.float16)
    W[rng.random(W.size) < 0.8] = 0
    x = rng.integers(-2, 3, (50, 32)).astype(np.float64)
    raw, genc = R.network64(x, W, nl)
    Ws = MR.split(W, 32, 64, nl)
    xt = torch.from_numpy(x).requires_grad_(True)
    a = xt
    fb = []
    for l in range(nl):
        a = torch.relu(a @ torch.from_numpy(Ws[l]).T)
        fb.append(a.detach().numpy())
    out0 = (a @ torch.from_numpy(Ws[nl]).T)[:, 0]
    out0.sum().backward()
    assert np.array_equal(out0.detach().numpy(), raw) and np.array_equal(xt.grad.numpy(), genc) and (genc != 0).any()
    fb = np.stack(fb)
    assert np.array_equal(fb, fb.astype(np.float16).astype(np.float64))
    q = R.chain_grad_enc(fb.astype(np.float16), W, nl)
    assert np.array_equal(q["ref"], genc) and (q["bound"] >= 0).all() and (q["bound"][q["ref"] != 0] > 0).all()


# ---------------------------------------------------------------- mutants
def _outside(got, ref, bound):
    return np.abs(got - ref) > bound


def test_contraction_mutants_land_outside_the_bound():
    case, table, rng = _case(seed=4)
    inside = np.all((case["x"] >= 0) & (case["x"] <= 1), axis=1)
    dy, mag = R.dy_dx(case, table)
    ge = rng.standard_normal((case["B"], 32))
    ref, bound = R.contract(ge, dy, mag)
    for mutant in ("axis_swapped", "lc_transposed"):
        got, _ = R.contract(ge, dy, mag, mutant=mutant)
        assert _outside(got, ref, bound)[inside].any(axis=1).all(), mutant           # every in-range point
    dy_m, _ = R.dy_dx(case, table, mutant="scale_dropped")
    got, _ = R.contract(ge, dy_m, mag)
    assert _outside(got, ref, bound)[inside].any(axis=1).all()
    dy_m, _ = R.dy_dx(case, table, mutant="oob_nonzero")
    got, _ = R.contract(ge, dy_m, mag)
    assert (~inside).sum() >= 3 and _outside(got, ref, bound)[~inside].all() and not _outside(got, ref, bound)[inside].any()
    n_ref = R.normalise(ref)
    assert (n_ref[~inside] == 0).all() and (np.linalg.norm(R.normalise(got)[~inside], axis=1) > 0.99).all()       # a non-zero normal out of range


def test_normal_mutants_land_outside_the_bound():
    rng = np.random.default_rng(6)
    g = rng.standard_normal((300, 3))
    from focnerf_amd import Placement
    Rm = Placement.rotated((1, 2, 3), 37).rotation.astype(np.float32)
    ref = R.encode(R.normalise(g), Rm)
    nb = R.rgb_bound(R.normal_bound(g, 0.0))
    for mutant in ("sign_flipped", "wrong_norm"):
        got = R.encode(R.normalise(g, mutant=mutant), Rm)
        assert _outside(got, ref, nb).any(axis=1).all(), mutant
    got = R.encode(R.normalise(g), Rm, mutant="rotation_transposed")
    assert _outside(got, ref, nb).any(axis=1).all()
    assert not _outside(R.encode(R.normalise(g), Rm), ref, nb).any()
    # a rotation that is a whole quarter turn about an axis: its transpose is the opposite turn, still outside
    Rq = Placement.rotated((0, 0, 1), 90).rotation
    assert _outside(R.encode(R.normalise(g), Rq, mutant="rotation_transposed"), R.encode(R.normalise(g), Rq), nb).any(axis=1).all()


@pytest.mark.parametrize("nl", [1, 2, 3])
def test_ignored_gates_land_outside_the_bound(nl):
    import oracle
    rng = np.random.default_rng(70 + nl)
    W = MR.weights(32, 64, nl, rng)
    x = (rng.standard_normal((120, 32)) * 0.3).astype(np.float16)
    _, fb = oracle.ffmlp_forward(x, W, 32, 64, nl, activation=0, training=True)
    q = R.chain_grad_enc(fb, W, nl)
    m = R.chain_grad_enc(fb, W, nl, mutant="gates_ignored")
    assert ((fb == 0).mean() > 0.2) and _outside(m["ref"], q["ref"], q["bound"]).any(axis=1).all()
    # the reference inside its own bound against a half-rounding model of the kernel's chain (deltas rounded to half per layer)
    Ws = MR.split(W, 32, 64, nl)
    d = np.where(fb[nl - 1] > 0, Ws[nl][0][None, :], 0.0)
    for l in range(nl - 1, 0, -1):
        d = np.where(fb[l - 1] > 0, (d @ Ws[l]).astype(np.float32).astype(np.float16).astype(np.float64), 0.0)
    got = (d @ Ws[0]).astype(np.float32)
    MR.worst_ratio(got, q, "half-rounding model")
