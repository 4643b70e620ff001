"""CPU: pin the float64 reference of the background model (tests/background_ref.py) that the GPU tests measure csrc/background.hip
against — against the CPU torch restatement of the reference's encoders with autograd (oracle/torch_cpu_nerf.py), against the C
oracle's grid encoder at D = 2, against autograd's numerical gradient — and its error bound against an fp32 evaluation of the same
expressions, on the cases the GPU tests use; the share of undecided ReLU gates of every such case stays under its cap."""
import numpy as np
import pytest
import torch

import oracle
import background_ref as br
from oracle.torch_cpu_nerf import HashGridCPU, sh_encode_deg4

SMALL = [k for k, v in br.cases().items() if v[0] <= 4097]
SHARES = {}         # case -> share of undecided (ray, neuron) pairs
WORST = {}          # output -> worst ratio of the fp32 evaluation to the bound


def test_level_parameters_are_the_oracles():
    for l, (sc, res) in enumerate(br.levels(br.LOG2_SCALE, br.BASE_RESOLUTION)):
        assert oracle.grid_level_params(l, br.LOG2_SCALE, br.BASE_RESOLUTION) == (float(sc), res)
    assert [r for _, r in br.levels(br.LOG2_SCALE, br.BASE_RESOLUTION)] == [16, 81, 407, 2048]


def _torch_chain(log2_hashmap_size, seed):
    torch.manual_seed(seed)
    enc = HashGridCPU(input_dim=2, num_levels=4, level_dim=2, base_resolution=16, log2_hashmap_size=log2_hashmap_size, desired_resolution=2048).double()
    with torch.no_grad():
        enc.embeddings.uniform_(-0.5, 0.5)
    l0, l1 = torch.nn.Linear(24, 64, bias=False).double(), torch.nn.Linear(64, 3, bias=False).double()

    def f(emb, W0, W1, coords, d):
        h = torch.func.functional_call(enc, {"embeddings": emb}, (coords,))
        h = torch.cat([sh_encode_deg4(d), h], -1)
        return torch.sigmoid(torch.relu(h @ W0.T) @ W1.T)
    return enc, l0.weight.detach().clone(), l1.weight.detach().clone(), f


@pytest.mark.parametrize("log2_hashmap_size", [9, 5])
def test_smooth_chain_is_the_torch_restatement_with_autograd(log2_hashmap_size):
    """Every fp16 rounding off and float64 positions: rgb and the three gradients agree with HashGridCPU(input_dim=2) + the SH
    polynomials + two bias-free linear layers under autograd to float64 noise. 2^9 rows: level 0 dense, levels 1-3 hashed; 2^5: all
    hashed. (SHEncoderCPU casts its input to fp32, so the float64 chain calls its polynomials directly.)"""
    enc, W0, W1, f = _torch_chain(log2_hashmap_size, 0)
    coords, d = br.rays(257, 3)
    g = np.random.default_rng(0).normal(0, 1, (257, 3))
    emb = enc.embeddings.detach().clone().requires_grad_(True)
    W0.requires_grad_(True), W1.requires_grad_(True)
    rgb = f(emb, W0, W1, torch.from_numpy(coords).double(), torch.from_numpy(d).double())
    ge, g0, g1 = torch.autograd.grad(rgb, [emb, W0, W1], torch.from_numpy(g))
    fwd = br.forward(coords, d, emb.detach().numpy(), enc.offsets.numpy(), br.LOG2_SCALE, br.BASE_RESOLUTION, W0.detach().numpy(),
                     W1.detach().numpy(), half=False, pos32=False)
    assert not fwd["inside"].all() and fwd["inside"].sum() > 200
    bwd = br.backward(fwd, g)
    for name, got, want in (("rgb", fwd["rgb"], rgb), ("grad_embeddings", bwd["grad_embeddings"], ge), ("dW0", bwd["dW0"], g0), ("dW1", bwd["dW1"], g1)):
        want = want.detach().numpy()
        assert np.abs(want).max() > 1e-3
        assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), name


def test_torch_restatement_passes_gradcheck():
    enc, W0, W1, f = _torch_chain(5, 1)
    coords, d = br.rays(6, 0)
    coords, d = torch.from_numpy(coords).double(), torch.from_numpy(d).double()
    args = [t.detach().clone().requires_grad_(True) for t in (enc.embeddings, W0, W1)]
    assert torch.autograd.gradcheck(lambda e, a, b: f(e, a, b, coords, d), args, eps=1e-6, atol=1e-7, fast_mode=True)


@pytest.mark.parametrize("grid", "abc")
def test_grid_stage_is_the_compiled_oracles(grid):
    """fp32 positions, no fp16 rounding: the four levels' pairs against orc_grid_encode_forward at D = 2 on an fp32 table, and the table
    gradient against orc_grid_encode_backward; the bound is the fp32 sums' own (4 U sum |w e|; per row count U sum |addends|)."""
    coords, d = br.rays(1500, 5)
    emb, off = br.table(grid, 0.5), br.GRIDS[grid]
    W0, W1 = br.weights("lin")
    fwd = br.forward(coords, d, emb, off, br.LOG2_SCALE, br.BASE_RESOLUTION, W0, W1, half=False)
    u = (coords + np.float32(1)) / np.float32(2)
    want = oracle.grid_encode_forward(u, emb, off, 2, 2, 4, br.LOG2_SCALE, br.BASE_RESOLUTION)          # [L,B,C]
    got = fwd["x"][:, 16:].reshape(-1, 4, 2).transpose(1, 0, 2)
    assert (want[:, ~fwd["inside"]] == 0).all() and (got[:, ~fwd["inside"]] == 0).all() and (~fwd["inside"]).sum() > 50
    assert np.abs(got - want).max() <= 8 * br.U * 0.5 and np.abs(want).max() > 0.3
    gg = np.random.default_rng(1).normal(0, 1, (1500, 8)).astype(np.float32)
    want = oracle.grid_encode_backward(np.ascontiguousarray(gg.reshape(-1, 4, 2).transpose(1, 0, 2)), u, off, off[-1], 2, 2, 4, br.LOG2_SCALE,
                                       br.BASE_RESOLUTION)
    got = br.table_gradient(fwd, gg)
    sum_abs = br.table_gradient(dict(fwd, wts=np.abs(fwd["wts"])), np.abs(gg))
    count = np.bincount(fwd["rows"][fwd["inside"]].ravel(), minlength=off[-1])[:, None]
    assert (np.abs(got - want) <= (count + 1) * br.U * sum_abs).all() and np.abs(want).max() > 1
    if grid == "b":
        assert count[off[1]:].min() > 20, "every hashed row is shared"


def _ratio(name, got, want, bound, worst):
    got, want, bound = (np.asarray(a, np.float64) for a in (got, want, bound))
    err = np.abs(got - want)
    assert np.isfinite(err).all() and np.isfinite(bound).all(), name
    assert not (err[bound == 0] > 0).any(), f"{name}: a value with a zero bound differs"
    r = float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))
    worst[name] = max(worst.get(name, 0.0), r)
    assert r <= 1.0, f"{name}: fp32 evaluation at {r:.3g} of the bound"


@pytest.mark.parametrize("name", SMALL)
def test_fp32_evaluation_stays_inside_the_bounds(name):
    """The dry run of the GPU assertion: the reference's own expressions in fp32 (numpy float32 sums in BLAS's order, np.exp) against
    float64 within bounds(), rgb and every gradient for each channel of grad_rgb alone and all three; both modes' table bound."""
    c = br.make_case(name)
    f64 = c["fwd"]
    f32 = br.forward(c["coords"], c["rays_d"], c["emb"], c["offsets"], br.LOG2_SCALE, br.BASE_RESOLUTION, c["W0"], c["W1"], dtype=np.float32)
    worst = {}
    assert np.array_equal(f32["rows"], f64["rows"]) and np.array_equal(f32["wts"], f64["wts"])
    _ratio("rgb", f32["rgb"], f64["rgb"], f64["E_rgb"], worst)
    flipped = (f32["a"] > 0) != (f64["a"] > 0)
    assert not (flipped & ~f64["undecided"]).any(), "a ReLU gate flipped outside the undecided mask"
    for combo in br.COMBOS:
        g = br.only(c["grad_rgb"], combo)
        b64, b32 = br.backward(f64, g), br.backward(f32, g)
        for det in (False, True):
            bd = br.bounds(f64, b64, deterministic=det)
            _ratio("grad_embeddings", b32["grad_embeddings"].astype(np.float32), b64["grad_embeddings"], bd["grad_embeddings"], worst)
        _ratio("dW0", b32["dW0"], b64["dW0"], bd["dW0"], worst)
        _ratio("dW1", b32["dW1"], b64["dW1"], bd["dW1"], worst)
        assert c["N"] < 63 or (np.abs(b64["dW0"]).max() > 0 and np.abs(b64["dW1"]).max() > 0 and np.abs(b64["grad_embeddings"]).max() > 0)
        assert np.isfinite(b64["dW0"]).all() and np.isfinite(b64["grad_embeddings"]).all()
    for k, v in worst.items():
        WORST[k] = max(WORST.get(k, 0.0), v)


@pytest.mark.parametrize("name", list(br.cases()))
def test_undecided_gates_stay_under_the_cap(name):
    c = br.make_case(name)
    f = c["fwd"]
    share = float(f["undecided"].mean())
    SHARES[name] = share
    assert share <= br.CAP, f"{name}: {100 * share:.3g} % of the (ray, neuron) pairs are undecided"
    assert np.isfinite(f["rgb"]).all() and np.abs(f["z"]).max() < 1000
    if c["N"] >= 63:
        uv = (c["coords"] + np.float32(1)) / np.float32(2)
        assert 0 < (~f["inside"]).sum() < c["N"] // 4, "rays outside the square, and not too many"
        assert all((t & f["inside"]).any() for t in (uv[:, 0] == 0, uv[:, 0] == 1, uv[:, 1] == 0, uv[:, 1] == 1)), "rays on each edge"
        assert all(((t) & ~f["inside"]).any() for t in (uv[:, 0] < 0, uv[:, 0] > 1, uv[:, 1] < 0, uv[:, 1] > 1)), "rays beyond each edge"
    if name == "4097-b-sat":
        assert (f["rgb"] == 1).sum() > 100 and ((f["rgb"] > 0) & (f["rgb"] < 2.0 ** -14)).sum() > 100, "saturated and subnormal sigmoids"
    if name == "4097-a-subnormal-table":
        x = np.abs(f["x"][:, 16:])
        assert ((x > 0) & (x < 2.0 ** -14)).mean() > 0.3, "subnormal grid features"


def test_a_wrong_corner_weight_leaves_the_bounds():
    """The bound is tight enough to see a small mistake: with the weights of corners 1 and 2 swapped on the backward, the float64
    table gradient itself leaves the bounds."""
    c = br.make_case("129-c")
    f, g = c["fwd"], c["grad_rgb"]
    b, bm = br.backward(f, g), br.backward(dict(f, wts=f["wts"][:, :, [0, 2, 1, 3]]), g)
    assert (np.abs(bm["grad_embeddings"] - b["grad_embeddings"]) > br.bounds(f, b)["grad_embeddings"]).any()
