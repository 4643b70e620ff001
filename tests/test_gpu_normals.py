"""GPU: surface normals from the density field (csrc/normals.hip foc_field_normals; focnerf_amd/normals.py; channels="normal" through
render_field4, the culled lists and the combiner; mesh.extract_geometry(normals="field")) against tests/normal_ref.py.

1. stage by stage on the kernel's own operands, no sample left out;   2. exactly representable data, the chained float64 network;
3. every subset of the outputs, twice;   4. the three render_field4 paths;   5. two objects combined, decoded;   6. mesh normals;
7. the autograd fallback.

Grid: the FOC shape with log2_hashmap_size 14 (most levels hash, a 0.4 MB table), embeddings uniform in [-0.5, 0.5] (the 1e-4
initialisation puts every pre-activation at the gate), weights at their initialisation."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mlp_ref as MR        # noqa: E402
import normal_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS, SIZES = (1, 2, 3), (1, 65, 257, 1000)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    assert torch.equal(_bits(got), _bits(want)), tag


def _network(nl):
    """network.NeRFNetwork with `nl` hidden layers in the sigma network (one: tinycudann's one-hidden-layer FFMLP, network_tcnn.TcnnMLP)."""
    from focnerf_amd import network
    m = network.NeRFNetwork(num_layers=max(nl, 2), bound=1, cuda_ray=False)
    if nl == 1:
        from focnerf_amd.network_tcnn import TcnnMLP
        m.sigma_net = TcnnMLP(32, 16, 64, 1)
    return m


@functools.lru_cache(maxsize=None)
def _model(nl, seed=0):
    from focnerf_amd.gridencoder import GridEncoder
    torch.manual_seed(100 * seed + nl)
    m = _network(nl)
    m.encoder = GridEncoder(log2_hashmap_size=14, desired_resolution=2048)
    m = m.cuda().eval()
    m.encoder.embeddings.data.uniform_(-0.5, 0.5)
    return m


@functools.lru_cache(maxsize=None)
def _points(M):
    rng = np.random.default_rng(7000 + M)
    x, n_plain = R.points(rng, M)
    fresh = np.random.default_rng(7100 + M)
    keep = x[n_plain:].copy()
    x = R.settle(R.FOC14, x, lambda n: fresh.random((n, 3)).astype(np.float32))
    inside = np.all((x >= 0) & (x <= 1), axis=1)
    if M >= 65:                                                      # the edge and outside points are still there
        assert (~inside).sum() >= 3 and (x[inside] == 0).any() and (x[inside] == 1).any() and np.array_equal(x[n_plain:][~inside[n_plain:]], keep[~inside[n_plain:]])
    return x, inside


def _rotation():
    from focnerf_amd import Placement
    return Placement.rotated((1, 2, 3), 37).rotation


def _launch(model, xn, rot=None, **want):
    from focnerf_amd import normals
    r = normals.rotation_tensor(rot, xn.device)
    out = normals._launch(model, xn, r, **want)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- 1. stage by stage
@functools.lru_cache(maxsize=None)
def _stage(nl, M):
    """The full call on the case's points, the plain encoder + MLP forward on the same points, and the float64 dy_dx — computed once."""
    from focnerf_amd.backend import _gridencoder, _ffmlp
    from focnerf_amd.field import field_infer
    model = _model(nl)
    x, inside = _points(M)
    xn = torch.from_numpy(x).to(DEV)
    sigma, grad_raw, rgb, genc = _launch(model, xn, None, want_grad=True, want_rgb=True, want_enc=True)
    _, _, rgb_rot, _ = _launch(model, xn, _rotation(), want_sigma=False, want_rgb=True)
    enc, sn = model.encoder, model.sigma_net
    emb, w = enc.embeddings.detach().half().contiguous(), sn.weights.detach().half().contiguous()
    grid = enc.spec()
    rows = torch.empty(M, 32, dtype=torch.half, device=DEV)
    _gridencoder.grid_encode_forward(xn, emb, enc.offsets, rows, M, 3, 2, 16, grid.log2_scale, grid.base_resolution, None, *grid.tail(), out_bl=True)
    fb = torch.empty(nl, M, 64, dtype=torch.half, device=DEV)
    h = torch.empty(M, 16, dtype=torch.half, device=DEV)
    _ffmlp.ffmlp_forward(rows, w, M, 32, 16, 64, nl, 0, 6, fb, h)
    dirs = torch.nn.functional.normalize(torch.from_numpy(np.random.default_rng(5).standard_normal((M, 3)).astype(np.float32)).to(DEV), dim=-1)
    sigma_infer, _ = field_infer(model, xn, dirs)
    torch.cuda.synchronize()
    case = R.grid_case(f"stage_{nl}_{M}", R.FOC14, x)
    assert np.array_equal(case["off"], enc.offsets.cpu().numpy()) and abs(case["S"] - grid.log2_scale) < 1e-12
    assert sum(int(R.G.level(case, l)["near"].sum()) for l in range(16)) == 0
    dy, mag = R.dy_dx(case, emb.cpu().numpy())
    to = lambda t: t.cpu().numpy()
    return dict(x=x, inside=inside, sigma=sigma, sigma_infer=sigma_infer, grad_raw=to(grad_raw), rgb=to(rgb), rgb_rot=to(rgb_rot), genc=to(genc),
                fb=to(fb), W=to(w), dy=dy, mag=mag, hashed=[bool(R.G.level(case, l)["hashed"]) for l in range(16)])


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("nl", LAYERS)
def test_stage_by_stage(nl, M):
    s = _stage(nl, M)
    inside = s["inside"]
    assert sum(s["hashed"]) >= 8                                     # most levels hash
    # sigma: the bits of the inference path
    _same(s["sigma"], s["sigma_infer"], "sigma")
    # grad_enc against the float64 deltas / grad_inputs built from the plain forward's forward_buffer
    q = R.chain_grad_enc(s["fb"], s["W"], nl)
    worst_enc = MR.worst_ratio(s["genc"], q, f"grad_enc nl={nl} M={M}")
    assert (np.abs(s["genc"][inside]).sum(axis=1) > 0).mean() > 0.5 or M == 1
    # grad_raw against the contraction of the kernel's OWN grad_enc with the float64 dy_dx
    ref, bound = R.contract(s["genc"], s["dy"], s["mag"])
    err = np.abs(s["grad_raw"].astype(np.float64) - ref)
    worst_raw = float((err / np.maximum(bound, 1e-300)).max())
    print(f"nl={nl} M={M}: worst error / bound grad_enc {worst_enc:.3f} grad_raw {worst_raw:.3f}")
    assert (err <= bound).all(), f"grad_raw: {int((err > bound).sum())} outside, worst {worst_raw:.3f}"
    # normal_rgb from the kernel's OWN grad_raw, with and without a rotation
    g = s["grad_raw"].astype(np.float64)
    nb = R.rgb_bound(R.normal_bound(g, 0.0))
    for name, rot in (("rgb", None), ("rgb_rot", _rotation())):
        want = R.encode(R.normalise(g), None if rot is None else np.asarray(rot, np.float64).astype(np.float32))
        e = np.abs(s[name].astype(np.float64) - want)
        assert (e <= nb).all(), f"{name}: worst error / bound {float((e / nb).max()):.3f}"
    length = np.linalg.norm(2.0 * s["rgb"].astype(np.float64) - 1.0, axis=-1)
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))
    # out of range: exactly nothing
    out = ~inside
    assert (s["genc"][out] == 0).all() and (s["grad_raw"][out] == 0).all() and (s["rgb"][out] == 0.5).all() and (s["rgb_rot"][out] == 0.5).all()
    if M >= 65:
        assert out.any() and (length[inside] > 0).mean() > 0.9


# ---------------------------------------------------------------- 2. exact data, chained
def _sparse(rng, rows, cols, nnz, values):
    W = np.zeros((rows, cols), np.float16)
    for r in range(rows):
        W[r, rng.choice(cols, nnz, replace=False)] = rng.choice(values, nnz)
    return W


@pytest.mark.parametrize("nl", LAYERS)
def test_exact_data_chained(nl):
    """Every intermediate exactly representable: a grid with integer level scales 2^l * 2 - 1 (per_level_scale 2, base resolution 2), table
    values in {-1, 0, 1}, points on the lattice of quarters, weight matrices with 3 (W0) / 2 (hidden) entries of +-1 per row and 2 entries
    of +-1/4 in output row 0. The chained float64 network (its own activations and gates) and the kernel must agree exactly on raw (read
    back from sigma: the nearest multiple of the data's quantum to log(sigma), and sigma within expf's 2 ulps of exp(raw)), on grad_enc and
    on grad_raw. The table of levels 8..15 is zero: with scales from 511 up the 32-term fp32 contraction would no longer be exact in
    every order (the assertion below states the condition on the data: all terms multiples of 2^-10, their absolute sum below 2^14)."""
    from focnerf_amd.gridencoder import GridEncoder
    rng = np.random.default_rng(900 + nl)
    m = _network(nl)
    m.encoder = GridEncoder(per_level_scale=2, base_resolution=2, log2_hashmap_size=14)
    m = m.cuda().eval()
    enc = m.encoder
    off = enc.offsets.numpy() if not enc.offsets.is_cuda else enc.offsets.cpu().numpy()
    table = rng.integers(-1, 2, (int(off[-1]), 2)).astype(np.float16)
    table[off[8]:] = 0
    mats = [_sparse(rng, 64, 32, 3, [-1.0, 1.0])] + [_sparse(rng, 64, 64, 2, [-1.0, 1.0]) for _ in range(nl - 1)]
    Wout = _sparse(rng, 16, 64, 2, [-1.0, 1.0])
    Wout[0] = 0
    Wout[0, rng.choice(64, 2, replace=False)] = rng.choice([-0.25, 0.25], 2)
    W = np.concatenate([a.reshape(-1) for a in mats + [Wout]]).astype(np.float16)
    enc.embeddings.data.copy_(torch.from_numpy(table.astype(np.float32)))
    m.sigma_net.weights.data.copy_(torch.from_numpy(W.astype(np.float32)))
    q = np.arange(5, dtype=np.float32) / 4
    x = np.stack(np.meshgrid(q, q, q, indexing="ij"), -1).reshape(-1, 3)
    x = np.concatenate([x, x[:13] * 0 + np.float32(1.25)]).astype(np.float32)       # 138 points: a ragged tile, 13 of them outside
    spec = (3, 2, 16, 2, 14, 2 * 2 ** 15, 0, False, 0)
    case = R.grid_case("exact", spec, x)
    assert np.array_equal(case["off"], off) and case["S"] == 1.0
    feats, dy = R.G.forward64(case, table)                                           # [L, B, 2], [B, L, 3, 2]
    X = feats.transpose(1, 0, 2).reshape(len(x), 32)
    raw, genc = R.network64(X, W, nl)
    terms = genc.reshape(-1, 16, 1, 2) * dy
    graw = terms.sum(axis=(1, 3))
    for v in (X, raw, genc, terms):
        assert np.all(v * 1024 == np.round(v * 1024))
    assert np.array_equal(X, X.astype(np.float16).astype(np.float64)) and np.abs(terms).sum(axis=(1, 3)).max() < 2 ** 14
    assert np.abs(raw).max() < 80 and (genc != 0).any() and (graw != 0).any() and len(np.unique(raw)) > 4
    sigma, grad_raw, _, ge = _launch(m, torch.from_numpy(x).to(DEV), None, want_grad=True, want_enc=True)
    sig = sigma.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.round(np.log(sig) * 1024) / 1024, raw)
    assert (np.abs(sig - np.exp(raw)) <= 2 * np.spacing(np.exp(raw).astype(np.float32))).all()
    assert np.array_equal(ge.cpu().numpy().astype(np.float64), genc)
    assert np.array_equal(grad_raw.cpu().numpy().astype(np.float64), graw)


# ---------------------------------------------------------------- 3. outputs with NULLs
def test_every_subset_of_the_outputs_and_twice():
    model = _model(2)
    x, _ = _points(257)
    xn = torch.from_numpy(x).to(DEV)
    names = ("want_sigma", "want_grad", "want_rgb", "want_enc")
    full = _launch(model, xn, _rotation(), **{n: True for n in names})
    again = _launch(model, xn, _rotation(), **{n: True for n in names})
    for a, b, n in zip(full, again, names):
        _same(a, b, ("twice", n))
    for k in range(1, 4):
        for pick in itertools.combinations(range(4), k):
            got = _launch(model, xn, _rotation(), **{n: (i in pick) for i, n in enumerate(names)})
            for i, n in enumerate(names):
                if i in pick:
                    _same(got[i], full[i], (pick, n))
                else:
                    assert got[i] is None


# ---------------------------------------------------------------- 4. the render_field4 paths
def _rays(N, seed=3):
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.4, 0.4, (N, 2)), np.full((N, 1), 2.5)], -1)
    d = rng.uniform(-0.15, 0.15, (N, 3)) - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return torch.from_numpy(o.astype(np.float32)).to(DEV), torch.from_numpy(d.astype(np.float32)).to(DEV)


@functools.lru_cache(maxsize=None)
def _sphere():
    from focnerf_amd import raymarching, synthetic
    from focnerf_amd.fixedcull import Occupancy
    grid = synthetic.analytic_density_grid(1, radius_frac=0.35, device=DEV)
    return Occupancy(raymarching.packbits(grid, 25.0), grid.shape[0], 128, 1)


@pytest.mark.parametrize("path", ["dense", "occupancy", "placed"])
def test_render_field4_normal_channels(path):
    from focnerf_amd import Placement, raymarching
    from focnerf_amd.fixedcull import fixed_cull, fixed_cull_emit
    from focnerf_amd.fixedstep import fixed_sample, render_field4
    from focnerf_amd.normals import field_normals
    N, T = 70, 96
    model = _model(2)
    o, d = _rays(N)
    P = Placement.rotated((1, 2, 3), 37, translation=(0.1, -0.05, 0.0), scale=0.8) if path == "placed" else None
    box = torch.tensor([-1.5] * 3 + [1.5] * 3, dtype=torch.float32, device=DEV) if P is not None else None
    kw = dict(num_steps=T, occupancy=None if path == "dense" else _sphere(), placement=P, scene_aabb=box)
    rgb4 = render_field4(model, o, d, **kw)
    nrm4 = render_field4(model, o, d, channels="normal", **kw)
    _same(nrm4[..., 0].contiguous(), rgb4[..., 0].contiguous(), "sigma channel")
    aabb = box if P is not None else model.aabb_infer
    nears, fars = raymarching.near_far_from_aabb(o, d, aabb, model.min_near)
    if path == "dense":
        enc_in, _ = fixed_sample(o, d, nears, fars, aabb, None, T, model.bound, ray_block=0)     # [N * T, 3], ray-major
        _, direct = field_normals(model, enc_in)
        direct = direct.view(N, T, 3)
    else:
        occ = kw["occupancy"]
        mask, offsets, count = fixed_cull(o, d, nears, fars, aabb, T, occ, P, None if P is None else model.aabb_infer)
        m_occ = int(count.item())
        assert 0 < m_occ < N * T
        enc_c, _ = fixed_cull_emit(o, d, nears, fars, aabb, T, model.bound, mask, offsets, m_occ, P)
        _, rgb_c = field_normals(model, enc_c, None if P is None else P.rotation)
        # compact order: rows (block, step), lanes ascending (tests/test_gpu_combine_culled.py Obj.slot)
        words = mask.cpu().numpy().view(np.uint64).reshape(-1, T)                               # [nblk, T]
        occb = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
        direct = torch.zeros(occb.shape[0] * 64, T, 3, device=DEV)
        blk, step, lane = np.nonzero(occb)
        direct[torch.from_numpy(blk * 64 + lane).to(DEV), torch.from_numpy(step).to(DEV)] = rgb_c
        direct = direct[:N]
    kept = (rgb4[..., 1:] != 0).any(dim=-1) | (nrm4[..., 1:] != 0).any(dim=-1)                # the pack's own-weight mask (an rgb of exactly 0 0 0 aside)
    assert kept.any() and ((~kept).any() or path == "dense")               # (a random dense field keeps every sample)
    want = torch.where(kept[..., None], direct, torch.zeros_like(direct))
    _same(nrm4[..., 1:].contiguous(), want.contiguous(), "normal channels")
    assert torch.equal((rgb4[..., 1:] != 0).any(dim=-1), kept)                                  # the same mask in both renders


# ---------------------------------------------------------------- 5. combined
def test_two_objects_combined_and_decoded():
    from focnerf_amd import Placement
    from focnerf_amd.combine import combine_packed, placed_field_fns, render_scene_culled
    from focnerf_amd.normals import decode_normal_map
    N, T = 70, 96
    models, occs = [_model(2), _model(3)], [_sphere()] * 2
    placements = [Placement.rotated((1, 2, 3), 37, translation=(-0.3, 0.05, 0.0), scale=0.75), None]
    box = torch.tensor([-2.0] * 3 + [2.0] * 3, dtype=torch.float32, device=DEV)
    o, d = _rays(N, seed=4)
    fns, nears, fars = placed_field_fns(models, occs, placements, o, d, T, box, channels="normal")
    fields = [fn(0, N) for fn in fns]
    want_img, want_dep, want_att = combine_packed(fields, nears, fars, (1.0, 0.0), attribution=True)
    img, dep, att = render_scene_culled(models, occs, placements, o, d, T, box, max_ray_batch=64, attribution=True, channels="normal")
    for name, g, w in [("image4", img, want_img), ("depth", dep, want_dep), ("weights", att.weights, want_att.weights), ("instance", att.instance, want_att.instance)]:
        _same(g, w, name)
    _, _, att_rgb = render_scene_culled(models, occs, placements, o, d, T, box, max_ray_batch=64, attribution=True)
    assert torch.equal(att.instance, att_rgb.instance) and set(att.instance.unique().tolist()) >= {0, 1}
    # decode against the float64 select + composite + decode of the kernels' own fields
    ref_img, ref_ws, _ = R.composite([f.cpu().numpy() for f in fields], nears.cpu().numpy(), fars.cpu().numpy())
    b = R.composite_bound(T)
    assert np.abs(img[..., :3].cpu().numpy() - np.clip(ref_img, 0, 1)).max() <= b
    normal, opacity = decode_normal_map(img)
    ref_n, ref_op = R.decode_normal_map(ref_img)
    assert np.abs(opacity.cpu().numpy() - ref_op).max() <= 2 * b + R.U
    s = 2.0 * ref_img[1] - ref_op[:, None]
    nb = R.normal_bound(s, 4 * b)
    sel = np.isfinite(nb[:, 0]) & (ref_op > 0)
    assert sel.sum() > N // 2
    assert (np.abs(normal.cpu().numpy()[sel] - ref_n[sel]) <= nb[sel]).all()
    length = normal.norm(dim=-1).cpu().numpy()
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))


def test_render_normals_is_field4_composite_decode():
    from focnerf_amd import raymarching
    from focnerf_amd.combine import combine_packed
    from focnerf_amd.fixedstep import render_field4
    from focnerf_amd.normals import decode_normal_map, render_normals
    N, T = 70, 96
    model = _model(2)
    o, d = _rays(N, seed=9)
    for occ in (None, _sphere()):
        normal, opacity, encoded = render_normals(model, o, d, num_steps=T, occupancy=occ)
        field4 = render_field4(model, o, d, num_steps=T, occupancy=occ, channels="normal")
        nears, fars = raymarching.near_far_from_aabb(o, d, model.aabb_infer, model.min_near)
        image4, _ = combine_packed([field4], nears, fars, (1.0, 0.0))
        want_n, want_op = decode_normal_map(image4)
        _same(normal, want_n, "normal")
        _same(opacity, want_op, "opacity")
        _same(encoded, image4[0, :, :3].contiguous(), "encoded")
        ref_n, ref_op = R.decode_normal_map(image4.cpu().numpy())
        assert np.abs(opacity.cpu().numpy() - ref_op).max() <= 4 * R.U and (opacity > 0.25).any()       # (a random field: thin everywhere)
        hit = ref_op > 0.25
        assert np.abs(normal.cpu().numpy()[hit] - ref_n[hit]).max() <= 1e-5
        length = normal.norm(dim=-1).cpu().numpy()
        assert np.all((np.abs(length - 1) < 1e-5) | (length == 0))


# ---------------------------------------------------------------- 6. mesh
def test_mesh_field_normals(tmp_path):
    from focnerf_amd import mesh
    from focnerf_amd.normals import density_gradient
    model = _model(2)
    vol = mesh.density_volume(model, 32)
    thr = float(vol.median())
    v, f, n = mesh.extract_geometry(model, resolution=32, threshold=thr, normals="field")
    v0, f0 = mesh.extract_geometry(model, resolution=32, threshold=thr)
    assert len(f) > 0 and torch.equal(v, v0) and torch.equal(f, f0) and n.shape == v.shape and n.dtype == torch.float32
    _, grad = density_gradient(model, v)
    g = grad.cpu().numpy().astype(np.float64)
    want = R.normalise(g)
    assert np.abs(n.cpu().numpy() - want).max() <= R.CC * R.U * R.KK
    length = n.norm(dim=-1).cpu().numpy()
    assert np.all((np.abs(length - 1) < 1e-5) | (length == 0)) and (length > 0).mean() > 0.9
    path = str(tmp_path / "normals.ply")
    mesh.write_ply(path, v, f, n)
    pv, pf, pn = mesh.read_ply(path)
    assert np.array_equal(pv, v.cpu().numpy()) and np.array_equal(pf, f.cpu().numpy()) and np.array_equal(pn, n.cpu().numpy())
    nv, nf = mesh.save_mesh(model, path, 32, thr, normals="field")
    assert (nv, nf) == (len(v), len(f)) and np.array_equal(mesh.read_ply(path)[2], n.cpu().numpy())


# ---------------------------------------------------------------- 7. the fallback
def test_density_gradient_fallback_has_the_fused_routes_shapes(monkeypatch):
    from focnerf_amd.field import field_plan
    from focnerf_amd.normals import density_gradient
    model = _model(2)
    x = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (5, 13, 3)).astype(np.float32)).to(DEV)
    assert field_plan(model).normals
    with torch.no_grad():
        sigma, grad = density_gradient(model, x)
    monkeypatch.setenv("FOC_FUSED_NORMALS", "0")
    assert not field_plan(model).normals
    with torch.no_grad():
        sigma0, grad0 = density_gradient(model, x)
    for a, b_ in ((sigma, sigma0), (grad, grad0)):
        assert a.shape == b_.shape and a.dtype == b_.dtype == torch.float32 and a.device == b_.device and not b_.requires_grad
    assert sigma.shape == (5, 13) and grad.shape == (5, 13, 3) and torch.isfinite(grad0).all() and (grad0 != 0).any() and (grad != 0).any()
