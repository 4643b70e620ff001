"""CPU: torch-ngp's default network (focnerf_amd/network_linear.py) keeps the reference's parameters — state_dict, parameters() and
get_params of legacy/nerf/network.py, its seeded initialisation, its optimizer state and the cpu_network.npz parameters — packs them into
the FFMLP blobs the kernels read with the gradient routed back to each layer, gets the fused paths and the background kernel from
field_plan, and the background entry points check their arguments on the host. The reference module is built only where the reference
tree is (as tests/test_tcnn_dropin.py); elsewhere the layout is checked against tests/golden/network_linear_layout.json."""
import ctypes
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_tcnn_dropin import REF, REPO

GOLDEN = os.path.join(REPO, "tests", "golden")
KW = dict(encoding="hashgrid", bound=2, cuda_ray=True, density_scale=1, min_near=0.05, density_thresh=10)
VERDICTS = ("field", "train_forward", "tail", "infer", "occ", "native_loop", "head", "background")
SWITCHES = {"FOC_FUSED_FIELD": ("field", "train_forward", "infer", "occ", "native_loop"), "FOC_FUSED_TAIL": ("tail", "train_forward", "occ"),
            "FOC_FUSED_INFER": ("infer", "native_loop"), "FOC_FUSED_OCC": ("occ",), "FOC_RENDER_NATIVE": ("native_loop",),
            "FOC_FUSED_HEAD": ("head",), "FOC_FUSED_BG": ("background",)}


def _reference(**kw):
    """legacy/nerf/network.py, unmodified, on this package's drop-in modules (the recipe of test_tcnn_dropin._construct)."""
    sys.dont_write_bytecode = True
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    try:
        for k in [k for k in sys.modules if k.split(".")[0] in ("nerf", "legacy", "raymarching", "gridencoder", "ffmlp", "encoding", "activation")]:
            del sys.modules[k]
        sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
        utils = types.ModuleType("legacy.nerf.utils")
        utils.custom_meshgrid = lambda *args: torch.meshgrid(*args, indexing="ij")
        sys.modules["legacy.nerf.utils"] = utils
        sys.path.insert(0, REF)
        sys.path.insert(0, os.path.join(REPO, "focnerf_amd", "dropin"))
        return __import__("legacy.nerf.network", fromlist=["NeRFNetwork"]).NeRFNetwork(**kw)
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]


def _net(seed=0, **kw):
    from focnerf_amd.network_linear import NeRFNetwork
    torch.manual_seed(seed)
    return NeRFNetwork(**{**KW, **kw})


def _layout(m):
    return {"state_dict": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()],
            "parameters": [list(p.shape) for p in m.parameters()], "get_params": [[list(p.shape) for p in g["params"]] for g in m.get_params(1e-2)]}


@pytest.mark.parametrize("bg", [-1, 32])
def test_layout_matches_the_committed_list(bg):
    want = json.load(open(os.path.join(GOLDEN, "network_linear_layout.json")))["bg_off" if bg < 0 else "bg_on"]
    assert _layout(_net(bg_radius=bg)) == want


@pytest.mark.parametrize("bg", [-1, 32])
def test_layout_and_seeded_initialisation_are_the_reference_module(bg):
    if not os.path.isdir(os.path.join(REF, "legacy", "nerf")):
        pytest.skip("reference tree not present")
    torch.manual_seed(7)
    ref = _reference(**KW, bg_radius=bg)
    m = _net(seed=7, bg_radius=bg)
    assert _layout(ref) == _layout(m)
    a, b = ref.state_dict(), m.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # checkpoints both ways
    ref.load_state_dict(_net(seed=9, bg_radius=bg).state_dict(), strict=True)
    m.load_state_dict(_reference(**KW, bg_radius=bg).state_dict(), strict=True)


def test_constructor_keywords():
    from focnerf_amd.network_linear import NeRFNetwork
    m = NeRFNetwork(encoding="hashgrid", bound=2, cuda_ray=True, density_scale=1, min_near=0.05, density_thresh=10, bg_radius=-1, n_chunks=4)
    assert m.bg_net is None and not hasattr(m, "encoder_bg") and m.bound == 2 and m.cuda_ray
    m = NeRFNetwork(num_layers=3, hidden_dim=32, num_layers_color=2, hidden_dim_color=32, num_layers_bg=3, hidden_dim_bg=32, bg_radius=8)
    assert [tuple(l.weight.shape) for l in m.sigma_net] == [(32, 32), (32, 32), (16, 32)]
    assert [tuple(l.weight.shape) for l in m.color_net] == [(32, 31), (3, 32)]
    assert [tuple(l.weight.shape) for l in m.bg_net] == [(32, 24), (32, 32), (3, 32)]
    assert m.encoder_bg.input_dim == 2 and m.encoder_bg.num_levels == 4 and m.encoder_bg.embeddings.shape[0] == 697776
    assert all(l.bias is None for net in (m.sigma_net, m.color_net, m.bg_net) for l in net)


def test_optimizer_state_and_cpu_fixture_load():
    """A reference-layout Adam state (one step on every group) loads into the class's optimizer; cpu_network.npz's param/* load with
    strict=True into the class built with the fixture's small grid."""
    m = _net(bg_radius=32)
    src = _net(seed=3, bg_radius=32)
    opt = torch.optim.Adam(src.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    for p in src.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    mine = torch.optim.Adam(m.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)
    mine.load_state_dict(opt.state_dict())
    assert [tuple(s["exp_avg"].shape) for s in mine.state_dict()["state"].values()] == [tuple(p.shape) for p in m.parameters()]

    from focnerf_amd import network_linear
    from focnerf_amd.encoding import get_encoder
    g = np.load(os.path.join(GOLDEN, "cpu_network.npz"))
    nl, base, log2, des = (int(v) for v in g["encoder_cfg"])
    small = dict(num_levels=nl, base_resolution=base, log2_hashmap_size=log2, desired_resolution=des)
    saved = network_linear.get_encoder
    network_linear.get_encoder = lambda enc, **kw: get_encoder(enc, **{**kw, **(small if enc == "hashgrid" else {})})
    try:
        f = network_linear.NeRFNetwork(bound=int(g["bound"]))
    finally:
        network_linear.get_encoder = saved
    params = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}
    assert np.array_equal(f.encoder.offsets.numpy(), params["encoder.offsets"].numpy())
    f.load_state_dict(params, strict=True)
    assert torch.equal(f.color_net[2].weight, params["color_net.2.weight"])


def test_packed_blobs_and_their_gradients():
    """The FFMLP blobs: [W0 | 0 columns] | hidden | [W_last | 0 rows], each matrix row-major; the blob's gradient reaches each layer as its
    slice, the padding entries dropped."""
    from focnerf_amd.field import MlpShape, fused_mlp
    m = _net(bg_radius=32)
    shapes = {n: MlpShape.of(fused_mlp(m, n)) for n in ("sigma_net", "color_net", "bg_net")}
    assert shapes == {"sigma_net": MlpShape(32, 64, 1, 0, 6, 16), "color_net": MlpShape(32, 64, 2, 0, 6, 16), "bg_net": MlpShape(32, 64, 1, 0, 6, 16)}
    for name, width in (("sigma_net", 32), ("color_net", 31), ("bg_net", 24)):
        layers = getattr(m, name)
        blob = fused_mlp(m, name).weights
        assert blob.numel() == shapes[name].blob_numel()
        w0 = blob[:64 * 32].view(64, 32)
        assert torch.equal(w0[:, :width], layers[0].weight) and not w0[:, width:].any()
        last = blob[-16 * 64:].view(16, 64)
        assert torch.equal(last[:layers[-1].out_features], layers[-1].weight) and not last[layers[-1].out_features:].any()
        if len(layers) == 3:
            assert torch.equal(blob[64 * 32: 64 * 96].view(64, 64), layers[1].weight)
        g = torch.arange(blob.numel(), dtype=torch.float32)
        blob.backward(g)
        assert torch.equal(layers[0].weight.grad, g[:64 * 32].view(64, 32)[:, :width])
        assert torch.equal(layers[-1].weight.grad, g[-16 * 64:].view(16, 64)[:layers[-1].out_features])
    # one packing per half_cache_scope
    from focnerf_amd.field import half_cache_scope
    with torch.no_grad(), half_cache_scope():
        assert fused_mlp(m, "color_net").weights is fused_mlp(m, "color_net").weights
    assert fused_mlp(m, "color_net").weights is not fused_mlp(m, "color_net").weights


def _row(plan):
    return {v: getattr(plan, v) for v in VERDICTS}


@pytest.mark.parametrize("bg", [-1, 32])
def test_field_plan_rows(bg, monkeypatch):
    from focnerf_amd.field import field_plan
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    m = _net(bg_radius=bg)
    plan = field_plan(m)
    on = {v: True for v in VERDICTS}
    on["background"] = bg > 0
    assert _row(plan) == on and plan.colour_input_pad == 0.0 and (plan.sigma.num_layers, plan.colour.num_layers) == (1, 2)
    for switch, off in SWITCHES.items():
        monkeypatch.setenv(switch, "0")
        if switch == "FOC_FUSED_BG" and bg > 0:
            off = off + ("occ",)                  # with a background, the occupancy node takes it from the kernel (field.py)
        want = {v: on[v] and v not in off for v in VERDICTS}
        assert _row(field_plan(m)) == want, switch
        monkeypatch.delenv(switch)
    # a background the kernel does not serve: op by op, everything else unchanged; bg_radius > 0 then keeps the occupancy node off
    if bg > 0:
        from focnerf_amd.network_linear import NeRFNetwork
        torch.manual_seed(0)
        other = NeRFNetwork(**KW, bg_radius=bg, hidden_dim_bg=32)
        assert _row(field_plan(other)) == {**on, "background": False, "occ": False}
    # the existing networks never get the background path
    from focnerf_amd.network import NeRFNetwork as Plain
    assert not field_plan(Plain(bound=1)).background


def test_background_entry_points_refuse_bad_arguments_on_the_host():
    from focnerf_amd import _lib
    lib = _lib.lib
    header = open(os.path.join(REPO, "include", "focnerf.h")).read()
    for n in ("foc_background_forward", "foc_background_backward", "foc_background_backward_workspace_bytes"):
        assert n + "(" in header and n in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), n)
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    assert lib.foc_background_forward(None, one, None, 32.0, 16, one, one, 2.3, 16, one, one, None) == 1
    assert b"null pointer" in lib.foc_last_error()
    assert lib.foc_background_forward(one, one, None, 0.0, 16, one, one, 2.3, 16, one, one, None) == 1
    assert b"radius" in lib.foc_last_error()
    assert lib.foc_background_forward(None, one, one, 0.0, 16, one, one, 2.3, 16, one, None, None) == 1
    need = lib.foc_background_backward_workspace_bytes(4096)
    assert need == 64 * 1728 * 4 and lib.foc_background_backward_workspace_bytes(1 << 24) == 2048 * 1728 * 4
    rc = lib.foc_background_backward(one, one, one, None, 32.0, 4096, one, one, 2.3, 16, one, one, one, one, need - 1, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error()
    rc = lib.foc_background_backward(one, one, one, None, 32.0, 4096, one, one, 2.3, 16, one, None, one, one, need, None)
    assert rc == 1 and b"null pointer" in lib.foc_last_error()
    assert lib.foc_abi_version() == 2
