"""CPU: FOC's own tcnn networks (nerf/network_tcnn.py, legacy/nerf/network_tcnn.py of the reference) import and construct, unedited, with
focnerf_amd/dropin first on sys.path — `import tinycudann as tcnn` is served by focnerf_amd/tcnn.py. The construction tests need the
reference tree and run only where it is (as tests/test_dropin.py); the configuration and ABI checks run everywhere, without a GPU."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

REF = "/root/reference"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HASH = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16}
MLP = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}


def _mlp_params(n_in, hidden, layers):
    """[hidden x padded input] | (layers - 1) x [hidden x hidden] | [16 x hidden]"""
    return hidden * (-(-n_in // 16) * 16) + (layers - 1) * hidden * hidden + 16 * hidden


def _construct(module, bound):
    import focnerf_amd.tcnn  # noqa: F401  (loaded before the snapshot: the modules it returns stay importable afterwards)
    sys.dont_write_bytecode = True
    dropin = os.path.join(REPO, "focnerf_amd", "dropin")
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    try:
        for k in [k for k in sys.modules if k.split(".")[0] in ("nerf", "legacy", "raymarching", "gridencoder", "freqencoder", "ffmlp", "encoding",
                                                              "activation", "tinycudann")]:
            del sys.modules[k]
        sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))       # absent third-party viewer lib
        if module.startswith("legacy."):
            # legacy/nerf/renderer.py takes one helper from legacy/nerf/utils.py, whose training-harness imports (imageio, tensorboardX, cv2,
            # lpips, ...) are not installed: a stand-in module carries that helper alone
            utils = types.ModuleType("legacy.nerf.utils")
            utils.custom_meshgrid = lambda *args: torch.meshgrid(*args, indexing="ij")
            sys.modules["legacy.nerf.utils"] = utils
        sys.path.insert(0, REF)
        sys.path.insert(0, dropin)
        import tinycudann
        assert tinycudann.Network.__module__ == "focnerf_amd.tcnn"
        NeRFNetwork = __import__(module, fromlist=["NeRFNetwork"]).NeRFNetwork     # the reference file, unmodified
        return NeRFNetwork(encoding="hashgrid", bound=bound, cuda_ray=True, density_scale=1)
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]


def _check_common(net, bound, colour_params, names):
    from focnerf_amd import tcnn
    from focnerf_amd.gridencoder import level_offsets
    for name in names:
        assert type(getattr(net, name)).__module__ == "focnerf_amd.tcnn", name
    assert isinstance(net.encoder, tcnn.Encoding) and isinstance(net.encoder_dir, tcnn.Encoding)
    assert net.sigma_net.params.numel() == 3072 == _mlp_params(32, 64, 1)
    assert net.color_net.params.numel() == colour_params
    # the encoder's table: this package's GridEncoder layout at FOC's per_level_scale, two features per row
    scale = np.exp2(np.log2(2048 * bound / 16) / (16 - 1))
    rows = int(level_offsets(3, 16, scale, 16, 19)[-1])
    assert net.encoder.params.numel() == rows * 2 and net.encoder.n_output_dims == 32
    assert net.encoder_dir.params.numel() == 0 and net.encoder_dir.n_output_dims == 16
    # hash-table init U(-1e-4, 1e-4), every parameter fp32
    assert net.encoder.params.abs().max() <= 1e-4 and net.encoder.params.std() > 1e-5
    assert all(p.dtype == torch.float32 for p in net.parameters())
    sd = net.state_dict()
    assert {k for k in sd if k.endswith("params")} == {f"{n}.params" for n in names}
    assert not any("offsets" in k for k in sd), "the grid's level offsets are not part of a tcnn state_dict"
    # state_dict round trip
    twin = type(net)(encoding="hashgrid", bound=bound, cuda_ray=True, density_scale=1)
    with torch.no_grad():
        for p in twin.parameters():
            p.zero_()
    twin.load_state_dict(sd)
    for n in names:
        assert torch.equal(getattr(twin, n).params, getattr(net, n).params)
    torch.optim.Adam(net.get_params(1e-2), betas=(0.9, 0.99), eps=1e-15)


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("bound", [1, 2])
def test_foc_network_tcnn_constructs_on_the_dropin(bound):
    net = _construct("nerf.network_tcnn", bound)
    # nerf/network_tcnn.py: sigma 32 -> 64 -> 16 (one hidden layer), yolo encoder 144 -> 16 -> 16 (one hidden layer); the colour network gets
    # n_hidden_layers = num_layers_color - 1 = 2 from the constructor's default num_layers_color = 3 (the `self.num_layers_color = 2` beside it
    # is an attribute the config does not read): 47 (padded 48) -> 64 -> 64 -> 3
    _check_common(net, bound, 8192, ["encoder", "sigma_net", "yolo_feat_encoder", "encoder_dir", "color_net"])
    assert net.color_net.params.numel() == _mlp_params(47, 64, 2)
    assert net.yolo_feat_encoder.params.numel() == 2560 == _mlp_params(144, 16, 1)
    assert net.in_dim_color == 31 and net.color_net.n_input_dims == 47
    assert len(net.get_params(1e-2)) == 5


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree not present (GPU box)")
@pytest.mark.parametrize("bound", [1, 2])
def test_legacy_network_tcnn_constructs_on_the_dropin(bound):
    net = _construct("legacy.nerf.network_tcnn", bound)
    # legacy/nerf/network_tcnn.py: the colour input is SH 16 + geo 15 = 31 (padded 32), two hidden layers
    _check_common(net, bound, _mlp_params(31, 64, 2), ["encoder", "sigma_net", "encoder_dir", "color_net"])
    assert net.color_net.params.numel() == 7168
    assert len(net.get_params(1e-2)) == 4


def test_parameter_layout_and_seeded_init():
    from focnerf_amd import tcnn
    a, b = tcnn.Network(47, 3, dict(MLP)), tcnn.Network(47, 3, dict(MLP))
    assert torch.equal(a.params, b.params), "the init is seeded"
    assert not torch.equal(a.params, tcnn.Network(47, 3, dict(MLP), seed=7).params)
    # per matrix Xavier-uniform with the padded widths: [64 x 48] | [16 x 64]
    w0, w1 = a.params[:64 * 48], a.params[64 * 48:]
    assert w1.numel() == 16 * 64
    assert w0.abs().max() <= np.sqrt(6 / (64 + 48)) and w0.abs().max() > 0.9 * np.sqrt(6 / (64 + 48))
    assert w1.abs().max() <= np.sqrt(6 / (16 + 64)) and w1.abs().max() > 0.9 * np.sqrt(6 / (16 + 64))
    assert tcnn.PAD_VALUE == 1.0
    e = tcnn.Encoding(3, dict(HASH, per_level_scale=1.5))
    assert e.params.numel() == int(e._offsets[-1]) * 2 and e.n_output_dims == 32
    assert torch.equal(e.params, tcnn.Encoding(3, dict(HASH, per_level_scale=1.5)).params)
    sh = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})
    assert sh.params.numel() == 0 and sh.n_output_dims == 16 and list(sh.state_dict()) == ["params"]
    both = tcnn.NetworkWithInputEncoding(3, 4, dict(HASH, n_levels=4, log2_hashmap_size=12, per_level_scale=2.0), dict(MLP))
    assert both.params.numel() == _mlp_params(8, 64, 1) + int(both._offsets[-1]) * 2 and list(both.state_dict()) == ["params"]
    # tiled / dense-typed grids take the GridEncoder layout of their type
    assert tcnn.Encoding(3, dict(HASH, otype="TiledGrid")).params.numel() == tcnn.Encoding(3, dict(HASH, otype="Grid", type="Tiled")).params.numel()


@pytest.mark.parametrize("cfg,why", [
    (dict(MLP, otype="CutlassMLP"), "FullyFusedMLP"),
    (dict(MLP, n_neurons=256), "n_neurons"),
    (dict(MLP, n_neurons=48), "n_neurons"),
    (dict(MLP, n_hidden_layers=0), "n_hidden_layers"),
    (dict(MLP, n_hidden_layers=17), "n_hidden_layers"),
    (dict(MLP, activation="Sine"), "hidden activation"),
    (dict(MLP, output_activation="Sigmoid"), "output activation"),
    (dict(MLP, n_neurons=128, n_hidden_layers=6), "LDS"),
])
def test_unsupported_networks_are_refused_at_construction(cfg, why):
    from focnerf_amd import tcnn
    with pytest.raises(ValueError, match=why):
        tcnn.Network(32, 16, cfg)


def test_unsupported_shapes_and_encodings_are_refused_at_construction():
    from focnerf_amd import tcnn
    with pytest.raises(ValueError, match="n_output_dims"):
        tcnn.Network(32, 17, dict(MLP))
    with pytest.raises(ValueError, match="n_input_dims"):
        tcnn.Network(257, 16, dict(MLP))
    with pytest.raises(ValueError, match="Frequency"):
        tcnn.Encoding(3, {"otype": "Frequency", "n_frequencies": 6})
    with pytest.raises(ValueError, match="degree 4"):
        tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 3})
    with pytest.raises(ValueError, match="interpolation"):
        tcnn.Encoding(3, dict(HASH, interpolation="Nearest"))
    with pytest.raises(ValueError, match="Grid type"):
        tcnn.Encoding(3, dict(HASH, otype="Grid", type="Dense"))
    with pytest.raises(ValueError, match="n_features_per_level"):
        tcnn.Encoding(3, dict(HASH, n_features_per_level=3))
    with pytest.raises(ValueError, match="dtype"):
        tcnn.Encoding(3, dict(HASH), dtype=torch.float64)


def test_ffmlp_module_still_refuses_one_hidden_layer():
    """The reference's FFMLP asserts num_layers >= 2 (ffmlp.py:115); its drop-in keeps that — one hidden layer is tcnn's, through tcnn.py."""
    from focnerf_amd.ffmlp import FFMLP
    with pytest.raises(AssertionError, match="num_layers"):
        FFMLP(32, 16, 64, 1)


def test_one_hidden_layer_abi_without_a_gpu():
    """num_layers = 1 at the C ABI: a workspace size for every width (the single-pass kernel's slots at hidden, input <= 64), an undersized
    buffer refused, hidden 256 and the colour head refused with the reason — all on the host, before any launch."""
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    for I, Hd in [(32, 64), (48, 64), (16, 16), (64, 32), (144, 16), (32, 128)]:
        need = lib.foc_ffmlp_backward_workspace_bytes(I, Hd, 1)
        blob = Hd * (I + 16) * 4
        assert need >= blob
        if Hd <= 64 and I <= 64:
            assert need >= 1024 * 2 * 4096 * 4, "slots of two stages for up to 1024 workgroups"
        rc = lib.foc_ffmlp_backward(one, one, one, None, 128, I, 16, Hd, 1, 0, 6, 1, None, one, one, one, need - 1, None)
        assert rc == 1 and b"workspace of" in lib.foc_last_error()
    assert lib.foc_ffmlp_backward_workspace_bytes(32, 64, 1) < lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2)
    rc = lib.foc_ffmlp_backward_planar(one, one, one, 128, 32, 16, 64, 1, 0, 6, 1, one, one, one, lib.foc_ffmlp_backward_workspace_bytes(32, 64, 1) - 1, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error()
    rc = lib.foc_ffmlp_forward(one, one, 128, 32, 16, 256, 1, 0, 6, one, one, None)
    assert rc == 1 and b"hidden_dim 256 needs num_layers >= 2" in lib.foc_last_error()
    rc = lib.foc_ffmlp_forward(one, one, 128, 32, 16, 64, 0, 0, 6, one, one, None)
    assert rc == 1 and b"num_layers must be in [1,16]" in lib.foc_last_error()
    rc = lib.foc_color_head_forward(one, one, 1, one, 128, 64, 1, 0, one, 16, None, None)
    assert rc == 1 and b"color_head_forward: num_layers" in lib.foc_last_error()
    rc = lib.foc_color_head_backward(one, one, one, 1, None, one, 128, 64, 1, 0, one, one, one, 1 << 30, 16, None, None, None)
    assert rc == 1 and b"num_layers 2 or 3" in lib.foc_last_error()


def test_single_pass_routing_of_one_hidden_layer(monkeypatch):
    from focnerf_amd import ffmlp
    monkeypatch.setattr(ffmlp, "_fused_backward_switch", lambda: True)
    assert ffmlp.single_pass_backward(32, 64, 1) and ffmlp.single_pass_backward(48, 64, 1, ffmlp.NO_ACTIVATION)
    assert not ffmlp.single_pass_backward(144, 16, 1) and not ffmlp.single_pass_backward(32, 128, 1)
    assert not ffmlp.single_pass_backward(32, 64, 1, ffmlp.ACTIVATIONS["sine"])
    monkeypatch.setenv("FOC_MLP_RECOMPUTE", "1")
    assert not ffmlp._keeps_activations(32, 64, 1) and ffmlp._keeps_activations(144, 16, 1)
    monkeypatch.setenv("FOC_MLP_RECOMPUTE", "0")
    assert ffmlp._keeps_activations(32, 64, 1)
