"""CPU: focnerf_amd.network_tcnn.NeRFNetwork has the parameter layout of FOC's nerf/network_tcnn.py on the tinycudann drop-in — checkpoints
load in both directions with strict=True — and the field plan gives it the fused paths. The reference network is built only where the reference
tree is (as tests/test_tcnn_dropin.py); the fallback builds the same modules from focnerf_amd.tcnn in FOC's configurations."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_tcnn_dropin import REF, _construct

VERDICTS = ("field", "tail", "train_forward", "infer")


def _tcnn_model(bound):
    """FOC's tcnn network's modules (network_tcnn.py:476-543) from the drop-in, on this package's renderer, without the reference tree."""
    from focnerf_amd import tcnn
    from focnerf_amd.renderer import NeRFRenderer
    mlp = lambda n, l: {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": n, "n_hidden_layers": l}

    class Model(NeRFRenderer):
        def __init__(self):
            super().__init__(bound, cuda_ray=True, density_scale=1)
            self.encoder = tcnn.Encoding(3, {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                                             "base_resolution": 16, "per_level_scale": np.exp2(np.log2(2048 * bound / 16) / (16 - 1))})
            self.sigma_net = tcnn.Network(32, 16, mlp(64, 1))
            self.yolo_feat_encoder = tcnn.Network(144, 16, mlp(16, 1))
            self.encoder_dir = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})
            self.color_net = tcnn.Network(47, 3, mlp(64, 2))

    return Model()


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)


def _check_round_trip(dropin, tmp_path):
    from focnerf_amd.checkpoint import load_checkpoint, save_checkpoint
    from focnerf_amd.network_tcnn import NeRFNetwork
    bound = dropin.bound
    fresh = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1)
    sd_new = fresh.state_dict()
    sd_old = dropin.state_dict()
    assert list(sd_new) == list(sd_old)
    assert all(sd_new[k].shape == sd_old[k].shape and sd_new[k].dtype == sd_old[k].dtype for k in sd_old)
    # the same seeded initialisation as the drop-in's modules
    for k in sd_old:
        if k.endswith(".params"):
            assert torch.equal(sd_new[k], sd_old[k]), k

    # drop-in -> fused class
    _randomise(dropin, 1)
    model = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1)
    model.load_state_dict(dropin.state_dict(), strict=True)
    for k, v in dropin.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    assert torch.equal(model.encoder.embeddings.detach().reshape(-1), dropin.encoder.params.detach())
    assert torch.equal(model.sigma_net.weights.detach(), dropin.sigma_net.params.detach())
    assert torch.equal(model.color_net.weights.detach(), dropin.color_net.params.detach())
    # fused class -> drop-in
    _randomise(model, 2)
    dropin.load_state_dict(model.state_dict(), strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(dropin.state_dict()[k], v), k
    # a checkpoint file written from the drop-in model
    path = str(tmp_path / f"dropin_{bound}.pth")
    save_checkpoint(dropin, path)
    other = NeRFNetwork(bound=bound, cuda_ray=True, density_scale=1)
    missing, unexpected = load_checkpoint(other, path)
    assert missing == [] and unexpected == []
    for k, v in dropin.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    # five optimizer groups, every parameter in one
    groups = other.get_params(1e-2)
    assert len(groups) == 5
    assert sum(len(list(g["params"])) for g in groups) == len(list(other.parameters()))


@pytest.mark.parametrize("bound", [1, 2])
def test_reference_network_checkpoints_round_trip(bound, tmp_path):
    if not os.path.isdir(os.path.join(REF, "nerf")):
        pytest.skip("reference tree not present")
    _check_round_trip(_construct("nerf.network_tcnn", bound), tmp_path)


@pytest.mark.parametrize("bound", [1, 2])
def test_dropin_modules_checkpoints_round_trip(bound, tmp_path):
    _check_round_trip(_tcnn_model(bound), tmp_path)


def test_topology_and_defaults():
    from focnerf_amd.network_tcnn import NeRFNetwork
    m = NeRFNetwork(bound=2, cuda_ray=True, density_scale=1)
    assert (m.sigma_net.input_dim, m.sigma_net.hidden_dim, m.sigma_net.num_layers, m.sigma_net.output_dim) == (32, 64, 1, 16)
    assert (m.color_net.input_dim, m.color_net.hidden_dim, m.color_net.num_layers, m.color_net.output_dim) == (48, 64, 2, 3)
    assert m.colour_input_pad == 1.0 and m.uses_object_feature
    assert float(m.encoder.per_level_scale) == float(np.exp2(np.log2(2048 * 2 / 16) / 15))
    assert NeRFNetwork(num_layers=3, num_layers_color=4).sigma_net.num_layers == 2
    assert NeRFNetwork(num_layers_color=4).color_net.num_layers == 3
    # a checkpoint of another size is refused by strict loading, not half-loaded
    sd = m.state_dict()
    sd["sigma_net.params"] = sd["sigma_net.params"][:-1]
    with pytest.raises(RuntimeError, match="sigma_net"):
        NeRFNetwork(bound=2, cuda_ray=True, density_scale=1).load_state_dict(sd)


def test_ffmlp_keeps_refusing_one_hidden_layer_without_the_opt_in():
    from focnerf_amd.ffmlp import FFMLP
    from focnerf_amd.network_tcnn import TcnnMLP
    with pytest.raises(AssertionError, match="num_layers"):
        FFMLP(32, 16, 64, 1)
    assert TcnnMLP(32, 16, 64, 1).num_layers == 1
    with pytest.raises(ValueError, match="n_hidden_layers"):
        TcnnMLP(32, 16, 64, 0)


def _plan_bits(plan):
    return tuple(bool(getattr(plan, v)) for v in VERDICTS)


def test_field_plan_rows(monkeypatch):
    from focnerf_amd import _lib
    from focnerf_amd.field import field_plan
    from focnerf_amd.network import NeRFNetwork as Plain
    from focnerf_amd.network_foc import NeRFNetwork as Foc
    from focnerf_amd.network_tcnn import NeRFNetwork
    for k in ("FOC_FUSED_FIELD", "FOC_FUSED_TAIL", "FOC_FUSED_INFER", "FOC_FUSED_HEAD", "FOC_FUSED_OCC", "FOC_RENDER_NATIVE"):
        monkeypatch.delenv(k, raising=False)
    assert _lib.get_option("FOC_FIELD_FWD_FUSED") != 0 and _lib.get_option("FOC_MLP_BWD_FUSED") != 0
    for layers in ((2, 3), (2, 4)):
        m = NeRFNetwork(num_layers=layers[0], num_layers_color=layers[1], cuda_ray=True, density_scale=1)
        p = field_plan(m)
        assert (p.sigma.num_layers, p.colour.num_layers) == (layers[0] - 1, layers[1] - 1)
        assert _plan_bits(p) == (True,) * 4
        assert not p.occ and not p.native_loop and not p.head and p.colour_input_pad == 1.0
    m = NeRFNetwork(cuda_ray=True, density_scale=1)
    # each switch off turns its verdict off (the field node carries the training forward and the inference kernel)
    for switch, off in (("FOC_FUSED_FIELD", {"field", "train_forward", "infer"}), ("FOC_FUSED_TAIL", {"tail", "train_forward"}),
                        ("FOC_FUSED_INFER", {"infer"})):
        monkeypatch.setenv(switch, "0")
        p = field_plan(m)
        assert {v for v in VERDICTS if not getattr(p, v)} == off, switch
        monkeypatch.delenv(switch)
    _lib.set_option("FOC_FIELD_FWD_FUSED", 0)
    try:
        assert {v for v in VERDICTS if not getattr(field_plan(m), v)} == {"train_forward"}
    finally:
        _lib.set_option("FOC_FIELD_FWD_FUSED", 1)
    # the rows of the other two networks keep their verdicts and a zero pad
    pf, pp = field_plan(Foc(cuda_ray=True, density_scale=1)), field_plan(Plain(cuda_ray=True))
    assert _plan_bits(pf) == (True,) * 4 and pf.head and not pf.occ and pf.colour_input_pad == 0
    assert _plan_bits(pp) == (True,) * 4 and pp.head and pp.occ and pp.native_loop and pp.colour_input_pad == 0


def test_pad_entry_points_in_header_signatures_and_library():
    from focnerf_amd import _lib
    from test_abi import _declared
    new = {"foc_color_head_forward_pad": "foc_color_head_forward", "foc_color_head_backward_pad": "foc_color_head_backward",
           "foc_field_forward_train_pad": "foc_field_forward_train", "foc_nerf_field_inference_pad": "foc_nerf_field_inference"}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared()
    for name, old in new.items():
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        old_res, old_args = _lib.SIGNATURES[old]
        # the twin is the old signature with a float before the stream
        assert res == old_res and args == old_args[:-1] + [ctypes.c_float, old_args[-1]], name
    # the old signatures are untouched
    assert len(_lib.SIGNATURES["foc_color_head_forward"][1]) == 12 and len(_lib.SIGNATURES["foc_color_head_backward"][1]) == 18
    assert len(_lib.SIGNATURES["foc_field_forward_train"][1]) == 15 and len(_lib.SIGNATURES["foc_nerf_field_inference"][1]) == 17
    assert _lib.lib.foc_abi_version() == 2


def test_pad_entry_points_validate_on_the_host():
    """No launch: a pad without an object feature, and layer counts that are not built, are refused with the reason."""
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    rc = lib.foc_field_forward_train_pad(one, one, 1, one, 1, one, 2, 64, 0, 128, one, one, 4, None, 1.0, None)
    assert rc == 1 and b"needs obj_feat" in lib.foc_last_error()
    rc = lib.foc_field_forward_train_pad(one, one, 1, one, 1, one, 4, 64, 0, 128, one, one, 4, one, 1.0, None)
    assert rc == 1 and b"(1, 4) are not built (1/2, 1/3" in lib.foc_last_error()
    rc = lib.foc_nerf_field_inference_pad(one, 1, one, 1, 0, 1, one, 1, one, 2, 64, 0, 128, one, one, None, 1.0, None)
    assert rc == 1 and b"needs obj_feat" in lib.foc_last_error()
    rc = lib.foc_nerf_field_inference(one, 1, one, 1, 0, 1, one, 4, one, 2, 64, 0, 128, one, one, None, None)
    assert rc == 1 and b"(4, 2) are not built" in lib.foc_last_error()
    rc = lib.foc_color_head_forward_pad(one, one, 1, one, 128, 64, 2, 0, one, 16, None, 1.0, None)
    assert rc == 1 and b"needs obj_feat" in lib.foc_last_error()
    rc = lib.foc_color_head_backward_pad(one, one, one, 1, None, one, 128, 64, 2, 0, one, one, one, 1 << 30, 16, None, None, 1.0, None)
    assert rc == 1 and b"needs obj_feat" in lib.foc_last_error()
