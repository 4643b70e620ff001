"""CPU: focnerf_amd.network_tcnn_legacy.NeRFNetwork has the parameter layout of torch-ngp's legacy/nerf/network_tcnn.py on the tinycudann
drop-in — checkpoints load in both directions with strict=True — the field plan gives it every fused path but the head kernels, and the
*_pad31 entry points (column 31 of the 32-wide colour input) are declared, exported and validate their arguments on the host. The reference
network is built only where the reference tree is (as tests/test_tcnn_dropin.py); the drop-in modules in the legacy network's configuration
stand in for it everywhere."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from test_tcnn_dropin import REF, REPO, _mlp_params

LAYERS = [(2, 3), (2, 2), (3, 3)]
VERDICTS = ("field", "tail", "train_forward", "infer", "occ", "native_loop", "head")
ON = ("field", "tail", "train_forward", "infer", "occ", "native_loop")
HASH = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16}


def _mlp(layers):
    return {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": layers}


def _reference_legacy(bound, num_layers, num_layers_color):
    """legacy/nerf/network_tcnn.py, unmodified, on the drop-in (the recipe of test_tcnn_dropin._construct with the layer counts passed)."""
    import focnerf_amd.tcnn  # noqa: F401
    sys.dont_write_bytecode = True
    saved_path, saved_mods = list(sys.path), dict(sys.modules)
    try:
        for k in [k for k in sys.modules if k.split(".")[0] in ("nerf", "legacy", "raymarching", "gridencoder", "ffmlp", "encoding", "activation",
                                                              "tinycudann")]:
            del sys.modules[k]
        sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
        utils = types.ModuleType("legacy.nerf.utils")              # the one helper legacy/nerf/renderer.py takes from the training harness
        utils.custom_meshgrid = lambda *args: torch.meshgrid(*args, indexing="ij")
        sys.modules["legacy.nerf.utils"] = utils
        sys.path.insert(0, REF)
        sys.path.insert(0, os.path.join(REPO, "focnerf_amd", "dropin"))
        cls = __import__("legacy.nerf.network_tcnn", fromlist=["NeRFNetwork"]).NeRFNetwork
        return cls(encoding="hashgrid", bound=bound, num_layers=num_layers, num_layers_color=num_layers_color, cuda_ray=True, density_scale=1)
    finally:
        sys.path[:] = saved_path
        for k in list(sys.modules):
            if k not in saved_mods:
                del sys.modules[k]


def _dropin_legacy(bound, num_layers, num_layers_color):
    """The legacy network's modules (legacy/nerf/network_tcnn.py:30-79) from the drop-in, on this package's renderer."""
    from focnerf_amd import tcnn
    from focnerf_amd.renderer import NeRFRenderer

    class Model(NeRFRenderer):
        def __init__(self):
            super().__init__(bound, cuda_ray=True, density_scale=1)
            self.encoder = tcnn.Encoding(3, dict(HASH, per_level_scale=np.exp2(np.log2(2048 * bound / 16) / (16 - 1))))
            self.sigma_net = tcnn.Network(32, 16, _mlp(num_layers - 1))
            self.encoder_dir = tcnn.Encoding(3, {"otype": "SphericalHarmonics", "degree": 4})
            self.color_net = tcnn.Network(31, 3, _mlp(num_layers_color - 1))

    return Model()


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(torch.rand(p.shape, generator=g) * 2 - 1)


def _check_round_trip(other, bound, layers, tmp_path):
    from focnerf_amd.checkpoint import load_checkpoint, save_checkpoint
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    make = lambda: NeRFNetwork(bound=bound, num_layers=layers[0], num_layers_color=layers[1], cuda_ray=True, density_scale=1)
    fresh = make()
    sd_new, sd_old = fresh.state_dict(), other.state_dict()
    assert list(sd_new) == list(sd_old)
    assert all(sd_new[k].shape == sd_old[k].shape and sd_new[k].dtype == sd_old[k].dtype for k in sd_old)
    for k in sd_old:                                  # the drop-in's seeded initialisation
        if k.endswith(".params"):
            assert torch.equal(sd_new[k], sd_old[k]), k
    # drop-in -> fused class
    _randomise(other, 1)
    model = make()
    model.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    assert torch.equal(model.encoder.embeddings.detach().reshape(-1), other.encoder.params.detach())
    assert torch.equal(model.sigma_net.weights.detach(), other.sigma_net.params.detach())
    assert torch.equal(model.color_net.weights.detach(), other.color_net.params.detach())
    # fused class -> drop-in
    _randomise(model, 2)
    other.load_state_dict(model.state_dict(), strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    # a checkpoint file written from the drop-in model
    path = str(tmp_path / f"legacy_{bound}_{layers[0]}{layers[1]}.pth")
    save_checkpoint(other, path)
    loaded = make()
    missing, unexpected = load_checkpoint(loaded, path)
    assert missing == [] and unexpected == []
    for k, v in other.state_dict().items():
        assert torch.equal(loaded.state_dict()[k], v), k
    # the reference's four optimizer groups, every parameter in one
    groups = loaded.get_params(1e-2)
    assert len(groups) == 4
    assert sum(len(list(g["params"])) for g in groups) == len(list(loaded.parameters()))


@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("layers", LAYERS)
def test_reference_network_checkpoints_round_trip(bound, layers, tmp_path):
    if not os.path.isdir(os.path.join(REF, "legacy", "nerf")):
        pytest.skip("reference tree not present")
    _check_round_trip(_reference_legacy(bound, *layers), bound, layers, tmp_path)


@pytest.mark.parametrize("bound", [1, 2])
@pytest.mark.parametrize("layers", LAYERS)
def test_dropin_modules_checkpoints_round_trip(bound, layers, tmp_path):
    _check_round_trip(_dropin_legacy(bound, *layers), bound, layers, tmp_path)


def test_topology_parameter_counts_and_keys():
    from focnerf_amd import tcnn
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    m = NeRFNetwork(bound=2, cuda_ray=True, density_scale=1)
    assert (m.sigma_net.input_dim, m.sigma_net.hidden_dim, m.sigma_net.num_layers, m.sigma_net.output_dim) == (32, 64, 1, 16)
    assert (m.color_net.input_dim, m.color_net.hidden_dim, m.color_net.num_layers, m.color_net.output_dim) == (32, 64, 2, 3)
    assert m.in_dim_color == 31 and m.colour_input_pad == tcnn.PAD_VALUE == 1.0
    assert not getattr(m, "uses_object_feature", False)
    assert float(m.encoder.per_level_scale) == float(np.exp2(np.log2(2048 * 2 / 16) / 15))
    sd = m.state_dict()
    assert sd["sigma_net.params"].numel() == 3072 == _mlp_params(32, 64, 1)
    assert sd["color_net.params"].numel() == 7168 == _mlp_params(31, 64, 2)
    assert sd["encoder_dir.params"].numel() == 0
    assert {k for k in sd if k.endswith("params")} == {"encoder.params", "sigma_net.params", "encoder_dir.params", "color_net.params"}
    assert {k for k in sd if not k.endswith("params")} == {"aabb_train", "aabb_infer", "density_grid", "density_bitfield", "step_counter"}
    assert set(NeRFNetwork(bound=1).state_dict()) == {"encoder.params", "sigma_net.params", "encoder_dir.params", "color_net.params",
                                                       "aabb_train", "aabb_infer"}
    assert NeRFNetwork(num_layers=3).sigma_net.num_layers == 2 and NeRFNetwork(num_layers_color=2).color_net.num_layers == 1
    # the keywords main_nerf.py passes
    m = NeRFNetwork(encoding="hashgrid", bound=1, cuda_ray=True, density_scale=1, min_near=0.2, density_thresh=10, bg_radius=-1)
    assert (m.min_near, m.density_thresh, m.bg_radius) == (0.2, 10, -1)
    # a checkpoint of another size is refused by strict loading
    sd = m.state_dict()
    sd["color_net.params"] = sd["color_net.params"][:-1]
    with pytest.raises(RuntimeError, match="color_net"):
        NeRFNetwork(bound=1, cuda_ray=True, density_scale=1).load_state_dict(sd)


def test_background_model_is_refused():
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    with pytest.raises(ValueError, match="bg_radius"):
        NeRFNetwork(bound=1, bg_radius=0.5)


def _off(plan):
    return {v for v in VERDICTS if not getattr(plan, v)}


def test_field_plan_rows(monkeypatch):
    from focnerf_amd import _lib
    from focnerf_amd.field import field_plan
    from focnerf_amd.network import NeRFNetwork as Plain
    from focnerf_amd.network_foc import NeRFNetwork as Foc
    from focnerf_amd.network_tcnn import NeRFNetwork as FocTcnn
    from focnerf_amd.network_tcnn_legacy import NeRFNetwork
    for k in ("FOC_FUSED_FIELD", "FOC_FUSED_TAIL", "FOC_FUSED_INFER", "FOC_FUSED_HEAD", "FOC_FUSED_OCC", "FOC_RENDER_NATIVE"):
        monkeypatch.delenv(k, raising=False)
    assert _lib.get_option("FOC_FIELD_FWD_FUSED") != 0 and _lib.get_option("FOC_MLP_BWD_FUSED") != 0
    for layers in ((2, 3), (2, 4), (3, 3), (3, 4), (4, 4)):
        p = field_plan(NeRFNetwork(num_layers=layers[0], num_layers_color=layers[1], cuda_ray=True, density_scale=1))
        assert (p.sigma.num_layers, p.colour.num_layers) == (layers[0] - 1, layers[1] - 1)
        assert _off(p) == {"head"}, layers                 # sample_head writes a 0 in column 31
        assert p.colour_input_pad == 1.0 and not p.uses_object_feature and p.colour.input_dim == 32
    m = NeRFNetwork(cuda_ray=True, density_scale=1)
    # each switch turns off its own verdict and those built on it
    for switch, off in (("FOC_FUSED_FIELD", {"field", "train_forward", "infer", "occ", "native_loop"}),
                        ("FOC_FUSED_TAIL", {"tail", "train_forward", "occ"}), ("FOC_FUSED_INFER", {"infer", "native_loop"}),
                        ("FOC_FUSED_OCC", {"occ"}), ("FOC_RENDER_NATIVE", {"native_loop"}), ("FOC_FUSED_HEAD", set())):
        monkeypatch.setenv(switch, "0")
        assert _off(field_plan(m)) == off | {"head"}, switch
        monkeypatch.delenv(switch)
    _lib.set_option("FOC_FIELD_FWD_FUSED", 0)
    try:
        assert _off(field_plan(m)) == {"train_forward", "head"}
    finally:
        _lib.set_option("FOC_FIELD_FWD_FUSED", 1)
    assert _off(field_plan(NeRFNetwork(cuda_ray=True, density_scale=2))) == {"native_loop", "head"}
    # the rows of the other networks keep their verdicts and pads
    pp, pf, pt = field_plan(Plain(cuda_ray=True)), field_plan(Foc(cuda_ray=True, density_scale=1)), field_plan(FocTcnn(cuda_ray=True, density_scale=1))
    assert _off(pp) == set() and pp.colour_input_pad == 0
    assert _off(pf) == {"occ", "native_loop"} and pf.colour_input_pad == 0
    assert _off(pt) == {"occ", "native_loop", "head"} and pt.colour_input_pad == 1.0


NEW = {"foc_color_head_forward_pad31": "foc_color_head_forward", "foc_color_head_backward_pad31": "foc_color_head_backward",
       "foc_field_forward_train_pad31": "foc_field_forward_train", "foc_nerf_field_inference_pad31": "foc_nerf_field_inference",
       "foc_occ_render_step_pad31": "foc_occ_render_step", "foc_occ_train_forward_pad31": "foc_occ_train_forward",
       "foc_occ_train_backward_pad31": "foc_occ_train_backward"}


def test_pad31_entry_points_in_header_signatures_and_library():
    from focnerf_amd import _lib
    from test_abi import _declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    declared = _declared()
    for name, old in NEW.items():
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        old_res, old_args = _lib.SIGNATURES[old]
        assert res == old_res and args == old_args[:-1] + [ctypes.c_float, old_args[-1]], name      # the old signature, a float before the stream
    assert len(_lib.SIGNATURES["foc_occ_render_step"][1]) == 43 and len(_lib.SIGNATURES["foc_occ_train_forward"][1]) == 2
    assert _lib.lib.foc_abi_version() == 2


def _refused(rc, what):
    from focnerf_amd import _lib
    msg = _lib.lib.foc_last_error()
    assert rc == 1 and what in msg, (rc, msg)


def test_pad31_entry_points_validate_on_the_host():
    """No launch: an object feature (the 48-wide row) is refused by every *_pad31 twin, whatever the pad; a pad on a layer pair that is not
    built is refused; the *_pad entry points keep refusing a pad without an object feature."""
    from focnerf_amd import _lib
    from focnerf_amd._lib import FocOccTrainNode
    lib = _lib.lib
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    for pad in (1.0, 0.0):
        _refused(lib.foc_field_forward_train_pad31(one, one, 1, one, 1, one, 2, 64, 0, 128, one, one, 4, one, pad, None), b"obj_feat must be NULL")
        _refused(lib.foc_color_head_forward_pad31(one, one, 1, one, 128, 64, 2, 0, one, 16, one, pad, None), b"obj_feat must be NULL")
        _refused(lib.foc_color_head_backward_pad31(one, one, one, 1, None, one, 128, 64, 2, 0, one, one, one, 1 << 30, 16, one, None, pad, None),
                 b"obj_feat must be NULL")
        _refused(lib.foc_nerf_field_inference_pad31(one, 1, one, 1, 0, 1, one, 1, one, 2, 64, 0, 128, one, one, one, pad, None), b"obj_feat must be NULL")
    _refused(lib.foc_field_forward_train_pad31(one, one, 1, one, 1, one, 4, 64, 0, 128, one, one, 4, None, 1.0, None), b"(1, 4) are not built")
    _refused(lib.foc_nerf_field_inference_pad31(one, 1, one, 1, 0, 1, one, 3, one, 2, 64, 0, 128, one, one, None, 1.0, None), b"(3, 2) are not built")
    _refused(lib.foc_nerf_field_inference_pad31(one, 0, one, 1, 0, 1, one, 1, one, 2, 64, 0, 128, one, one, None, 1.0, None), b"planar")
    _refused(lib.foc_color_head_forward_pad31(one, one, 1, one, 128, 64, 1, 0, one, 16, None, 1.0, None), b"num_layers")
    _refused(lib.foc_color_head_backward_pad31(one, one, one, 1, None, one, 128, 64, 4, 0, one, one, one, 1 << 30, 16, None, None, 1.0, None),
             b"num_layers 2 or 3")
    # the render step: both refusals before anything is enqueued
    step = lambda sl, cl, obj, pad: lib.foc_occ_render_step_pad31(64, 1, one, one, one, one, one, one, 1.0, 0.0, 1024, 1, 128, one, one, one, one, one, one,
                                                                  one, one, one, one, one, 16, 0.5, 16, one, sl, one, cl, 0, obj, 1e-4, one, one, one, one,
                                                                  0, one, 0, 1, pad, None)
    _refused(step(1, 2, one, 1.0), b"obj_feat must be NULL")
    _refused(step(3, 2, None, 1.0), b"(got 3, 2)")
    # the node: a pad on a layer pair that is not built, before anything is enqueued
    nd = FocOccTrainNode()
    nd.struct_bytes = ctypes.sizeof(FocOccTrainNode)
    nd.cap, nd.n_rays, nd.grid_workspace, nd.grid_workspace_bytes, nd.offsets_host = 128, 4, 8, 1 << 20, 8
    nd.sigma_layers, nd.color_layers = 3, 2
    _refused(lib.foc_occ_train_forward_pad31(ctypes.byref(nd), 1.0, None), b"occ_train_forward_pad31: a pad needs")
    _refused(lib.foc_occ_train_backward_pad31(ctypes.byref(nd), 1.0, None), b"occ_train_backward_pad31: a pad needs")
    # the 48-wide twins are unchanged: a pad without an object feature is still refused
    _refused(lib.foc_color_head_forward_pad(one, one, 1, one, 128, 64, 2, 0, one, 16, None, 1.0, None), b"needs obj_feat")
    _refused(lib.foc_field_forward_train_pad(one, one, 1, one, 1, one, 2, 64, 0, 128, one, one, 4, None, 1.0, None), b"needs obj_feat")
