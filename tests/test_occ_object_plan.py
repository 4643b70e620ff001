"""CPU: the object-conditioned networks on the occupancy-grid path — what can be checked without a device.

  * `field.field_plan`'s two verdicts for it (`occ_object`, `native_loop_object`) across networks, switches, layer pairs and a background
    radius, with `occ` / `native_loop` as they were;
  * every refusal of foc_occ_train_forward_obj / _backward_obj, foc_occ_render_step_pad and the *_sumsq tails: non-zero, a message that
    names the entry point, nothing enqueued (there is no device to enqueue on);
  * a mask that is not per ray raises before anything is launched.
"""
import ctypes
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REPO, "focnerf_amd", "libfocnerf_hip.so")), reason="libfocnerf_hip.so not built")


def _net(kind, **kw):
    from focnerf_amd import network, network_foc, network_tcnn
    cls = {"ff": network.NeRFNetwork, "foc": network_foc.NeRFNetwork, "tcnn": network_tcnn.NeRFNetwork}[kind]
    if kind == "tcnn":                                       # its constructor draws tinycudann's seeded initialisation: a real (CPU) module
        return cls(bound=1, cuda_ray=True, **kw)
    with torch.device("meta"):
        return cls(bound=1, cuda_ray=True, **kw)


def _plan(m):
    from focnerf_amd.field import field_plan
    return field_plan(m)


# ---------------------------------------------------------------- the plan
@pytest.mark.parametrize("kind", ["foc", "tcnn"])
def test_default_object_networks_take_the_object_node_and_loop(kind, monkeypatch):
    for switch in ("FOC_FUSED_OCC", "FOC_RENDER_NATIVE"):
        monkeypatch.delenv(switch, raising=False)
    m = _net(kind)
    p = _plan(m)
    assert p.uses_object_feature and p.occ_object is True and p.native_loop_object is True
    assert not p.occ and not p.native_loop                   # pinned by tests/test_field_plan.py and test_network_tcnn_layout.py: unchanged
    assert p.colour_input_pad == (1.0 if kind == "tcnn" else 0.0)

    monkeypatch.setenv("FOC_FUSED_OCC", "0")
    p = _plan(m)
    assert not p.occ_object and p.native_loop_object
    monkeypatch.delenv("FOC_FUSED_OCC")
    monkeypatch.setenv("FOC_RENDER_NATIVE", "0")
    p = _plan(m)
    assert p.occ_object and not p.native_loop_object
    monkeypatch.delenv("FOC_RENDER_NATIVE")

    m.bg_radius = 1
    p = _plan(m)
    assert not p.occ_object and not p.native_loop_object and not p.occ and not p.native_loop


def test_plain_network_keeps_its_verdicts(monkeypatch):
    for switch in ("FOC_FUSED_OCC", "FOC_RENDER_NATIVE"):
        monkeypatch.delenv(switch, raising=False)
    p = _plan(_net("ff"))
    assert p.occ and p.native_loop and not p.uses_object_feature
    assert p.occ_object is False and p.native_loop_object is False


def test_layer_pairs_of_the_object_node(monkeypatch):
    """The whole-field pairs (1,2), (1,3), (2,2), (2,3), (3,3) — (sigma, colour) layers of the two FFMLPs — and nothing else."""
    for switch in ("FOC_FUSED_OCC", "FOC_RENDER_NATIVE"):
        monkeypatch.delenv(switch, raising=False)
    for sigma_layers, colour_layers, want in ((2, 2, True), (2, 3, True), (3, 3, True), (3, 2, False), (4, 3, False), (2, 4, False)):
        p = _plan(_net("foc", num_layers=sigma_layers, num_layers_color=colour_layers + 1))
        assert (p.sigma.num_layers, p.colour.num_layers) == (sigma_layers, colour_layers)
        assert bool(p.occ_object) is want and bool(p.native_loop_object) is want, (sigma_layers, colour_layers)
    p = _plan(_net("tcnn", num_layers=2, num_layers_color=3))                       # tinycudann counts hidden layers: (1, 2)
    assert (p.sigma.num_layers, p.colour.num_layers) == (1, 2) and p.occ_object and p.native_loop_object


# ---------------------------------------------------------------- refusals
ONE = ctypes.c_void_p(8)        # never dereferenced: every call below is refused first


def _node(sigma_layers=2, color_layers=2):
    from focnerf_amd import _lib
    nd = _lib.FocOccTrainNode()
    nd.struct_bytes = ctypes.sizeof(_lib.FocOccTrainNode)
    nd.cap, nd.n_rays = 128, 4
    nd.grid_workspace, nd.grid_workspace_bytes, nd.offsets_host = 8, 1 << 20, 8
    nd.sigma_input_dim, nd.sigma_hidden, nd.sigma_layers, nd.sigma_activation, nd.sigma_output_activation = 32, 64, sigma_layers, 0, 6
    nd.color_hidden, nd.color_layers, nd.color_activation, nd.c_width = 64, color_layers, 0, 4
    return nd


def _object(pad=0.0, feat=8):
    from focnerf_amd import _lib
    ob = _lib.FocOccTrainObject()
    ob.struct_bytes, ob.input_pad, ob.obj_feat = ctypes.sizeof(_lib.FocOccTrainObject), pad, feat
    return ob


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_object_node_refusals_need_no_gpu(which):
    from focnerf_amd import _lib
    lib = _lib.lib
    fn = getattr(lib, f"foc_occ_train_{which}_obj")
    who = f"occ_train_{which}_obj".encode()

    def refused(nd, ob, *words):
        rc = fn(ctypes.byref(nd) if nd is not None else None, ctypes.byref(ob) if ob is not None else None, None)
        msg = lib.foc_last_error()
        assert rc != 0 and who in msg and all(w in msg for w in words), (rc, msg)

    refused(None, _object(), b"null node")
    refused(_node(), None, b"null object")
    ob = _object()
    ob.struct_bytes -= 8
    refused(_node(), ob, b"FocOccTrainObject", b"bytes")
    nd = _node()
    nd.struct_bytes -= 8
    refused(nd, _object(), b"FocOccTrainNode", b"bytes")
    refused(_node(), _object(feat=None), b"obj_feat is NULL")
    refused(_node(), _object(pad=1.0, feat=None), b"a pad", b"needs an object feature")
    for pair in ((3, 2), (4, 3), (2, 4), (1, 1)):
        refused(_node(*pair), _object(pad=1.0), b"(1,2), (1,3), (2,2), (2,3), (3,3)", b"got %d, %d" % pair)
        refused(_node(*pair), _object(pad=0.0), b"(1,2), (1,3), (2,2), (2,3), (3,3)")
    if which == "backward":
        nd = _node()
        nd.mlp_workspace, nd.mlp_workspace_bytes = 8, int(lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2))      # sized for the 32-wide head
        refused(nd, _object(), b"workspace of", b"48")


def test_render_step_pad_and_sumsq_tail_refusals_need_no_gpu():
    from focnerf_amd import _lib
    lib = _lib.lib

    def step(sigma_layers, color_layers, obj, pad):
        return lib.foc_occ_render_step_pad(64, 1, ONE, ONE, ONE, ONE, ONE, ONE, 1.0, 0.0, 1024, 1, 128, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, 16,
                                           0.5, 16, ONE, sigma_layers, ONE, color_layers, 0, obj, 1e-4, ONE, ONE, ONE, ONE, 0, None, 0, 0, pad, None)
    assert step(2, 2, None, 1.0) != 0 and b"occ_render_step_pad: input_pad is column 47" in lib.foc_last_error()
    assert step(3, 2, ONE, 1.0) != 0 and b"occ_render_step_pad: a pad needs" in lib.foc_last_error() and b"got 3, 2" in lib.foc_last_error()
    rc = lib.foc_occ_tail_forward_sumsq(ONE, ONE, 4, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, ONE, ONE, ONE, ONE, None, None)
    assert rc != 0 and b"occ_tail_forward_sumsq: null ray_sumsq" in lib.foc_last_error()
    rc = lib.foc_occ_tail_backward_sumsq(ONE, None, ONE, ONE, 4, ONE, ONE, ONE, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, None, None)
    assert rc != 0 and b"occ_tail_backward_sumsq: null grad_sumsq" in lib.foc_last_error()
    rc = lib.foc_occ_tail_forward_sumsq(ONE, ONE, 8, ONE, ONE, 128, 4, 1e-4, 1.0, None, 1.0, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None)
    assert rc != 0 and b"occ_tail_forward_sumsq: c_width" in lib.foc_last_error()


# ---------------------------------------------------------------- the mask
def test_ray_mask_shapes():
    from focnerf_amd.occtrain import ray_mask
    want = torch.tensor([True, False, True, True, False])
    for shape in ((5,), (1, 5), (1, 5, 1)):
        assert torch.equal(ray_mask(want.view(shape), 5), want)
    for bad in (torch.ones(1, 5, 8, dtype=torch.bool), torch.ones(4, dtype=torch.bool), torch.ones(1, 6, dtype=torch.bool)):
        with pytest.raises(ValueError, match="one entry per ray"):
            ray_mask(bad, 5)


@pytest.mark.parametrize("kind", ["foc", "tcnn"])
def test_a_mask_of_the_wrong_size_raises_before_any_launch(kind, monkeypatch):
    from focnerf_amd import _lib, network_foc, network_tcnn
    cls = {"foc": network_foc.NeRFNetwork, "tcnn": network_tcnn.NeRFNetwork}[kind]
    m = cls(bound=1, cuda_ray=True).train()
    launched = []
    for name, (_, args) in _lib.SIGNATURES.items():
        if args and args[-1] is _lib.c_vp and not name.endswith(("_bytes", "_option")):          # every entry point that takes a stream
            monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: launched.append(_n) or 1)
    monkeypatch.setattr(m, "encode_object_feature", lambda *a: launched.append("encode_object_feature"))
    n = 64
    o, d = torch.zeros(1, n, 3), torch.nn.functional.normalize(torch.ones(1, n, 3), dim=-1)
    for mask in (torch.ones(1, n, 512, dtype=torch.bool), torch.ones(1, n - 1, dtype=torch.bool)):
        with pytest.raises(ValueError, match="one entry per ray"):
            m.render(o, d, (mask, None, torch.zeros(144)), staged=False, dt_gamma=1 / 128, max_steps=64)
    assert launched == []
