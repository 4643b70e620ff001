"""CPU: what the surface-normal feature decides on the host — foc_field_normals' refusals (before any launch, no GPU needed),
`FieldPlan.normals` for every network class and under FOC_FUSED_NORMALS=0, and the ValueErrors of channels="normal" and of
extract_scene_geometry(normals="field")."""
import ctypes
import importlib
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(HERE), "focnerf_amd", "libfocnerf_hip.so")),
                                reason="libfocnerf_hip.so not built")

ONE = ctypes.c_void_p(16)             # never dereferenced: validation fails first (16-byte aligned, so alignment is not what refuses)
GOOD = dict(D=3, C=2, L=16, gridtype=0, align_corners=0, interp=0, dtype=1, sigma_layers=2, hidden_dim=64, activation=0)


def _call(xn=ONE, emb=ONE, offsets=ONE, weights=ONE, out=ONE, M=4, **over):
    from focnerf_amd import _lib
    a = dict(GOOD, **over)
    rc = _lib.lib.foc_field_normals(xn, M, emb, offsets, a["D"], a["C"], a["L"], 1.0, 16, a["gridtype"], a["align_corners"], a["interp"], a["dtype"], None, weights,
                                    a["sigma_layers"], a["hidden_dim"], a["activation"], None, out, None, None, None, None)
    return rc, _lib.lib.foc_last_error().decode()


@pytest.mark.parametrize("over, code, word", [
    (dict(L=15), 1, "L must be 16"), (dict(L=17), 1, "L must be 16"), (dict(C=4), 1, "C must be 2"), (dict(C=1), 1, "C must be 2"),
    (dict(D=2), 1, "D must be 3"), (dict(D=4), 1, "D must be 3"), (dict(hidden_dim=32), 1, "hidden_dim must be 64"),
    (dict(hidden_dim=128), 1, "hidden_dim must be 64"), (dict(activation=6), 1, "activation must be relu"), (dict(activation=3), 1, "activation must be relu"),
    (dict(sigma_layers=0), 1, "sigma_layers must be 1, 2 or 3"), (dict(sigma_layers=4), 1, "sigma_layers must be 1, 2 or 3"),
    (dict(gridtype=1), 1, "gridtype must be hash"), (dict(align_corners=1), 1, "align_corners must be off"), (dict(interp=1), 1, "interp must be linear"),
    (dict(dtype=0), 2, "dtype must be FOC_F16")])
def test_shapes_outside_the_served_one_are_refused_by_name(over, code, word):
    rc, msg = _call(**over)
    assert rc == code and "foc_field_normals" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("null", ["xn", "emb", "offsets", "weights"])
def test_null_pointers_are_refused(null):
    rc, msg = _call(**{null: None})
    assert rc == 1 and "null pointer" in msg, (rc, msg)


def test_misaligned_weights_are_refused_and_nothing_to_do_is_ok():
    rc, msg = _call(weights=ctypes.c_void_p(8))
    assert rc == 1 and "aligned" in msg
    assert _call(M=0)[0] == 0                                     # no samples: nothing is launched
    assert _call(out=None)[0] == 0                                # no output asked for: nothing is launched


def test_abi_version_is_unchanged_and_the_entry_is_bound():
    from focnerf_amd import _lib
    assert _lib.lib.foc_abi_version() == 2 and "foc_field_normals" in _lib.SIGNATURES and len(_lib.SIGNATURES["foc_field_normals"][1]) == 24


# ---------------------------------------------------------------- the plan
NETWORKS = ["network", "network_foc", "network_tcnn", "network_tcnn_legacy", "network_linear"]


def _meta(mod, **kw):
    with torch.device("meta"):
        return importlib.import_module("focnerf_amd." + mod).NeRFNetwork(**kw)


@pytest.mark.parametrize("mod", NETWORKS)
def test_every_network_class_of_the_package_is_served_and_the_switch_turns_it_off(mod, monkeypatch):
    from focnerf_amd.field import field_plan
    m = _meta(mod)
    assert field_plan(m).normals
    monkeypatch.setenv("FOC_FUSED_NORMALS", "0")
    assert not field_plan(m).normals
    monkeypatch.setenv("FOC_FUSED_NORMALS", "1")
    assert field_plan(m).normals


@pytest.mark.parametrize("change", ["tiled", "align_corners", "smoothstep", "sigmoid", "4 layers", "hidden 32", "level_dim 4", "12 levels", "no grid"])
def test_shape_rules_of_the_verdict(change):
    from focnerf_amd.field import field_plan
    m = _meta("network", num_layers=4) if change == "4 layers" else _meta("network", hidden_dim=32) if change == "hidden 32" else _meta("network")
    e = m.encoder
    if change == "tiled":
        e.gridtype, e.gridtype_id = "tiled", 1
    elif change == "align_corners":
        e.align_corners = True
    elif change == "smoothstep":
        e.interpolation, e.interp_id = "smoothstep", 1
    elif change == "sigmoid":
        m.sigma_net.activation = 3
    elif change == "level_dim 4":
        e.level_dim = 4
    elif change == "12 levels":
        e.offsets = e.offsets[:13]
    elif change == "no grid":
        m.encoder = torch.nn.Identity()
    assert not field_plan(m).normals


# ---------------------------------------------------------------- refusals of the Python layer
def test_channels_normal_refusals(monkeypatch):
    from focnerf_amd import normals
    from focnerf_amd.field import field_plan
    from focnerf_amd.fixedstep import render_field4
    m = _meta("network")
    rays = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="channels must be 'rgb' or 'normal'"):
        render_field4(m, rays, rays, num_steps=8, channels="depth")
    with pytest.raises(ValueError, match="channels must be"):
        normals.check_channels("x", "normals")
    assert normals.check_channels("x", "rgb", field_plan(m)) is False and normals.check_channels("x", "normal", field_plan(m)) is True
    monkeypatch.setenv("FOC_FUSED_NORMALS", "0")
    assert normals.check_channels("x", "rgb", field_plan(m)) is False                       # the colour path never asks for the verdict
    with pytest.raises(ValueError, match="channels='normal' needs a network the fused normals kernel serves"):
        render_field4(m, rays, rays, num_steps=8, channels="normal")
    with pytest.raises(ValueError, match="channels='normal' needs"):
        normals.field_normals(m, rays)
    monkeypatch.setenv("FOC_FUSED_NORMALS", "1")
    smooth = _meta("network")
    smooth.encoder.interpolation, smooth.encoder.interp_id = "smoothstep", 1
    with pytest.raises(ValueError, match="channels='normal' needs"):
        render_field4(smooth, rays, rays, num_steps=8, channels="normal")
    with_bg = _meta("network", bg_radius=2)
    with pytest.raises(ValueError, match="without a background model"):
        render_field4(with_bg, rays, rays, num_steps=8, channels="normal")


def test_scene_refusals():
    from focnerf_amd import mesh
    from focnerf_amd.combine import culled_field_fns, placed_field_fns, render_scene_culled
    m = _meta("network")
    with pytest.raises(ValueError, match="not served for a scene"):
        mesh.extract_scene_geometry([m], [None], [-1, -1, -1, 1, 1, 1], resolution=8, normals="field")
    with pytest.raises(ValueError, match="normals must be False, True or 'field'"):
        mesh.extract_geometry(m, resolution=8, normals="lattice")
    rays = torch.zeros(4, 3)
    for fn in (placed_field_fns, culled_field_fns):
        with pytest.raises(ValueError):
            fn([m], [object()], [None], rays, rays, 8, None, channels="normal")                # the occupancy is checked as before
    with pytest.raises(ValueError):
        render_scene_culled([m], [object()], [None], rays, rays, 8, None, channels="depth")


def test_decode_normal_map_checks_its_input():
    from focnerf_amd.normals import decode_normal_map
    with pytest.raises(ValueError, match=r"\[2,N,4\]"):
        decode_normal_map(torch.zeros(3, 5, 4))
    n, op = decode_normal_map(torch.stack([torch.ones(5, 4), torch.zeros(5, 4)]))             # nothing but background
    assert n.shape == (5, 3) and op.shape == (5,) and (n == 0).all() and (op == 0).all()
