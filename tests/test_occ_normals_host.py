"""CPU: what foc_occ_render_step_normals and foc_normal_map_finish refuse on the host (FOC_E_INVALID, the message names the argument, nothing
is enqueued: there is no device here), and the ValueErrors of run_cuda(normals=...) / render_normals(path="occupancy") that fire before any
device work. Pattern: tests/test_optim_host.py."""
import ctypes

import pytest
import torch

ONLY, AUX = 1, 2                  # FOC_OCC_NORMALS_ONLY, FOC_OCC_NORMALS_AUX (include/focnerf.h)
ONE = 64                          # an aligned non-null address; never dereferenced: every call below is refused on the host

# the arguments of foc_occ_render_step_normals by name, in the header's order, of a call that passes every host check
_VALID = dict(n_alive=130, n_step=8, rays_alive=ONE, rays_alive_out=ONE, count=ONE, rays_t=ONE, rays_o=ONE, rays_d=ONE, bound=1.0, dt_gamma=0.0,
              max_steps=256, C=1, H=128, grid=ONE, nears=ONE, fars=ONE, noises=ONE, samples=ONE, planes=ONE, sigma=ONE, rgb=ONE, embeddings=ONE,
              offsets=ONE, offsets_host=None, L=16, S=0.5, base_res=16, sigma_weights=ONE, sigma_layers=2, color_weights=ONE, color_layers=3,
              activation=0, obj_feat=None, T_thresh=1e-4, weights_sum=ONE, depth=ONE, image=ONE, scratch=ONE, flags=0, deaths=None, deaths_base=0,
              deaths_len=1, input_pad=0.0, pad_column=0, mode=ONLY, normal_rgb=ONE, normal_acc=ONE, stream=None)
_COLOUR_ONLY = ("planes", "rgb", "color_weights", "image")


def _refused(word, **change):
    from focnerf_amd import _lib
    assert not set(change) - set(_VALID)
    rc = _lib.lib.foc_occ_render_step_normals(*{**_VALID, **change}.values())
    msg = _lib.lib.foc_last_error()
    assert rc == 1 and word in msg, (change, rc, msg)
    return msg


def test_the_entry_points_exist_and_the_abi_version_stays():
    from focnerf_amd import _lib
    assert _lib.lib.foc_abi_version() == 2
    assert len(_lib.SIGNATURES["foc_occ_render_step_normals"][1]) == len(_VALID) == len(_lib.SIGNATURES["foc_occ_render_step"][1]) + 5
    assert _lib.SIGNATURES["foc_occ_render_step_normals"][1][-6:-1] == [ctypes.c_float, ctypes.c_uint32, ctypes.c_uint32, _lib.c_vp, _lib.c_vp]
    assert len(_lib.SIGNATURES["foc_normal_map_finish"][1]) == 6
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "foc_occ_render_step_normals") and not hasattr(raw, "composite_compact_aux")          # the second launcher stays inside


def test_mode_and_pad_column_are_refused_by_name():
    for mode in (0, 3, 7):
        _refused(b"mode", mode=mode)
    for col in (1, 32, 48):
        _refused(b"pad_column", pad_column=col)
    _refused(b"input_pad must be 0", pad_column=0, input_pad=1.0)
    _refused(b"obj_feat must be NULL", pad_column=31, input_pad=1.0, obj_feat=ONE)
    _refused(b"obj_feat must be NULL", pad_column=31, input_pad=0.0, obj_feat=ONE)
    _refused(b"needs obj_feat", pad_column=47, input_pad=1.0)
    _refused(b"needs obj_feat", pad_column=47, input_pad=0.0)
    for col, obj in ((31, None), (47, ONE)):
        for pair in ((3, 2), (2, 1), (1, 1)):
            msg = _refused(b"(sigma_layers, color_layers)", pad_column=col, input_pad=1.0, obj_feat=obj, sigma_layers=pair[0], color_layers=pair[1])
            assert b"got %d, %d" % pair in msg


@pytest.mark.parametrize("mode", [ONLY, AUX])
def test_null_pointers_are_refused_by_mode(mode):
    for name in ("normal_rgb", "normal_acc"):
        _refused(b"normal_rgb, normal_acc", mode=mode, **{name: None})
    _refused(b"null pointer", mode=mode, count=None)
    for name in ("rays_alive", "rays_alive_out", "rays_t", "rays_o", "rays_d", "grid", "fars", "noises", "samples", "sigma", "embeddings", "offsets",
                 "sigma_weights", "weights_sum", "depth", "scratch"):
        _refused(b"null pointer", mode=mode, **{name: None})
    for name in _COLOUR_ONLY:
        if mode == AUX:
            _refused(b"planes, rgb, color_weights, image", mode=mode, **{name: None})
        else:                                                    # not needed: the call gets as far as the NEXT refusal (there is no device to go on to)
            _refused(b"L must be 16", mode=mode, L=8, **{name: None})
    _refused(b"L must be 16", mode=ONLY, L=8, obj_feat=None, **{name: None for name in _COLOUR_ONLY})


@pytest.mark.parametrize("mode", [ONLY, AUX])
def test_what_the_normals_kernel_refuses_is_refused_before_the_first_launch(mode):
    _refused(b"n_step must be in [1, 16]", mode=mode, n_step=17)
    _refused(b"n_step must be in [1, 16]", mode=mode, n_step=0)
    for L in (8, 15, 17):
        _refused(b"foc_field_normals: L must be 16", mode=mode, L=L)
    for layers in (0, 4):
        _refused(b"foc_field_normals: sigma_layers", mode=mode, sigma_layers=layers)
    _refused(b"foc_field_normals: activation", mode=mode, activation=1)
    _refused(b"foc_field_normals: H must be", mode=mode, base_res=0)
    _refused(b"16-byte aligned", mode=mode, sigma_weights=ONE + 8)
    _refused(b"4-byte", mode=mode, embeddings=ONE + 2)


def test_normal_map_finish_refusals():
    from focnerf_amd import _lib
    fin = _lib.lib.foc_normal_map_finish
    assert fin(None, None, 0, None, None, None) == 0                    # nothing to do
    for hole in range(4):
        args = [ONE, ONE, ONE, ONE]
        args[hole] = None
        assert fin(args[0], args[1], 5, args[2], args[3], None) == 1 and b"foc_normal_map_finish: null pointer" in _lib.lib.foc_last_error()


# ---------------------------------------------------------------- Python: never a silent fallback
def _cpu_model():
    from focnerf_amd.network import NeRFNetwork
    torch.manual_seed(0)
    return NeRFNetwork(bound=1, cuda_ray=True)


def test_run_cuda_normals_raises_by_condition(monkeypatch):
    m = _cpu_model()
    o, d = torch.zeros(1, 4, 3), torch.ones(1, 4, 3)
    with torch.no_grad():
        with pytest.raises(ValueError, match="must be False, True or 'only'"):
            m.run_cuda(o, d, normals="both")
    m.train()
    for mode in (True, "only"):
        with pytest.raises(ValueError, match="training mode"):
            m.run_cuda(o, d, normals=mode)
        with pytest.raises(ValueError, match="training mode"):
            m.render(o, d, normals=mode)                                # through render()'s kwargs
    m.eval()
    with pytest.raises(ValueError, match="gradients are enabled"):
        m.run_cuda(o, d, normals=True)
    with torch.no_grad():
        assert not torch.is_autocast_enabled()
        with pytest.raises(ValueError, match="autocast is off"):
            m.run_cuda(o, d, normals="only")
        monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: True)      # (no device here: torch would not enable it)
        with pytest.raises(ValueError, match="device_compaction=False"):
            m.run_cuda(o, d, normals="only", device_compaction=False)
        from focnerf_amd.field import field_plan
        assert field_plan(m).normals and field_plan(m).native_loop
        monkeypatch.setenv("FOC_FUSED_NORMALS", "0")
        with pytest.raises(ValueError, match=r"field_plan\(model\)\.normals is false"):
            m.run_cuda(o, d, normals=True)
        monkeypatch.delenv("FOC_FUSED_NORMALS")
        monkeypatch.setenv("FOC_RENDER_NATIVE", "0")
        with pytest.raises(ValueError, match=r"field_plan\(model\)\.native_loop is false"):
            m.run_cuda(o, d, normals=True, device_compaction=True)
        monkeypatch.delenv("FOC_RENDER_NATIVE")
        m.density_scale = 2
        with pytest.raises(ValueError, match=r"native_loop is false"):
            m.run_cuda(o, d, normals="only")
        m.density_scale = 1
        with pytest.raises(ValueError, match="not on a GPU"):
            m.run_cuda(o, d, normals="only")


def test_render_normals_occupancy_path_refusals():
    import focnerf_amd
    from focnerf_amd.network import NeRFNetwork
    assert "normal_map_finish" in focnerf_amd.__all__ and focnerf_amd.normal_map_finish is focnerf_amd.normals.normal_map_finish
    m = _cpu_model().eval()
    o, d = torch.zeros(4, 3), torch.ones(4, 3)
    with pytest.raises(ValueError, match="path must be"):
        focnerf_amd.render_normals(m, o, d, path="marching")
    with pytest.raises(ValueError, match="occupancy= / placement="):
        focnerf_amd.render_normals(m, o, d, path="occupancy", occupancy=object())
    with pytest.raises(ValueError, match="occupancy= / placement="):
        focnerf_amd.render_normals(m, o, d, path="occupancy", placement=object())
    with pytest.raises(ValueError, match="cuda_ray=True"):
        focnerf_amd.render_normals(NeRFNetwork(bound=1, cuda_ray=False).eval(), o, d, path="occupancy")
    with pytest.raises(ValueError):                                     # no device: run_cuda's own refusal, not a fallback to the fixed steps
        focnerf_amd.render_normals(m, o, d, path="occupancy")
    with pytest.raises(ValueError, match="fp32 GPU tensors"):
        focnerf_amd.normal_map_finish(torch.zeros(4, 3), torch.zeros(4))
