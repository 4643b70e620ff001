"""CPU: the FOC_DETERMINISTIC switch through every host layer (library option table, _lib.get_option / set_option, the package's
use_deterministic / is_deterministic / deterministic) and what the mode does on the host before any launch: larger workspaces and
refusals that name the option. No GPU: the library loads without a device."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPT = "FOC_DETERMINISTIC"


@pytest.fixture(autouse=True)
def _restore():
    from focnerf_amd import _lib
    old = _lib.get_option(OPT)
    yield
    _lib.set_option(OPT, old)


def test_option_exists_and_defaults_to_zero():
    env = {k: v for k, v in os.environ.items() if k != OPT}
    out = subprocess.run([sys.executable, "-c", f"from focnerf_amd import _lib; import focnerf_amd; print(_lib.get_option('{OPT}'), focnerf_amd.is_deterministic())"],
                         cwd=REPO, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["0", "False"]


def test_set_and_get_round_trip():
    from focnerf_amd import _lib
    for v in (1, 0, 2, 0):
        _lib.set_option(OPT, v)
        assert _lib.get_option(OPT) == v


def test_lib_option_fixture_takes_it(lib_option):
    from focnerf_amd import _lib
    lib_option(OPT, 1)
    assert _lib.get_option(OPT) == 1


def test_python_interface_reads_and_writes_the_same_value():
    import focnerf_amd
    from focnerf_amd import _lib
    focnerf_amd.use_deterministic(True)
    assert focnerf_amd.is_deterministic() and _lib.get_option(OPT) == 1
    focnerf_amd.use_deterministic(False)
    assert not focnerf_amd.is_deterministic() and _lib.get_option(OPT) == 0
    _lib.set_option(OPT, 1)
    assert focnerf_amd.is_deterministic()
    _lib.set_option(OPT, 0)
    with focnerf_amd.deterministic():
        assert focnerf_amd.is_deterministic() and _lib.get_option(OPT) == 1
        with focnerf_amd.deterministic(False):
            assert not focnerf_amd.is_deterministic()
        assert focnerf_amd.is_deterministic()
    assert not focnerf_amd.is_deterministic()
    # the value from before comes back, whatever it was, and also when the block raises
    _lib.set_option(OPT, 2)
    with focnerf_amd.deterministic(True):
        assert _lib.get_option(OPT) == 1
    assert _lib.get_option(OPT) == 2
    _lib.set_option(OPT, 0)
    with pytest.raises(ValueError):
        with focnerf_amd.deterministic():
            assert focnerf_amd.is_deterministic()
            raise ValueError("inside")
    assert not focnerf_amd.is_deterministic()


def test_environment_sets_the_initial_value():
    env = dict(os.environ, FOC_DETERMINISTIC="1")
    out = subprocess.run([sys.executable, "-c", f"import focnerf_amd; from focnerf_amd import _lib; print(_lib.get_option('{OPT}'), focnerf_amd.is_deterministic())"],
                         cwd=REPO, env=env, capture_output=True, text=True, check=True).stdout.split()
    assert out == ["1", "True"]


def test_symbols_header_and_signatures_still_agree():
    from focnerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "focnerf.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(foc_[A-Za-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert declared == set(_lib.SIGNATURES)
    for n in declared:
        assert hasattr(lib, n)
    assert _lib.lib.foc_abi_version() == 2


def test_the_header_lists_an_outcome_for_every_atomic_entry_point():
    text = open(os.path.join(REPO, "include", "focnerf.h")).read()
    block = text[text.index("Deterministic mode"):text.index("int foc_guard_pick_device")]
    for name in ("foc_grid_encode_backward_binned", "foc_background_backward", "foc_grid_update_apply", "foc_ffmlp_backward", "foc_grid_encode_backward ",
                 "foc_grad_total_variation", "fp32 tables: REFUSED"):
        assert name in block, name
    assert block.count("DETERMINISTIC FORM") == 4 and block.count("REFUSED") >= 2


def test_workspace_sizes_follow_the_option():
    """Each *_workspace_bytes of a kernel that got a deterministic form answers for the CURRENT value of the option, and the default
    mode's sizes are what they were."""
    from focnerf_amd import _lib
    lib = _lib.lib
    B, L = 1 << 20, 16
    off = dict(grid=lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 1), grid32=lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 0),
               bg=lib.foc_background_backward_workspace_bytes(4096), dg=lib.foc_grid_update_apply_workspace_bytes(1, 128),
               mlp128=lib.foc_ffmlp_backward_workspace_bytes(32, 128, 2), mlp64=lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2))
    assert off["bg"] == 64 * 1728 * 4 and off["dg"] == 128 ** 3 * 4 + 256
    _lib.set_option(OPT, 1)
    slots = L * 64
    image = 8192 * 2 * 8 + 8192 // 8                       # one slot: two int64 planes of 8192 rows and its bad-row bits
    on = dict(grid=lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 1), grid32=lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 0),
              bg=lib.foc_background_backward_workspace_bytes(4096), dg=lib.foc_grid_update_apply_workspace_bytes(1, 128),
              mlp128=lib.foc_ffmlp_backward_workspace_bytes(32, 128, 2), mlp64=lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2))
    assert off["grid"] + slots * image <= on["grid"] <= off["grid"] + slots * image + 256
    assert on["grid32"] == off["grid32"]                   # fp32 tables have no deterministic form: nothing to add
    assert on["bg"] >= off["bg"] + 32 * 4096 * 24          # a row table of at least 32 N entries of 24 bytes
    assert on["dg"] == off["dg"] + 2048 * 8
    assert on["mlp128"] >= 32 * off["mlp128"] and on["mlp64"] == off["mlp64"]
    _lib.set_option(OPT, 2)                                # the per-chunk planes of the measured variant: one image per chunk of the worst case
    chunks = (B * 5 * L + 32767) // 32768 + slots
    two = lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 1)
    assert off["grid"] + chunks * image <= two <= off["grid"] + chunks * image + 256
    _lib.set_option(OPT, 0)
    assert lib.foc_grid_encode_backward_workspace_bytes(B, 3, 2, L, 1) == off["grid"]


def test_short_workspaces_are_refused_under_the_option():
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)                               # never dereferenced: validation fails first
    offs = (ctypes.c_int32 * 3)(0, 4920, 4920 + 35944)
    host = ctypes.cast(offs, ctypes.c_void_p)
    small = lib.foc_grid_encode_backward_workspace_bytes(4096, 3, 2, 2, 1)
    need_bg, need_dg = lib.foc_background_backward_workspace_bytes(4096), lib.foc_grid_update_apply_workspace_bytes(1, 128)
    need_mlp = lib.foc_ffmlp_backward_workspace_bytes(32, 128, 2)
    _lib.set_option(OPT, 1)
    rc = lib.foc_grid_encode_backward_binned(one, one, one, one, one, 4096, 3, 2, 2, 1.0, 16, None, None, 0, 0, 0, 1, 0, host, one, small, None)
    assert rc == 1 and b"workspace too small" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    rc = lib.foc_background_backward(one, one, one, None, 32.0, 4096, one, one, 2.3, 16, one, one, one, one, need_bg, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    rc = lib.foc_grid_update_apply(ctypes.c_void_p(256), 1, 128, one, None, 128 ** 3, 1.0, 0.95, 0.01, one, None, one, need_dg, None)
    assert rc == 1 and b"workspace too small" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    rc = lib.foc_ffmlp_backward(one, one, one, one, 128, 32, 16, 128, 2, 0, 6, 1, one, one, one, one, need_mlp, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()


def test_entry_points_without_a_deterministic_form_refuse_on_the_host():
    """Before any launch (no device here), with a message that names the entry point and the option; the same calls pass the check with
    the option off (and then fail on their null pointers, which come first only there)."""
    from focnerf_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(8)
    offs = (ctypes.c_int32 * 3)(0, 4920, 4920 + 35944)
    host = ctypes.cast(offs, ctypes.c_void_p)

    def atomic_backward(D, C, dtype):
        return lib.foc_grid_encode_backward(one, one, one, one, one, 64, D, C, 2, 1.0, 16, None, None, 0, 0, 0, dtype, 0, None, None)

    def tv():
        return lib.foc_grad_total_variation(one, one, one, one, 1.0, 64, 3, 2, 2, 1.0, 16, 0, 0, 1, None)

    def binned_f32(ws_bytes):
        return lib.foc_grid_encode_backward_binned(one, one, one, one, one, 4096, 3, 2, 2, 1.0, 16, None, None, 0, 0, 0, 0, 0, host, one, ws_bytes, None)

    _lib.set_option(OPT, 1)
    for D, C, dtype in ((3, 2, 1), (3, 4, 1), (2, 2, 0), (4, 2, 1), (5, 8, 0)):
        assert atomic_backward(D, C, dtype) == 1
        assert b"grid_encode_backward:" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    assert tv() == 1 and b"grad_total_variation:" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    assert binned_f32(1 << 30) == 1 and b"grid_encode_backward_binned:" in lib.foc_last_error() and b"FOC_DETERMINISTIC" in lib.foc_last_error()
    _lib.set_option(OPT, 0)
    assert binned_f32(16) == 1 and b"FOC_DETERMINISTIC" not in lib.foc_last_error() and b"workspace too small" in lib.foc_last_error()


def test_python_raises_runtime_error_naming_the_option():
    from focnerf_amd import _lib
    _lib.set_option(OPT, 1)
    one = ctypes.c_void_p(8)
    with pytest.raises(RuntimeError, match="FOC_DETERMINISTIC"):
        _lib.check(_lib.lib.foc_grad_total_variation(one, one, one, one, 1.0, 64, 3, 2, 2, 1.0, 16, 0, 0, 1, None), "grad_total_variation")
