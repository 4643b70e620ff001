"""CPU: the C-ABI library loads and exports every symbol include/focnerf.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from util import HEADER, build_c_abi_consumer, c_struct_layouts

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(REPO, "include", "focnerf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(foc_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_expected_entry_points():
    names = _declared()
    for n in ["foc_near_far_from_aabb", "foc_march_rays_train", "foc_composite_rays_train_forward",
              "foc_composite_rays_train_backward", "foc_march_rays", "foc_composite_rays", "foc_grid_encode_forward",
              "foc_grid_encode_backward", "foc_grad_total_variation", "foc_freq_encode_forward", "foc_freq_encode_backward",
              "foc_ffmlp_forward", "foc_ffmlp_inference", "foc_ffmlp_backward", "foc_combine_select"]:
        assert n in names


def test_library_exports_every_declared_symbol():
    from focnerf_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in _declared():
        assert hasattr(lib, n), f"{n} declared in include/focnerf.h but not exported"
    assert set(_lib.SIGNATURES) == set(_declared()), "focnerf_amd/_lib.py binds a different set than the header declares"


def test_abi_version_and_arch():
    from focnerf_amd import _lib
    assert _lib.lib.foc_abi_version() == 2
    assert _lib.lib.foc_arch() == b"gfx950"
    assert isinstance(_lib.lib.foc_last_error(), bytes)           # (empty in a fresh process; other tests of a session may have left theirs)


def test_argument_validation_needs_no_gpu():
    """Null pointers / bad shapes are rejected on the host before any launch."""
    from focnerf_amd import _lib
    lib = _lib.lib
    assert lib.foc_near_far_from_aabb(None, None, None, 4, 0.2, None, None, None) == 1
    assert b"null pointer" in lib.foc_last_error()
    one = ctypes.c_void_p(8)  # never dereferenced: validation fails first
    rc = lib.foc_grid_encode_forward(one, one, one, one, 4, 3, 3, 16, 1.0, 16, None, 0, 0, 0, 0, None, None)
    assert rc == 1 and b"C must be 1, 2, 4, or 8" in lib.foc_last_error()
    rc = lib.foc_ffmlp_forward(one, one, 128, 32, 16, 48, 2, 0, 6, one, one, None)
    assert rc == 1 and b"hidden_dim" in lib.foc_last_error()
    rc = lib.foc_ffmlp_forward(one, one, 128, 24, 16, 64, 2, 0, 6, one, one, None)
    assert rc == 1 and b"input_dim" in lib.foc_last_error()
    rc = lib.foc_freq_encode_forward(one, 4, 3, 4, 26, one, None)
    assert rc == 1
    # ABI 2: the MLP backward's workspace travels with its size; a buffer sized by version 1's blob formula (~50 KB) is refused, not overrun
    need = lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2)
    assert need > 10 * 1024 * 1024
    rc = lib.foc_ffmlp_backward(one, one, one, None, 128, 32, 16, 64, 2, 0, 6, 1, None, one, one, one, 64 * (32 + 64 + 16) * 4, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error()
    rc = lib.foc_ffmlp_backward_planar(one, one, one, 128, 32, 16, 64, 2, 0, 6, 1, one, one, one, need - 1, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error()
    # the colour head with an object feature needs the 48-wide sizing: a buffer sized for 32 inputs is refused
    rc = lib.foc_color_head_backward(one, one, one, 1, None, one, 128, 64, 2, 0, one, one, one, lib.foc_ffmlp_backward_workspace_bytes(32, 64, 2), 4, one, None, None)
    assert rc == 1 and b"workspace of" in lib.foc_last_error()


STRUCTS = ["FocCulledField", "FocOccTrainNode", "FocOccTrainObject", "FocOccTrainTail", "FocOptimTensor", "FocOptimStep"]


@pytest.fixture(scope="module")
def c_layouts(tmp_path_factory):
    return c_struct_layouts(tmp_path_factory.mktemp("layout"), STRUCTS)


def test_the_binding_has_exactly_the_headers_structs():
    from focnerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.findall(r"typedef\s+struct\s+(\w+)", text) == STRUCTS == list(_lib.STRUCTS)
    assert all(getattr(_lib, n) is _lib.STRUCTS[n] and issubclass(_lib.STRUCTS[n], ctypes.Structure) for n in STRUCTS)
    assert ctypes.sizeof(_lib.FocCulledField) == 48


@pytest.mark.parametrize("name", STRUCTS)
def test_struct_layout_matches_the_header(name, c_layouts):
    """Every struct that travels by pointer, as gcc lays out include/focnerf.h against its ctypes class (focnerf_amd/_lib.py, read from the
    same header by focnerf_amd/_header.py): the field names in order — found here by tests/util.py's own regex —, sizeof, and the offset
    of every field."""
    from focnerf_amd import _lib
    S = getattr(_lib, name)
    size, offsets = c_layouts[name]
    assert list(offsets) == [f[0] for f in S._fields_]
    assert size == ctypes.sizeof(S)
    assert offsets == {n: getattr(S, n).offset for n in offsets}


def test_occ_train_node_struct_matches_the_header_and_is_validated_on_the_host():
    """include/focnerf.h `FocOccTrainNode` (its layout: test_struct_layout_matches_the_header above): a null node, a node of another size and
    an empty node are refused before any launch."""
    from focnerf_amd import _lib
    assert len(_lib.FocOccTrainNode._fields_) == 69 and _lib.FocOccTrainNode._fields_[0][0] == "struct_bytes"
    lib = _lib.lib
    for fn in (lib.foc_occ_train_forward, lib.foc_occ_train_backward):
        assert fn(None, None) == 1 and b"null node" in lib.foc_last_error()
        node = _lib.FocOccTrainNode()
        node.struct_bytes = ctypes.sizeof(_lib.FocOccTrainNode) - 8
        assert fn(ctypes.byref(node), None) == 1 and b"bytes" in lib.foc_last_error()
        node.struct_bytes = ctypes.sizeof(_lib.FocOccTrainNode)
        assert fn(ctypes.byref(node), None) == 1 and b"empty node" in lib.foc_last_error()
        node.cap, node.n_rays = 128, 4
        assert fn(ctypes.byref(node), None) == 1 and b"workspace" in lib.foc_last_error()


# ---------------------------------------------------------------- the header reader (focnerf_amd/_header.py)
def _same(got, want):
    return got[0] is want[0] and len(got[1]) == len(want[1]) and all(g is w for g, w in zip(got[1], want[1]))


def test_reader_gives_these_signatures_literally():
    """One entry point per row of the reader's type map, written out by hand and compared by identity: the ctypes functions get exactly
    these objects, and `c_vp` is what bench.py and the stream-wrapping of `_lib._Lib` test a last argument against."""
    from ctypes import POINTER, c_char_p, c_double as f64, c_float as f32, c_int, c_size_t, c_uint32 as u32, c_uint64 as u64
    from focnerf_amd import _lib
    vp, S = _lib.c_vp, _lib.SIGNATURES
    assert vp is ctypes.c_void_p and isinstance(S, dict) and all(isinstance(a, list) for _, a in S.values())
    want = {
        "foc_last_error": (c_char_p, []),                                                       # `const char *` returned, `(void)`
        "foc_abi_version": (c_int, []),
        "foc_set_option": (c_int, [c_char_p, c_int]),                                           # `const char *` taken
        "foc_march_rays_train_scratch_bytes": (u64, [u32, u32]),                                # a uint64_t return
        "foc_optim_workspace_bytes": (c_size_t, [c_int]),                                       # size_t
        "foc_score_view": (c_int, [vp, vp, u32, u32, u32, vp, u32, f64, f64, vp, vp, u64, vp]),   # double, uint64_t
        "foc_combine_select_composite": (c_int, [vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp]),      # `const float *const *`
        "foc_occ_train_forward_tail": (c_int, [POINTER(_lib.FocOccTrainNode), POINTER(_lib.FocOccTrainObject), f32, POINTER(_lib.FocOccTrainTail), vp]),
        "foc_combine_select_composite_culled": (c_int, [POINTER(_lib.FocCulledField), u32, u32, vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp,
                                                        vp, vp, vp, vp]),
        "foc_philox4x32_10": (c_int, [vp, vp, vp]),                                             # `uint32_t *`: a pointer like every other
        "foc_packbits": (c_int, [vp, u32, f32, vp, vp]),                                        # `uint8_t *`
    }
    for name, sig in want.items():
        assert _same(S[name], sig), (name, S[name])
    assert _lib.FocOptimTensor._fields_[5:8] == [("lr_tensor", vp), ("n", ctypes.c_int64), ("lr", f64)]                      # int64_t
    assert _lib.FocOptimStep._fields_[2:4] == [("n_tensors", ctypes.c_int32), ("phase", u32)]                                # int32_t
    assert dict(_lib.FocOptimStep._fields_)["tensors"] is POINTER(_lib.FocOptimTensor)
    assert _lib.FocOccTrainNode._fields_[10:15] == [(n, vp) for n in ("rays_o", "rays_d", "aabb", "jitter", "bitfield")]    # `a, *b` lists
    assert (_lib.FOC_F32, _lib.FOC_F16, _lib.FOC_U8) == (0, 1, 2) and _lib.DEFINES["FOC_OPTIM_CHUNK"] == 4096
    assert all(n.startswith("FOC_") and type(v) is int for n, v in _lib.DEFINES.items()) and len(_lib.DEFINES) == 17


def test_header_is_looked_for_in_the_tree_then_beside_the_package(tmp_path, monkeypatch):
    from focnerf_amd import _lib
    assert os.path.samefile(_lib._find_header(), HEADER)
    monkeypatch.setattr(_lib, "_HERE", str(tmp_path / "site" / "focnerf_amd"))
    with pytest.raises(ImportError) as e:
        _lib._find_header()
    assert str(tmp_path / "site" / "include" / "focnerf.h") in str(e.value) and str(tmp_path / "site" / "focnerf_amd" / "focnerf.h") in str(e.value)
    os.makedirs(tmp_path / "site" / "focnerf_amd")
    (tmp_path / "site" / "focnerf_amd" / "focnerf.h").write_text("")
    assert _lib._find_header() == str(tmp_path / "site" / "focnerf_amd" / "focnerf.h")       # an installed package: setup.py's copy


def test_reader_reads_a_small_header():
    from focnerf_amd import _header
    defines, structs, sigs = _header.parse("""
        /* a comment with int foc_not_this(void); inside */
        #ifndef H
        #define H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define FOC_N 0x10   /* sixteen */
        typedef struct FocA { uint32_t n, m; const float *p, *q; double d; } FocA;   // trailing
        typedef struct FocB { const FocA *a; FocA **list; int64_t k; } FocB;
        uint64_t foc_f(const FocB *b, const FocA *const *as, const char *name,
                       int32_t i, void *stream);
        const char *foc_g(void);
        #ifdef __cplusplus
        }
        #endif
        #endif
    """)
    A, B, vp = structs["FocA"], structs["FocB"], ctypes.c_void_p
    assert defines == {"FOC_N": 16} and list(structs) == ["FocA", "FocB"] and list(sigs) == ["foc_f", "foc_g"]
    assert A._fields_ == [("n", ctypes.c_uint32), ("m", ctypes.c_uint32), ("p", vp), ("q", vp), ("d", ctypes.c_double)]
    assert B._fields_ == [("a", ctypes.POINTER(A)), ("list", vp), ("k", ctypes.c_int64)]
    assert _same(sigs["foc_f"], (ctypes.c_uint64, [ctypes.POINTER(B), vp, ctypes.c_char_p, ctypes.c_int32, vp]))
    assert _same(sigs["foc_g"], (ctypes.c_char_p, []))


@pytest.mark.parametrize("text, names", [
    ("int foc_f(uint16_t n);", "uint16_t"),                                  # an unknown scalar: never taken for a pointer or an int
    ("int foc_f(uint8_t n);", "uint8_t"),                                    # known behind a pointer only
    ("int foc_f(unsigned int n);", "unsigned int n"),
    ("int foc_f(hipStream_t *s);", "hipStream_t"),
    ("long foc_f(void);", "long"),
    ("int foc_f(uint32_t);", "uint32_t"),                                    # an argument without a name
    ("int foc_f();", "foc_f"),
    ("int foc_f(const FocLater *p);\ntypedef struct FocLater { int a; } FocLater;", "FocLater"),     # a struct not declared yet
    ("typedef struct FocA { const FocNone *p; } FocA;", "FocNone"),
    ("typedef struct FocA { float v[3]; } FocA;", "v[3]"),
    ("typedef struct FocA { uint32_t a : 3; } FocA;", "a : 3"),
    ("int foc_f(void);\nint other(void);", "other"),                         # stray text: a declaration that is not foc_*
    ("static int foc_f(void);", "static"),
    ("int foc_f(void (*cb)(int));", "cb"),
    ("int foc_f(void)\nint foc_g(void);", "foc_f"),                          # a lost semicolon
    ("int foc_f(void);\n}", "}"),
    ('extern "C" {\nint foc_f(void);', "never closed"),
    ("#if FOC_X\nint foc_f(void);\n#endif", "#if FOC_X"),                    # a declaration behind a condition it cannot evaluate
    ("#define FOC_X 1.5f", "1.5f"),
    ("#define FOC_X (1 << \\\n 4)", "FOC_X"),
])
def test_reader_refuses_what_it_does_not_know(text, names):
    from focnerf_amd import _header
    with pytest.raises(ImportError) as e:
        _header.parse(text)
    assert names in str(e.value), str(e.value)


def test_a_c_caller_links_the_library_and_gets_host_side_refusals(tmp_path):
    """tests/c_abi_consumer.cpp, mode "cpu": a program that is not Python includes include/focnerf.h, links libfocnerf_hip.so and gets the ABI
    version, refusals with messages, the option table — without a device (the device half runs in tests/test_gpu_edge_cases.py)."""
    import subprocess
    import oracle                                                    # noqa: F401 — builds oracle/_build/liboracle.so if it is missing
    exe = build_c_abi_consumer(tmp_path)
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "C_ABI_CONSUMER_OK cpu" in r.stdout, r.stdout + r.stderr


def test_device_selection_rule_of_the_entry_points():
    """csrc/common.h FocDeviceGuard: a non-null stream decides; the NULL stream (torch's default stream on EVERY device) says nothing, then
    the first pointer argument's device does — a C caller with cuda:1 buffers on the default stream while cuda:0 is current; neither: the
    current device. (The two-device launch itself is tests/test_gpu_edge_cases.py::test_ops_follow_their_tensors_device, skipped below 2 GPUs.)"""
    from focnerf_amd import _lib
    pick = _lib.lib.foc_guard_pick_device
    assert pick(0, 3, 1, 0) == 3            # a real stream: its device, whatever the pointer or the current device say
    assert pick(1, -1, 1, 0) == 1           # NULL stream, device-1 pointer, device 0 current: device 1
    assert pick(1, 2, 1, 0) == 1            # a stream device reported for the NULL handle is ignored
    assert pick(1, -1, -1, 2) == 2          # NULL stream, no device pointer (host memory / NULL): stay where we are
    assert pick(0, -1, 1, 0) == 1           # a stream whose device cannot be read: fall back to the pointer
    assert pick(0, -1, -1, 5) == 5


def test_forward_index_path_admission_needs_no_gpu():
    """Which index arithmetic the fp16 D = 3 C = 2 forward takes per level (csrc/gridencoder.hip ge_forward_level): 24-bit multiplies up to
    2^22 rows, 32-bit byte offsets up to 2^30 rows (hashed levels: power-of-two sizes only), the general form beyond — the guard itself,
    asked on the host (a 2^30-row level is 4 GB of table: the GPU tests stop at 2^23)."""
    from focnerf_amd import _lib
    path = _lib.lib.foc_grid_forward_index_path
    assert path(4920, 16, 0) == 2                              # dense level 0 of the NeRF grid
    assert path(1 << 19, 2048, 373248) == 2                    # a hashed 2^19-row level
    assert path(1 << 22, 2048, 0) == 2 and path((1 << 22) + 8, 160, 0) == 1      # the 24-bit limit (a dense level of 2^22 + 8 rows: generic offsets)
    assert path(1 << 23, 2048, 0) == 1 and path(1 << 30, 4096, 0) == 1
    assert path((1 << 30) + 8, 4096, 0) == 0                   # beyond 2^30 rows: byte offsets no longer fit 32 bits
    assert path(1 << 31, 4096, 0) == 0
    assert path((1 << 19) + 8, 2048, 0) == 0                   # hashed, not a power of two: `%` is no mask
    assert path(1 << 19, 2048, 1) == 0 and path((1 << 19) + 1, 40, 0) == 0       # odd offset / odd size: row pairs not 8-byte aligned


def test_ops_refuse_cpu_tensors():
    import torch
    from focnerf_amd import raymarching
    if torch.cuda.is_available():
        pytest.skip("host-only check")
    with pytest.raises(Exception):   # .cuda() on a GPU-less host, or the explicit CUDA-tensor check
        raymarching.near_far_from_aabb(torch.zeros(4, 3), torch.ones(4, 3), torch.tensor([-1., -1, -1, 1, 1, 1]), 0.2)
