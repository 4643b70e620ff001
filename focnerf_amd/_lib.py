"""ctypes binding of libfocnerf_hip.so (the C ABI declared in include/focnerf.h).

There is NO fallback: if the shared library is missing or fails to load, importing this
module raises ImportError, and every op raises RuntimeError when the library reports an
error. PyTorch is used only for device memory and streams (tensor.data_ptr(),
torch.cuda.current_stream()).
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported first: the library then binds to torch's HIP runtime)

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# FOCNERF_LIB_PATH: another build of the same library (A/B timing of kernel variants on one box, tools/ab_libs.sh)
LIB_PATH = os.environ.get("FOCNERF_LIB_PATH") or os.path.join(_HERE, "libfocnerf_hip.so")

c_vp = ctypes.c_void_p


def _find_header():
    """include/focnerf.h of the source tree, or the copy setup.py puts beside this file in an installed package."""
    paths = [os.path.join(os.path.dirname(_HERE), "include", "focnerf.h"), os.path.join(_HERE, "focnerf.h")]
    for p in paths:
        if os.path.exists(p):
            return p
    raise ImportError(f"focnerf_amd: focnerf.h, which the binding is read from, is at neither {paths[0]} nor {paths[1]}")


# The binding is the header: DEFINES name -> int for every `#define FOC_*`, STRUCTS name -> ctypes.Structure for every `typedef struct`,
# SIGNATURES name -> (restype, [argtypes]) for every `foc_*` declaration; a pointer argument is `c_vp` unless it points to one of the structs.
DEFINES, STRUCTS, SIGNATURES = _header.read(_find_header())
globals().update(STRUCTS)       # FocOccTrainNode, FocOccTrainObject, FocOccTrainTail, FocCulledField, FocOptimTensor, FocOptimStep
FOC_F32, FOC_F16, FOC_U8 = DEFINES["FOC_F32"], DEFINES["FOC_F16"], DEFINES["FOC_U8"]      # FOC_U8: images of foc_batch_sample only


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"focnerf_amd: {LIB_PATH} is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C focnerf_amd/csrc`. There is no CPU or PyTorch fallback for these ops.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise ImportError(f"focnerf_amd: failed to load {LIB_PATH}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.restype = res
        fn.argtypes = args
    return lib


class _Stream(ctypes.c_void_p):
    """hipStream_t handle that remembers the device of the tensor it was taken for (`stream_of`)."""
    device_index = None


_multi_device = None        # torch.cuda.device_count() > 1, asked once (counting devices does not initialise the GPU)


def _on_tensor_device(fn):
    """Entry points taking a stream run with the device of THEIR tensors current. The library's own guard (csrc/common.h FocDeviceGuard)
    reads the device from the stream handle, and torch's default stream is the null handle on every device — `cuda:1` tensors on their
    default stream while `cuda:0` is current would launch on device 0 with device-1 pointers. The device therefore comes from the
    tensor `stream_of` was called with. One-GPU processes skip the check."""
    def call(*args):
        global _multi_device
        if _multi_device is None:
            _multi_device = torch.cuda.device_count() > 1
        if _multi_device and args:
            idx = getattr(args[-1], "device_index", None)
            if idx is not None and idx != torch.cuda.current_device():
                with torch.cuda.device(idx):
                    return fn(*args)
        return fn(*args)
    call.__name__ = getattr(fn, "__name__", "foc_call")
    return call


class _Lib:
    """The loaded library with every stream-taking entry point wrapped by `_on_tensor_device`."""

    def __init__(self, cdll):
        self._cdll = cdll
        for name, (_, args) in SIGNATURES.items():
            fn = getattr(cdll, name)
            setattr(self, name, _on_tensor_device(fn) if args and args[-1] is c_vp and not name.endswith("_bytes") else fn)


lib = _Lib(_load())


def check(rc, what=""):
    if rc != 0:
        msg = lib.foc_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"focnerf_amd {what}: {msg} (code {rc})")


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) if os.environ.get("FOC_RAW_STREAM", "1") != "0" else None


def raw_stream(index):
    """hipStream_t (as an int) of torch's current stream on device `index`. `torch.cuda.current_stream(dev).cuda_stream` builds a Stream
    object per call (4.7 us: the largest single item of the occupancy render loop's host time, ten calls per iteration); torch's raw
    accessor returns the handle itself."""
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def stream_of(t=None):
    """hipStream_t of torch's current stream on the tensor's device."""
    dev = t.device if t is not None else None
    index = dev.index if dev is not None and dev.index is not None else torch.cuda.current_device()
    s = _Stream(raw_stream(index))
    s.device_index = index
    return s


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("focnerf_amd: expected a CUDA(HIP) tensor; these ops have no CPU implementation")


def dtype_code(t):
    if t.dtype == torch.float32:
        return FOC_F32
    if t.dtype == torch.float16:
        return FOC_F16
    raise RuntimeError(f"focnerf_amd: unsupported dtype {t.dtype} (float32 or float16 expected)")


# ---------------------------------------------------------------- library options (csrc/common.h FocOpt, include/focnerf.h foc_set_option)
def get_option(name):
    """Current value of a library switch (an int; FOC_OCC_MARCH_FORM: -1 auto, 0 two, 1 row, 2 lane, 3 staged)."""
    v = ctypes.c_int(0)
    check(lib.foc_get_option(name.encode(), ctypes.cast(ctypes.byref(v), ctypes.c_void_p)), "get_option")
    return v.value


def set_option(name, value):
    """Set a library switch for the rest of the process (the environment variable of the same name only sets its INITIAL value)."""
    check(lib.foc_set_option(name.encode(), int(value)), "set_option")


class option:
    """`with option("FOC_GB_FACTORED", 0): ...` — a switch set for the block and put back afterwards (tests, A/B runs)."""

    def __init__(self, name, value):
        self.name, self.value = name, int(value)

    def __enter__(self):
        self.old = get_option(self.name)
        set_option(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.name, self.old)
        return False
