"""ctypes binding of ``libuavgnn.so`` - the C-ABI declared in ``include/uavgnn.h``.

The header is the only place where an entry point or an ABI constant is declared: ``SIGNATURES`` and the ``UAVGNN_*`` constants of
this module are read from its text at import (``parse_header``); nothing here restates a prototype.
PyTorch only supplies device memory and the current HIP stream; every call passes raw pointers and sizes.
There is NO CPU fallback: if the shared library is missing, or a tensor is not on the GPU, the call raises.
"""
from __future__ import annotations

import ctypes
import os
import re

import torch as th  # imported first on purpose: libuavgnn must bind to the HIP runtime torch already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
# UAVGNN_LIB: another build of the same library (kernel A/Bs of the probes: a variant compiled with different -D switches)
LIB_PATH = os.environ.get("UAVGNN_LIB") or os.path.join(_HERE, "csrc", "libuavgnn.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "uavgnn.h")   # the include directory build.py compiles against
# the second shared object: entry points that replace no reference call site (include/uavgnn_ext.h, csrc/ext/*.hip)
EXT_LIB_PATH = os.environ.get("UAVGNN_EXT_LIB") or os.path.join(_HERE, "csrc", "libuavgnn_ext.so")
EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "uavgnn_ext.h")
# the third: the quantile-regression head and its TD tail (include/uavgnn_qr.h, csrc/qr/*.hip)
QR_LIB_PATH = os.environ.get("UAVGNN_QR_LIB") or os.path.join(_HERE, "csrc", "libuavgnn_qr.so")
QR_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "uavgnn_qr.h")


class UavGnnError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
            "size_t": ctypes.c_size_t, "uavgnn_stream_t": ctypes.c_void_p}
# HOST arrays keep a typed pointer (ctypes then refuses an array of another element type); they are told by their parameter name,
# which no device pointer bears.  Every other pointer is c_void_p: callers pass data_ptr() integers and None.
_HOST_ARRAYS = {"int_consts": ctypes.POINTER(ctypes.c_int32), "f64_consts": ctypes.POINTER(ctypes.c_double),
                "fields": ctypes.POINTER(ctypes.c_longlong),
                "seen_params": ctypes.POINTER(ctypes.c_void_p), "near_params": ctypes.POINTER(ctypes.c_void_p)}


def _ctype(words, name, decl):
    """ctypes class of a result (name None) or of the parameter `name` whose type is the token list `words`."""
    if "*" in words:
        if name is None:
            return ctypes.c_char_p if words == ["const", "char", "*"] else ctypes.c_void_p
        return _HOST_ARRAYS.get(name, ctypes.c_void_p)
    c_type = " ".join(w for w in words if w != "const")
    if c_type not in _SCALARS:      # never a default: ctypes' own (int) is the silent truncation this table exists to rule out
        raise UavGnnError(f"no ctypes class for the type `{' '.join(words)}` of {name or 'the result'} in the declaration `{decl}`")
    return _SCALARS[c_type]


def parse_header(text: str):
    """(signatures, constants) of the text of a C header: name -> (restype, [argtypes]) for every ``<type> uavgnn_name(<params>);``
    and NAME -> value for every ``#define UAVGNN_NAME <integer>``.  Anything it cannot read raises UavGnnError with the declaration."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(UAVGNN_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                 # preprocessor lines
    text = re.sub(r'extern\s*"C"\s*\{|\}', "", text)                     # the extern "C" wrapper
    signatures = {}
    for decl in text.split(";"):
        decl = " ".join(decl.split())
        if not decl or decl.startswith("typedef "):                      # uavgnn_stream_t is in _SCALARS
            continue
        m = re.fullmatch(r"(.+?)\b(uavgnn_\w+) ?\((.*)\)", decl)
        if not m or m[2] in signatures:
            raise UavGnnError(f"not a prototype `<type> uavgnn_name(<params>)`, or a second one of its name: `{decl}`")
        restype = _ctype(m[1].replace("*", " * ").split(), None, decl)
        params = [] if m[3].strip() == "void" else [p.replace("*", " * ").split() or [""] for p in m[3].split(",")]
        signatures[m[2]] = (restype, [_ctype(p[:-1], p[-1], decl) for p in params])         # the last identifier is the name
    return signatures, constants


def _read_header(path=None):
    path = HEADER_PATH if path is None else path
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise UavGnnError(f"{path} is missing ({e}): the ctypes table and the UAVGNN_* constants are read from the header") from e


# name -> (restype, argtypes), and every UAVGNN_* integer macro (error codes, GEMM epilogue / variant bits, TD-return and workspace
# kinds) as an attribute of this module.  tests/test_cabi_symbols.py pins a set of entries by hand against this reading.
SIGNATURES, _CONSTANTS = _read_header()
globals().update(_CONSTANTS)
# the same reading of include/uavgnn_ext.h; it defines no constant of its own (the error codes are the main library's)
EXT_SIGNATURES = _read_header(EXT_HEADER_PATH)[0]
# and of include/uavgnn_qr.h (no constant of its own either)
QR_SIGNATURES = _read_header(QR_HEADER_PATH)[0]

_LIB = None
_EXT = None
_QR = None


def lib() -> ctypes.CDLL:
    """Loads libuavgnn.so once.  Fails loudly when it has not been built (``__graft_entry__.build()``)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise UavGnnError(f"{LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; "
                              f"g.build()'`.  uav_bs_ctrl_amd has no CPU / eager fallback.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _LIB = handle
        # Recorded vendor-GEMM solutions for the dense half of the path (uav_bs_ctrl_amd/tuned) are OPT-IN: PyTorch's
        # TunableOp switch is process-wide and would change GEMM selection for every other model of the host
        # application.  UAVGNN_TUNED_GEMM=1 or an explicit uav_bs_ctrl_amd.enable_tuned_gemms() turns it on
        # (bench.py does).
        if os.environ.get("UAVGNN_TUNED_GEMM", "0") == "1":
            from .tuned import enable_tuned_gemms
            enable_tuned_gemms()
    return _LIB


def ext() -> ctypes.CDLL:
    """Loads libuavgnn_ext.so once (``build.build_lib`` builds it beside the main library).  Fails loudly when it is missing."""
    global _EXT
    if _EXT is None:
        if not os.path.exists(EXT_LIB_PATH):
            raise UavGnnError(f"{EXT_LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; "
                              f"g.build()'`.  uav_bs_ctrl_amd has no CPU / eager fallback.")
        handle = ctypes.CDLL(EXT_LIB_PATH)
        for name, (res, args) in EXT_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _EXT = handle
    return _EXT


def qr() -> ctypes.CDLL:
    """Loads libuavgnn_qr.so once (``build.build_lib`` builds it beside the other two).  Fails loudly when it is missing."""
    global _QR
    if _QR is None:
        if not os.path.exists(QR_LIB_PATH):
            raise UavGnnError(f"{QR_LIB_PATH} is missing - build it with `python -c 'import __graft_entry__ as g; "
                              f"g.build()'`.  uav_bs_ctrl_amd has no CPU / eager fallback.")
        handle = ctypes.CDLL(QR_LIB_PATH)
        for name, (res, args) in QR_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _QR = handle
    return _QR


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().uavgnn_strerror(code).decode()
        raise UavGnnError(f"{what} failed with code {code}: {msg}")


def ptr(t: th.Tensor | None):
    """Raw device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def ptr_array(tensors):
    """Host array of device pointers (NULL for None) for the entry points that take a parameter block."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


_RAW_STREAM = getattr(th._C, "_cuda_getCurrentRawStream", None)


def stream() -> int:
    """The HIP stream PyTorch is currently recording on (so launches order with torch ops and graph capture works).  Through the raw
    accessor where this PyTorch has it: ``torch.cuda.current_stream()`` builds a Stream object behind three layers of device-index
    helpers (2.7 us against 0.3 - and a rollout step asks ten times)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(th.cuda.current_device())
    return th.cuda.current_stream().cuda_stream


def require_gpu(*tensors: th.Tensor) -> None:
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise UavGnnError("uav_bs_ctrl_amd ops run on the MI355X only: got a CPU tensor (no CPU fallback exists; "
                              "move the module and the graph to 'cuda').")


def f32c(t: th.Tensor) -> th.Tensor:
    """float32 + contiguous view of t (no copy when already so)."""
    if t.dtype != th.float32:
        raise UavGnnError(f"expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()
