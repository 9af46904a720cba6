"""ctypes binding of libweasal_hip.so (the C ABI declared in include/weasal_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C weasal_amd/csrc``.
There is NO fallback: if the shared object is missing or a symbol cannot be resolved the
import of any compute path raises, so that a silent CPU/PyTorch substitute can never stand
in for the HIP kernels.

The header is the single source of the binding: ``SIGNATURES`` and the fields of the descriptor
structures (``ABI.structs``) are parsed from its text by ``_abi.parse``, so a new entry needs a
declaration there and nothing here.  A declaration the parser cannot type raises by name.
"""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libweasal_hip.so")

_vp = C.c_void_p


class WeasalHipError(RuntimeError):
    pass


def header_abi(path):
    """_abi.parse of a C header of the library; WeasalHipError if the file is missing"""
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise WeasalHipError("%s not readable (%s): the binding takes every signature and struct layout from it" % (path, e))
    return _abi.parse(text)


HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "weasal_hip.h")
ABI = header_abi(HEADER_PATH)       # prototypes, struct fields and integer constants of the header
SIGNATURES = ABI.prototypes         # name -> (restype, argtypes), one entry per declaration of the header

# diagnostics switches of the library (integer globals), settable from the environment for A/B runs: variable -> symbol
ENV_SWITCHES = (
    ("WEASAL_NB_WIDE_CAPS", "ws_nb_wide_caps"),
    ("WEASAL_CLOSEST_BWD_VEC", "ws_closest_bwd_vec"),
    ("WEASAL_GEMM_STAGED", "ws_gemm_staged"),
    ("WEASAL_GEMM_SHALLOW", "ws_gemm_shallow"),
)

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise WeasalHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C weasal_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)   # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        for env, sym in ENV_SWITCHES:
            if env in os.environ:
                C.c_int.in_dll(handle, sym).value = int(os.environ[env])
        _lib = handle
    return _lib


def check(rc):
    """Map a ws_status to the exception type the reference's modules raise (RuntimeError)."""
    if rc != 0:
        msg = lib().ws_last_error()
        raise WeasalHipError("libweasal_hip status %d: %s" % (rc, msg.decode() if msg else "?"))


def ptr(t):
    """device/host pointer of a tensor (None -> NULL)"""
    return None if t is None else _vp(t.data_ptr())


_raw_stream = None


def current_stream():
    """the calling thread's current HIP stream as a void pointer.  torch.cuda.current_stream() builds a Stream object through
    three Python layers (~12 us per call, ~100 calls per training step: 1 ms of a 3 ms launch-bound step); the raw handle
    comes from one C call."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
        dev = getattr(torch._C, "_cuda_getDevice", None)
        if get is not None and dev is not None and torch.cuda.is_available():
            torch.cuda.current_stream()                          # (initialises the runtime once)
            _raw_stream = lambda: get(dev())
        else:
            _raw_stream = lambda: torch.cuda.current_stream().cuda_stream
    return _vp(_raw_stream())
