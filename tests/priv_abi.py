"""The library's private cross-file entries (`ws_priv_*`, `struct ws_xb_problem` / `ws_xty_problem`), typed for ctypes from
their declarations in weasal_amd/csrc/ws_common.h by the parser that types the public header (weasal_amd/_abi.py)."""
import ctypes as C
import os

from weasal_amd import _lib

ABI = _lib.header_abi(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "ws_common.h"))


def entry(name):
    """the exported function `name` with restype / argtypes as ws_common.h declares it"""
    fn = getattr(_lib.lib(), name)
    fn.restype, fn.argtypes = ABI.prototypes[name]
    return fn


def struct(name):
    """a ctypes.Structure class laid out as `struct name` of ws_common.h"""
    return type(name, (C.Structure,), {"_fields_": ABI.structs[name]})
