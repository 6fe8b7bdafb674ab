"""ctypes binding of libwavenet_logmel.so (include/wavenet_logmel.h): the log-mel front end, a library of its own next to
libwavenet_hip.so.  No fallback: a missing library or a failing call raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import load, raise_on

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwavenet_logmel.so")
ABI_VERSION = 1
WNL_OK, WNL_EARG, WNL_EHIP = 0, -1, -3
WN_LOGMEL_MAX_CLIPS = 64                                     # clips per launch
WN_LOGMEL_REFLECT_LEFT, WN_LOGMEL_REFLECT_RIGHT = 1, 2      # WnLogmelClip.flags: that end of the buffer is the signal's end


class WnLogmelClip(C.Structure):
    """One clip of a wn_logmel launch."""
    _fields_ = [("x", C.c_void_p), ("n", C.c_int64), ("origin", C.c_int64), ("out", C.c_void_p), ("out_stride", C.c_int64),
                ("first", C.c_int32), ("count", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


_SIGS = {
    "wn_logmel_abi_version": (C.c_int, []),
    "wn_logmel_last_error": (C.c_char_p, []),
    "wn_logmel": (C.c_int, [C.POINTER(WnLogmelClip), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                            C.c_int, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)
_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, _SIGS, "wn_logmel_abi_version", ABI_VERSION)
    return _lib


def check(rc: int, what: str = "wn_logmel") -> None:
    raise_on(rc, what, lib().wn_logmel_last_error)
