"""ctypes binding of libwavenet_resample.so (include/wavenet_resample.h): sample-rate conversion, a library of its own next to
libwavenet_hip.so.  No fallback: a missing library or a failing call raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import load, raise_on

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwavenet_resample.so")
ABI_VERSION = 1
WNR_OK, WNR_EARG, WNR_EHIP = 0, -1, -3
WN_RESAMPLE_MAX_CLIPS = 64                            # clips per launch
WN_RESAMPLE_TILE = 256                                # outputs per workgroup
WN_RESAMPLE_START, WN_RESAMPLE_END = 1, 2             # WnResampleClip.flags: that end of the buffer is the signal's end
WN_RESAMPLE_IN_PCM16, WN_RESAMPLE_IN_F32 = 0, 1
WN_RESAMPLE_OUT_F32, WN_RESAMPLE_OUT_PCM16, WN_RESAMPLE_OUT_TOKENS = 0, 1, 2
OUT_KIND = {"float": WN_RESAMPLE_OUT_F32, "pcm16": WN_RESAMPLE_OUT_PCM16, "tokens": WN_RESAMPLE_OUT_TOKENS}


class WnResampleClip(C.Structure):
    """One clip of a wn_resample launch."""
    _fields_ = [("x", C.c_void_p), ("n", C.c_int64), ("origin", C.c_int64), ("out", C.c_void_p), ("first", C.c_int64),
                ("count", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_int32)]


_SIGS = {
    "wn_resample_abi_version": (C.c_int, []),
    "wn_resample_last_error": (C.c_char_p, []),
    "wn_resample": (C.c_int, [C.POINTER(WnResampleClip), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                              C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)
_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, _SIGS, "wn_resample_abi_version", ABI_VERSION)
    return _lib


def check(rc: int, what: str = "wn_resample") -> None:
    raise_on(rc, what, lib().wn_resample_last_error)
