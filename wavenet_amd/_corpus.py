"""ctypes binding of libwavenet_corpus.so (include/wavenet_corpus.h): training crops gathered from a device-resident corpus, a
library of its own next to libwavenet_hip.so and libwavenet_logmel.so.  No fallback: a missing library or a failing call
raises."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from ._lib import load, raise_on

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libwavenet_corpus.so")
ABI_VERSION = 1
WNC_OK, WNC_EARG, WNC_EHIP = 0, -1, -3


class WnCorpusDesc(C.Structure):
    """The corpus of a wn_corpus_gather call: device pointers and the scalars of the padding rule."""
    _fields_ = [("tokens", C.c_void_p), ("file_offset", C.c_void_p), ("file_len", C.c_void_p), ("file_class", C.c_void_p),
                ("features", C.c_void_p), ("col_offset", C.c_void_p), ("col_count", C.c_void_p), ("total_cols", C.c_int64),
                ("n_files", C.c_int32), ("token_bytes", C.c_int32), ("F", C.c_int32), ("hop", C.c_int32),
                ("input_width", C.c_int32), ("silence", C.c_int32), ("pad_cols", C.c_int32), ("shift", C.c_int32)]


_SIGS = {
    "wn_corpus_abi_version": (C.c_int, []),
    "wn_corpus_last_error": (C.c_char_p, []),
    "wn_corpus_gather": (C.c_int, [C.POINTER(WnCorpusDesc), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(_SIGS)
_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = load(LIB_PATH, _SIGS, "wn_corpus_abi_version", ABI_VERSION)
    return _lib


def check(rc: int, what: str = "wn_corpus_gather") -> None:
    raise_on(rc, what, lib().wn_corpus_last_error)
