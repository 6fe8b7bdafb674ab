"""Compile wavenet_amd/csrc/*.hip into wavenet_amd/libwavenet_hip.so for gfx950 -- all but the sources of ``SIDE_LIBS``:
logmel.hip becomes wavenet_amd/libwavenet_logmel.so (include/wavenet_logmel.h) and corpus.hip wavenet_amd/libwavenet_corpus.so
(include/wavenet_corpus.h), libraries of their own: the first one's exports are pinned.  ``FRONT_LIBS`` does the same for the
sources of wavenet_amd/csrc/front/, which the ``csrc/*.hip`` glob does not see: front/resample.hip becomes
wavenet_amd/libwavenet_resample.so (include/wavenet_resample.h).  ``ANALYSIS_LIBS`` is the same table for wavenet_amd/csrc/analysis/:
analysis/pitch.hip becomes wavenet_amd/libwavenet_pitch.so (include/wavenet_pitch.h).

hipcc cross-compiles without a GPU, so this runs in the build container; the .so then travels
in-tree to the GPU box.  Usage: ``python -m wavenet_amd.build [--force]``.
"""
from __future__ import annotations

import glob
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "build")
LIB = os.path.join(HERE, "libwavenet_hip.so")
LOGMEL_LIB = os.path.join(HERE, "libwavenet_logmel.so")
CORPUS_LIB = os.path.join(HERE, "libwavenet_corpus.so")
# source -> (library, version script): a source that is a library of its own; every other source goes into LIB
SIDE_LIBS = {
    "logmel.hip": (LOGMEL_LIB, "logmel_exports.map"),
    "corpus.hip": (CORPUS_LIB, "corpus_exports.map"),
}
RESAMPLE_LIB = os.path.join(HERE, "libwavenet_resample.so")
# source below csrc/ -> (library, version script): front ends in a directory of their own, one library each
FRONT_LIBS = {
    "front/resample.hip": (RESAMPLE_LIB, "front/resample_exports.map"),
}
PITCH_LIB = os.path.join(HERE, "libwavenet_pitch.so")
# source below csrc/ -> (library, version script): analysers of audio, handled like the front ends
ANALYSIS_LIBS = {
    "analysis/pitch.hip": (PITCH_LIB, "analysis/pitch_exports.map"),
}
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -fvisibility=hidden: only what include/wavenet_hip.h declares (inside its `#pragma GCC visibility push(default)`) is exported
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-Wno-inline-asm"] + \
    os.environ.get("WAVENET_HIP_EXTRA_FLAGS", "").split()


def _newest_header() -> float:
    hs = glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))
    return max(os.path.getmtime(h) for h in hs)


def _compile(src: str, force: bool, hdr_mtime: float) -> str:
    obj = os.path.join(OBJ, os.path.basename(src).replace(".hip", ".o"))
    if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(src), hdr_mtime):
        return obj
    cmd = [HIPCC] + FLAGS + ["-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s\n%s" % (src, r.stdout, r.stderr))
    if r.stderr.strip():
        sys.stderr.write(r.stderr)
    return obj


def _link(lib: str, objs, version_script: str, force: bool) -> None:
    if force or not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs):
        # the version script drops what hipcc itself adds to the dynamic table (one __hip_cuid_* marker per translation unit)
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden",
               "-Wl,--version-script=" + os.path.join(CSRC, version_script), "-o", lib] + list(objs)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n%s\n%s" % (r.stdout, r.stderr))


def build(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(OBJ, exist_ok=True)
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    hdr = _newest_header()
    with ThreadPoolExecutor(max_workers=min(6, len(srcs))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, hdr), srcs))
    side = {os.path.basename(s): o for s, o in zip(srcs, objs) if os.path.basename(s) in SIDE_LIBS}
    _link(LIB, [o for o in objs if o not in side.values()], "exports.map", force)
    for src, (lib, version_script) in SIDE_LIBS.items():
        _link(lib, [side[src]], version_script, force)
    for src, (lib, version_script) in list(FRONT_LIBS.items()) + list(ANALYSIS_LIBS.items()):
        _link(lib, [_compile(os.path.join(CSRC, src), force, hdr)], version_script, force)
    if verbose:
        for lib in [LIB] + [lib for lib, _ in list(SIDE_LIBS.values()) + list(FRONT_LIBS.values()) + list(ANALYSIS_LIBS.values())]:
            print("built", lib)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
