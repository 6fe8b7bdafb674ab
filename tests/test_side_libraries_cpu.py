"""The five libraries side by side: the one build table, and what each library exports (no GPU needed).  What a single
library declares, maps and binds is checked in that library's own test."""
import os
import subprocess

import pytest

from wavenet_amd import _corpus, _lib, _logmel, _pitch, _resample, build

# source below csrc/ -> the binding of the library it becomes
SIDE = {"logmel.hip": _logmel, "corpus.hip": _corpus, "front/resample.hip": _resample, "analysis/pitch.hip": _pitch}
# binding -> (number of exports, the word that only its library's names hold)
LIBRARIES = {_lib: (69, None), _logmel: (3, "logmel"), _corpus: (3, "corpus"), _resample: (3, "resample"), _pitch: (3, "pitch")}


def test_the_build_table_sends_each_side_source_to_its_own_library():
    assert build.SIDE_LIBS == {
        "logmel.hip": ("libwavenet_logmel.so", "logmel_exports.map"),
        "corpus.hip": ("libwavenet_corpus.so", "corpus_exports.map"),
        "front/resample.hip": ("libwavenet_resample.so", "front/resample_exports.map"),
        "analysis/pitch.hip": ("libwavenet_pitch.so", "analysis/pitch_exports.map"),
    }
    for src, (name, version_script) in build.SIDE_LIBS.items():
        assert SIDE[src].LIB_PATH == os.path.join(build.HERE, name), src
        assert os.path.exists(os.path.join(build.CSRC, src)) and os.path.exists(os.path.join(build.CSRC, version_script)), src


@pytest.mark.parametrize("binding", list(LIBRARIES), ids=lambda b: b.__name__.rsplit(".", 1)[-1])
def test_a_library_exports_its_bindings_names_and_none_of_another_library(binding):
    count, _ = LIBRARIES[binding]
    nm = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[-1] for ln in nm.splitlines() if ln.strip()]
    assert len(names) == count and sorted(names) == sorted(binding.EXPORTS)
    for other, (_, word) in LIBRARIES.items():
        if other is not binding and word:
            assert not [s for s in names if word in s], (binding.__name__, word)
