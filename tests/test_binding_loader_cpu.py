"""The loader and the error path that every ctypes binding shares (wavenet_amd/_lib.py: load, raise_on); no GPU needed."""
import pytest

from wavenet_amd import _lib, _pitch


def test_load_refuses_a_missing_library_and_another_abi_version_and_types_every_entry(tmp_path):
    missing = str(tmp_path / "libwavenet_absent.so")
    with pytest.raises(_lib.WaveNetHipError, match="libwavenet_absent.so not found: build it with `python -m wavenet_amd.build`"):
        _lib.load(missing, _pitch._SIGS, "wn_pitch_abi_version", _pitch.ABI_VERSION)
    with pytest.raises(_lib.WaveNetHipError, match="ABI mismatch: .*libwavenet_pitch.so is version %d, the binding 0" % _pitch.ABI_VERSION):
        _lib.load(_pitch.LIB_PATH, _pitch._SIGS, "wn_pitch_abi_version", 0)
    lib = _lib.load(_pitch.LIB_PATH, _pitch._SIGS, "wn_pitch_abi_version", _pitch.ABI_VERSION)
    for name, (res, args) in _pitch._SIGS.items():
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args, name
    with pytest.raises(AttributeError):                              # an entry that the library does not export
        _lib.load(_pitch.LIB_PATH, dict(_pitch._SIGS, wn_pitch_absent=(None, [])), "wn_pitch_abi_version", _pitch.ABI_VERSION)


def test_raise_on_puts_the_label_the_code_and_the_librarys_last_error_into_the_message():
    lib = _pitch.lib()
    rc = lib.wn_pitch(None, 1, None, 0, 64, 16, 4, 40, 0.15, 1600.0, None)
    assert rc == _pitch.WNP_EARG
    with pytest.raises(_lib.WaveNetHipError, match=r"a label failed \(-1\): wn_pitch: NULL clips"):
        _lib.raise_on(rc, "a label", lib.wn_pitch_last_error)
    with pytest.raises(_lib.WaveNetHipError, match=r"wn_pitch failed \(-1\): wn_pitch: NULL clips"):
        _pitch.check(rc)
    assert _lib.raise_on(0, "a label", lib.wn_pitch_last_error) is None and _pitch.check(0) is None
