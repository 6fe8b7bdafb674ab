"""What LogMel and Pitch inherit from features.ClipAnalyser: how a clip is taken in, refused by the concrete class's name.
Both are built on the CPU device, where nothing is launched (no GPU needed)."""
import numpy as np
import pytest
import torch

from wavenet_amd import features, pitch

MAKE = {"LogMel": lambda: features.LogMel(1600, n_mels=8, hop=16, win=64, device="cpu"),
        "Pitch": lambda: pitch.Pitch(1600, 16, 64, 40.0, 400.0, device="cpu")}


@pytest.mark.parametrize("name", list(MAKE))
def test_an_analyser_takes_floats_or_tokens_and_refuses_a_mix_by_its_own_name(name):
    a = MAKE[name]()
    assert isinstance(a, features.ClipAnalyser) and type(a).__name__ == name
    assert a.device == torch.device("cpu") and a.launches == 0 and a._decode == {}
    for x in (np.zeros(100, np.int32), torch.zeros(100, dtype=torch.int64), np.zeros(100, np.uint8)):
        with pytest.raises(ValueError, match="^%s: integer input \\(torch\\..*\\) is tokens and needs quantization_steps" % name):
            a._signal(x, None)
    for x in (np.zeros(100, np.float32), torch.zeros(100, dtype=torch.float64)):
        with pytest.raises(ValueError, match="^%s: quantization_steps = 256 given with a torch.float.* signal; tokens are integers" % name):
            a._signal(x, 256)
    with pytest.raises(ValueError, match="^%s: integer input" % name):      # the public calls go through the same door
        a(np.zeros(100, np.int32))
    with pytest.raises(ValueError, match="^%s: quantization_steps = 256" % name):
        a.batch([np.zeros(100, np.float32)], 256)
    x64 = np.linspace(-1.0, 1.0, 30).reshape(5, 6)
    t = a._signal(x64, None)
    assert t.dtype == torch.float32 and t.shape == (30,) and t.is_contiguous()
    assert np.array_equal(t.numpy(), x64.reshape(-1).astype(np.float32))
    assert a._signal(torch.zeros(7, dtype=torch.float16), None).dtype == torch.float32
    for tok in (np.arange(40, dtype=np.int64), torch.arange(40, dtype=torch.uint8), np.arange(40, dtype=np.int32)):
        t = a._signal(tok, 256)
        assert t.dtype == torch.int32 and t.tolist() == list(range(40))
    assert a.batch([]) == [] and a.launches == 0


@pytest.mark.parametrize("name", list(MAKE))
def test_an_analyser_caches_one_decode_table_per_quantisation_and_checks_the_range_of_frames(name):
    from wavenet_amd import data
    a = MAKE[name]()
    assert a._table(None) is None and a._decode == {}
    tab = a._table(256)
    assert tab.dtype == torch.float32 and np.array_equal(tab.numpy(), data.mulaw_decode(np.arange(256), 256).astype(np.float32))
    assert a._table(256) is tab and a._table(16).shape == (16,) and sorted(a._decode) == [16, 256]
    x = np.zeros(700, np.float32)                                        # 44 columns at hop = 16
    for first, count, text in [(40, 5, "columns 40 .. 44 of a clip that has 44"), (-1, 2, "columns -1 .. 0 of a clip that has 44"),
                               (3, 0, "columns 3 .. 2 of a clip that has 44")]:
        with pytest.raises(ValueError, match="^%s.frames: %s" % (name, text)):
            a.frames(x, first, count)
    assert a.launches == 0


def test_logmel_keeps_its_length_check_and_pitch_takes_any_length():
    mel, p = MAKE["LogMel"](), MAKE["Pitch"]()
    for call in (lambda: mel(np.zeros(32, np.float32)), lambda: mel.batch([np.zeros(700, np.float32), np.zeros(32, np.float32)]),
                 lambda: mel.frames(np.zeros(32, np.float32), 0, 1)):
        with pytest.raises(ValueError, match="LogMel: a clip of 32 samples; the reflection at its ends needs more than win / 2 = 32"):
            call()
    assert p._check_length(0) is None and mel._check_length(33) is None
    assert mel.launches == 0
