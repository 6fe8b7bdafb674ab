"""Batched generation without a GPU: the header's new limit, the command-line flags, the prompt reader, and the argument
checks of ``FasterWaveNet.generate_batch`` that come before any device work."""
import os
import re
import subprocess

import numpy as np
import pytest

from wavenet_amd import FasterWaveNet, Params, _lib, data
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate
from wavenet_amd.train_audio.train import input_width_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"residual_conv_channels": [8, 8, 8], "residual_num_blocks": 2, "causal_conv_channels": [8],
         "softmax_conv_channels": [16, 256]}


def test_header_defines_the_any_shape_limit_and_the_abi_keeps_its_69_names():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    m = re.findall(r"^#define\s+WN_DECODER_BATCH_MAX_ANY\s+(\d+)", hdr, flags=re.M)
    assert m == ["1024"]
    assert _lib.WN_DECODER_BATCH_MAX_ANY == 1024
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    # the export map lets wn_* / wn16_* through: what it makes of the library is the library's dynamic symbol table
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    mapped = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert declared == mapped == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 69
    assert _lib.ABI_VERSION == 5


def test_new_flags_parse_and_their_absence_changes_nothing():
    a = cli_args.parse([])
    assert a.utterances is None and a.prompt is None
    assert cli_args.utterance_prompts(a) == (None, None)
    rest = {k: v for k, v in vars(a).items() if k not in ("utterances", "prompt")}
    assert rest == dict(gpu_device=0, wav_dir="wav", model_dir="model", output_dir="generated_audio", seconds=1.0, lr=0.001,
                        fast=False, seed=None, batch_size=16, train_width=500, max_epoch=2000, repeat=500, no_graph=False,
                        temperature=1.0, top_k=0, top_p=1.0)
    a = cli_args.parse(["--fast", "--utterances", "3"])
    assert cli_args.utterance_prompts(a) == (3, [None, None, None])
    a = cli_args.parse(["--utterances", "3", "--prompt", "a.wav"])
    assert cli_args.utterance_prompts(a) == (3, ["a.wav"] * 3)                         # one file seeds every utterance
    a = cli_args.parse(["--prompt", "a.wav", "--prompt", "b.wav"])
    assert a.utterances is None and cli_args.utterance_prompts(a) == (2, ["a.wav", "b.wav"])
    a = cli_args.parse(["--prompt", "a.wav"])
    assert cli_args.utterance_prompts(a) == (1, ["a.wav"])
    with pytest.raises(SystemExit):                                                     # two files for three utterances
        cli_args.parse(["--utterances", "3", "--prompt", "a.wav", "--prompt", "b.wav"])
    with pytest.raises(SystemExit):
        cli_args.parse(["--utterances", "0"])
    a.utterances, a.prompt = 2, ["a.wav", "b.wav", "c.wav"]
    with pytest.raises(ValueError, match="3 --prompt files for 2 utterances"):
        cli_args.utterance_prompts(a)


def test_prompt_window_is_the_files_last_tokens_left_padded_with_silence(tmp_path):
    from scipy.io import wavfile
    params = Params(SMALL)
    iw = input_width_of(params)
    assert iw == (2 ** 3 - 1) * 2 + 1 + 1
    rs = np.random.RandomState(3)
    for name, n in (("short", iw - 5), ("long", 3 * iw + 1)):
        pcm = rs.randint(-20000, 20000, n).astype(np.int16)
        pcm[0] = pcm[-2:] = 12000                                   # loud ends: trim_silence keeps all but the reference's last
        path = str(tmp_path / (name + ".wav"))
        wavfile.write(path, 8000, pcm)
        tokens = np.asarray(data.load_audio_file(path, quantization_steps=256)[0], dtype=np.int32)   # as training reads it
        assert abs(tokens.size - n) <= 1
        win = cli_generate.read_prompt(path, params)
        assert win.shape == (iw,) and win.dtype == np.int32
        if name == "short":
            pad = iw - tokens.size
            assert pad > 0 and (win[:pad] == 127).all()
            np.testing.assert_array_equal(win[pad:], tokens)
        else:
            np.testing.assert_array_equal(win, tokens[-iw:])
        np.testing.assert_array_equal(tokens[:8], data.mulaw_encode(pcm[:8].astype(float) / 32768.0, 256))


def test_generate_batch_refuses_malformed_prompts_before_any_device_work():
    """A model that was never moved to the GPU: anything past the argument checks would fail for another reason."""
    net = FasterWaveNet(Params(SMALL), seed=0)
    iw = net.input_width
    u = np.zeros((3, 5)) + 0.5
    bad = {
        "ragged": [[1, 2, 3], [4, 5]],
        "3-D": np.zeros((3, 2, iw), np.int32),
        "wrong N": np.zeros((2, iw), np.int32),
        "not integers": np.zeros((3, iw), np.float32),
        "outside [0, Q)": np.full((3, iw), 256, np.int32),
        "empty": np.zeros((3, 0), np.int32),
    }
    for what, tokens in bad.items():
        with pytest.raises(Exception, match="initial_tokens"):
            net.generate_batch(5, u, initial_tokens=tokens)
    # equal rows share a window; the order of first appearance is kept
    rows = np.arange(4 * iw, dtype=np.int32).reshape(4, iw) % 256
    rows[3] = rows[0]
    prompts, which = net._batch_prompts(rows, 4)
    assert which == [0, 1, 2, 0] and len(prompts) == 3 and all(p.dtype == np.int32 for p in prompts)
    prompts, which = net._batch_prompts(None, 2)
    assert which == [0, 0] and (prompts[0] == 127).all() and prompts[0].shape == (iw,)
    prompts, which = net._batch_prompts(rows[1], 2)
    assert which == [0, 0] and (prompts[0] == rows[1]).all()
