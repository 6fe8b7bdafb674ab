"""Given samples in the decode loop without a GPU: the descriptor flag in the header and the binding (and an ABI that did not
move), ``sampling.check_forced`` and ``sampling.draw_or_keep``, ``keep_mask``, and the command line's refusals -- all of them before
a model is built."""
import os
import re

import numpy as np
import pytest

from oracle import wavenet_ref as R
from wavenet_amd import _lib, data, sampling
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def test_the_header_defines_the_bit_as_512_and_the_abi_did_not_move():
    hdr = _header()
    assert re.findall(r"^#define\s+WN_DECODER_FORCED_TOKENS\s+(\d+)u", hdr, flags=re.M) == ["512"]
    assert _lib.WN_DECODER_FORCED_TOKENS == 512
    others = {k: v for k, v in vars(_lib).items() if re.match(r"WN_(EXEC|DECODER)_", k) and k not in
              ("WN_DECODER_FORCED_TOKENS", "WN_DECODER_BATCH_MAX_ANY")}
    assert others and all(isinstance(v, int) and not (v & 512) for v in others.values()), others
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 69
    assert _lib.ABI_VERSION == 5 == int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1))


def test_check_forced_accepts_and_refuses():
    Q = 256
    got = sampling.check_forced([-1, 0, 255, 7], 4, Q)
    assert got.dtype == np.int32 and got.tolist() == [-1, 0, 255, 7] and got.flags["C_CONTIGUOUS"]
    assert sampling.check_forced(np.array([3, -1], dtype=np.int64), 2, Q).dtype == np.int32
    assert sampling.check_forced(np.array([3, 200], dtype=np.uint8), 2, Q).tolist() == [3, 200]
    assert sampling.check_forced(np.zeros((0,), np.int32), 0, Q).shape == (0,)
    with pytest.raises(ValueError, match=r"forced\[2\] = 256"):
        sampling.check_forced([0, -1, 256, 300], 4, Q)
    with pytest.raises(ValueError, match=r"forced\[1\] = -2"):
        sampling.check_forced([0, -2, -7], 3, Q)
    with pytest.raises(ValueError, match=r"forced\[0\] = 4294967295"):                 # no wrap-around into -1
        sampling.check_forced(np.array([2 ** 32 - 1], dtype=np.int64), 1, Q)
    with pytest.raises(ValueError, match="n_samples = 5"):
        sampling.check_forced([1, 2, 3], 5, Q)
    with pytest.raises(ValueError, match="1-D"):
        sampling.check_forced(np.zeros((2, 3), np.int32), 6, Q)
    with pytest.raises(ValueError, match="integers"):
        sampling.check_forced(np.array([1.0, -1.0]), 2, Q)
    with pytest.raises(ValueError, match="integers"):
        sampling.check_forced(np.array([True, False]), 2, Q)


def test_draw_or_keep_is_the_given_token_or_the_existing_draw():
    rs = np.random.RandomState(3)
    for _ in range(20):
        p = rs.dirichlet(np.ones(16)).astype(np.float32)
        u = rs.random_sample()
        assert sampling.draw_or_keep(p, u, -1) == R.choice_from_uniform(p, u) == sampling.sample(p, u)
        assert sampling.draw_or_keep(p, u, -1, 0.7, 3, 0.8) == sampling.sample(p, u, 3, 0.8) == \
            R.choice_from_uniform(sampling.filter_probs(p, 3, 0.8), u)
        f = int(rs.randint(0, 16))
        assert sampling.draw_or_keep(p, u, f) == f == sampling.draw_or_keep(p, float("nan"), f, 0.7, 3, 0.8)
    # a given token the filter would have excluded is emitted all the same
    p = np.array([0.7, 0.2, 0.1], dtype=np.float32)
    assert sampling.filter_probs(p, 1)[2] == 0.0 and sampling.draw_or_keep(p, 0.5, 2, top_k=1) == 2
    with pytest.raises(ValueError):
        sampling.draw_or_keep(p, 0.5, 3)
    with pytest.raises(ValueError):
        sampling.draw_or_keep(p, 0.5, -2)


def test_keep_mask_on_ranges_that_touch_the_window_the_end_and_each_other():
    M, W, sr = 50, 10, 100.0
    assert cli_generate.keep_mask(M, W, [], sr).tolist() == [0] * 40
    t = cli_generate.keep_mask(M, W, [(0.10, 0.12)], sr)                       # starts exactly behind the window
    assert t.dtype == np.int32 and t.shape == (40,) and t.tolist() == [-1, -1] + [0] * 38
    with pytest.raises(SystemExit, match=r"0\.100000 s"):                      # one sample earlier: inside the window
        cli_generate.keep_mask(M, W, [(0.09, 0.12)], sr)
    t = cli_generate.keep_mask(M, W, [(0.45, 0.80)], sr)                       # cut off at the end of the file
    assert t.tolist() == [0] * 35 + [-1] * 5
    assert cli_generate.keep_mask(M, W, [(0.60, 0.80)], sr).tolist() == [0] * 40      # wholly behind the end: nothing
    t = cli_generate.keep_mask(M, W, [(0.20, 0.25), (0.25, 0.30), (0.28, 0.33)], sr)  # touching and overlapping
    assert t.tolist() == [0] * 10 + [-1] * 13 + [0] * 17
    t = cli_generate.keep_mask(M, W, [(0.104, 0.116)], sr)                     # rounded to samples: [10, 12)
    assert t.tolist() == [-1, -1] + [0] * 38
    assert cli_generate.keep_mask(11, 10, [], sr).shape == (1,)


def test_redraw_ranges_parse_or_stop():
    assert cli_generate.parse_redraw("0.5:1.25") == (0.5, 1.25)
    for bad in ("", "1", "1:2:3", "a:b", "1:", ":2", "-1:2", "nan:2", "1:inf"):
        with pytest.raises(SystemExit, match="A:B"):
            cli_generate.parse_redraw(bad)
    for empty in ("2:2", "3:1"):
        with pytest.raises(SystemExit, match="A < B"):
            cli_generate.parse_redraw(empty)


def _wav(path, n, Q=256, sr=100):
    tokens = (np.arange(n) * 7 % 200 + 20).astype(np.int32)
    data.save_audio_file(str(path), tokens, Q, format="16bit_pcm", sampling_rate=sr)
    return str(path)


def test_the_command_line_refuses_before_a_model_is_built(tmp_path, monkeypatch):
    def no_model(*a, **kw):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli_generate._model, "build", no_model)
    m = str(tmp_path / "model")
    wav = _wav(tmp_path / "a.wav", 64)
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(["-m", m, "--keep", wav])
    with pytest.raises(SystemExit, match="give --keep"):
        cli_generate.main(["-m", m, "--fast", "--redraw", "0.1:0.2"])
    for extra in (["--prompt", wav], ["-s", "1"], ["--seconds", "2.5"], ["--local-dir", str(tmp_path)]):
        with pytest.raises(SystemExit, match="do not go with it"):
            cli_generate.main(["-m", m, "--fast", "--keep", wav] + extra)
    for bad, what in (("0.3", "A:B"), ("0.2:0.2", "A < B"), ("0.5:0.1", "A < B"), ("x:y", "A:B")):
        with pytest.raises(SystemExit, match=what):
            cli_generate.main(["-m", m, "--fast", "--keep", wav, "--redraw", bad])
    with pytest.raises(SystemExit):                                           # three files for two utterances
        cli_generate.main(["-m", m, "--fast", "--utterances", "2", "--keep", wav, "--keep", wav, "--keep", wav])
    assert not os.path.exists(m)

    # what depends on the file and the checkpoint's shape: stopped behind load_params, still before a model is built
    class _P(object):
        quantization_steps, sampling_rate = 256, 100
    monkeypatch.setattr(cli_generate._model, "load_params", lambda d: _P())
    monkeypatch.setattr(cli_generate, "input_width_of", lambda p: 20)
    M = len(data.load_audio_file(wav, quantization_steps=256)[0])
    assert M > 22
    with pytest.raises(SystemExit, match=r"0\.200000 s"):
        cli_generate.main(["-m", m, "--fast", "--keep", wav, "--redraw", "0.1:0.4"])
    short = _wav(tmp_path / "short.wav", 21)
    Ms = len(data.load_audio_file(short, quantization_steps=256)[0])
    assert Ms < 22
    with pytest.raises(SystemExit, match=r"holds %d samples.*22 are needed" % Ms):
        cli_generate.main(["-m", m, "--fast", "--keep", short])
    # ... and a good command line gets as far as the model with the job laid out
    files, tokens, forced, single = cli_generate.keep_job(
        cli_args.parse(["-m", m, "--fast", "--keep", wav, "--redraw", "0.3:0.35", "--redraw", "0.5:9"]), False)
    assert single and files == [wav] and len(tokens[0]) == M and forced[0].shape == (M - 20,)
    want = tokens[0][20:].copy()
    want[10:15] = -1
    want[30:] = -1
    assert np.array_equal(forced[0], want) and (forced[0][:10] >= 0).all()
    with pytest.raises(AssertionError, match="the model was built"):
        cli_generate.main(["-m", m, "--fast", "--keep", wav, "--redraw", "0.3:0.35"])


def test_a_command_line_without_the_new_flags_parses_as_before():
    for argv in ([], ["--fast", "--best-of", "4", "--report", "r.json"], ["--utterances", "3", "--prompt", "p.wav", "-s", "2"],
                 ["--fast", "--local", "a.npy", "--speaker", "p225"]):
        a = cli_args.parse(argv)
        assert a.keep is None and a.redraw is None and "keep" not in vars(a) and "redraw" not in vars(a)
        # the namespace is what a parser without the two flags gives
        ap = cli_args.build_parser()
        ap._actions = [x for x in ap._actions if x.dest not in ("keep", "redraw")]
        for x in list(ap._option_string_actions):
            if x in ("--keep", "--redraw"):
                del ap._option_string_actions[x]
        assert vars(ap.parse_args(argv, namespace=cli_args.Args())) == vars(a)
    a = cli_args.parse(["--fast", "--keep", "a.wav", "--keep", "b.wav", "--redraw", "1:2", "--redraw", "3:4"])
    assert a.keep == ["a.wav", "b.wav"] and a.redraw == ["1:2", "3:4"]
    assert cli_args.kept_files(a) == (2, ["a.wav", "b.wav"]) and cli_args.utterance_count(a) == 2
    a = cli_args.parse(["--fast", "--utterances", "3", "--keep", "a.wav", "--local", "x.npy", "--local", "y.npy", "--local", "z.npy"])
    assert cli_args.kept_files(a) == (3, ["a.wav"] * 3)
    text = " ".join(cli_args.build_parser().format_help().split())
    assert "--keep" in text and "--redraw" in text and "how the real audio continues" in text
