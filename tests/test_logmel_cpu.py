"""The host side of the device log-mel: the streaming arithmetic, the basis, and the refusals that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from wavenet_amd import _logmel, features
from wavenet_amd.features import mel_stream_frames


@pytest.mark.parametrize("hop,win", [(1, 16), (16, 64), (40, 96), (256, 1024), (7, 16), (100, 64)])
def test_mel_stream_frames_counts_the_columns_whose_samples_have_arrived(hop, win):
    half = win // 2
    totals = sorted({0, 1, half - 1, half, half + 1, half + hop, half + hop + 1, win, win + 1, 3 * win + 5, 5 * hop + half,
                     5 * hop + half + 1})
    for total in totals:
        # column k exists if its centre k hop is a sample, and is out once sample k hop + win / 2 has arrived
        brute = sum(1 for k in range(total + 1) if k * hop < total and k * hop + half <= total - 1)
        assert mel_stream_frames(total, hop, win) == brute, (total, hop, win)
        assert mel_stream_frames(total, hop, win, True) == sum(1 for k in range(total + 1) if k * hop < total)
        assert mel_stream_frames(total, hop, win) <= mel_stream_frames(total, hop, win, True)


@pytest.mark.parametrize("win", [16, 96, 1024])
def test_the_basis_is_the_rfft_of_a_hann_windowed_frame(win):
    frame = np.random.RandomState(win).randn(3, win)
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    want = np.fft.rfft(frame * w[None, :], axis=1)
    got = frame @ features.dft_basis(win)
    nb = win // 2 + 1
    assert got.shape == (3, 2 * nb)
    assert np.abs(got[:, :nb] - want.real).max() < 1e-12 and np.abs(got[:, nb:] - want.imag).max() < 1e-12


def test_the_tables_are_the_float64_ones_rounded_once_and_cached():
    basis, fbT = features.logmel_tables(16000, 64, 8)
    assert basis.dtype == fbT.dtype == np.float32 and basis.shape == (64, 66) and fbT.shape == (33, 8)
    assert np.array_equal(basis, features.dft_basis(64).astype(np.float32))
    assert np.array_equal(fbT, features.mel_filterbank(16000, 64, 8).T.astype(np.float32))
    assert features.logmel_tables(16000, 64, 8)[0] is basis


def test_log_mel_itself_is_unchanged():
    """Columns 0, 9 and 18 of a sine, as the numpy definition gave them before the device face was added (float64 sums: 1e-5
    is a hundred float32 spacings at these magnitudes and far below any change of the definition)."""
    x = np.sin(np.arange(300) * 0.1)
    got = features.log_mel(x, 16000, 8, 16, 64)
    assert got.shape == (8, 19) and got.dtype == np.float32
    want = np.array([[1.94180977e+00, 2.73348737e+00, 2.74792457e+00],
                     [2.14938021e+00, 2.17734289e+00, 2.16110253e+00],
                     [1.37541890e+00, -3.29226756e+00, -1.89639223e+00],
                     [5.55019915e-01, -5.06118059e+00, -2.64372969e+00],
                     [6.22434949e-04, -6.45853519e+00, -3.20817828e+00],
                     [-3.86413991e-01, -7.51662350e+00, -3.59596992e+00],
                     [-6.64790452e-01, -8.43313503e+00, -3.87521744e+00],
                     [-8.01910460e-01, -9.32627201e+00, -4.01245356e+00]])
    assert np.abs(got[:, [0, 9, 18]] - want).max() < 1e-5


def test_wn_logmel_refuses_null_and_bad_shapes_without_a_gpu():
    lib = _logmel.lib()
    assert "wn_logmel" in _logmel.EXPORTS
    assert lib.wn_logmel(None, 1, None, 0, None, None, 64, 16, 8, None) == _logmel.WNL_EARG
    assert b"NULL" in lib.wn_logmel_last_error()
    clip = _logmel.WnLogmelClip(x=64, n=700, origin=0, out=64, out_stride=4, first=0, count=4, flags=3)
    one = C.byref(clip)
    for args, word in [((63, 16, 8), b"win = 63"), ((8, 16, 8), b"win = 8"), ((8192, 16, 8), b"win = 8192"),
                       ((64, 0, 8), b"hop = 0"), ((64, 16, 300), b"n_mels = 300"), ((64, 16, 0), b"n_mels = 0"),
                       ((4096, 2048, 8), b"163840")]:
        assert lib.wn_logmel(one, 1, None, 0, 64, 64, *args, None) == _logmel.WNL_EARG, args
        assert word in lib.wn_logmel_last_error(), (args, lib.wn_logmel_last_error())
    assert lib.wn_logmel(one, 65, None, 0, 64, 64, 64, 16, 8, None) == _logmel.WNL_EARG and b"65" in lib.wn_logmel_last_error()
    clip.n = 32
    assert lib.wn_logmel(one, 1, None, 0, 64, 64, 64, 16, 8, None) == _logmel.WNL_EARG and b"32 samples" in lib.wn_logmel_last_error()
    clip.n, clip.flags = 700, 0
    assert lib.wn_logmel(one, 1, None, 0, 64, 64, 64, 16, 8, None) == _logmel.WNL_EARG and b"sample -32" in lib.wn_logmel_last_error()


def test_the_python_face_refuses_unsupported_shapes_by_name():
    for kw, word in [(dict(win=63), "win = 63"), (dict(win=8), "win = 8"), (dict(win=8192), "win = 8192"),
                     (dict(n_mels=300), "n_mels = 300"), (dict(hop=0), "hop = 0"), (dict(win=4096, hop=2048), "163840")]:
        with pytest.raises(ValueError, match=word):
            features._check_logmel_shape(**dict(dict(n_mels=8, hop=16, win=64), **kw))
    features._check_logmel_shape(None, 4096, None)              # what is not known yet is not judged
    with pytest.raises(ValueError, match="win = 63"):
        features._check_logmel_shape(None, None, 63)


# ---- the command line: flags and local.json ---------------------------------------------------------------------------------------
def _error(argv, capsys):
    from wavenet_amd.train_audio import args as cli_args
    with pytest.raises(SystemExit):
        cli_args.parse(argv)
    return capsys.readouterr().err


def test_flag_combinations_are_refused_at_parse_time(capsys):
    from wavenet_amd.train_audio import args as cli_args
    assert "--local-mel (features made from the audio) and --local-dir" in _error(["--local-mel", "--local-dir", "d"], capsys)
    assert "--mels F and --win W go with --local-mel" in _error(["--mels", "8"], capsys)
    assert "--mels F and --win W go with --local-mel" in _error(["--win", "64", "--local-dir", "d"], capsys)
    assert "win = 63" in _error(["--local-mel", "--win", "63"], capsys)
    assert "n_mels = 300" in _error(["--local-mel", "--mels", "300"], capsys)
    assert "163840" in _error(["--local-mel", "--win", "4096", "--local-hop", "2048"], capsys)
    # a value that is not given is not judged at parse time: it may come from local.json (model.build checks what is used)
    assert cli_args.parse(["--local-mel", "--local-hop", "4096"]).local_hop == 4096
    assert "--local-hop H goes with --local-dir or --local-mel" in _error(["--local-hop", "16"], capsys)
    assert "--from-wav needs --fast" in _error(["--from-wav", "f.wav"], capsys)
    for other in (["--local", "f.npy"], ["--local-dir", "d"], ["--keep", "k.wav"]):
        assert "--from-wav FILE.wav (features made from a recording) excludes " + other[0] in _error(
            ["--fast", "--from-wav", "f.wav"] + other, capsys)
    assert "2 --from-wav files for 3 utterances" in _error(["--fast", "--utterances", "3", "--from-wav", "a.wav", "--from-wav", "b.wav"],
                                                           capsys)
    a = cli_args.parse(["--local-mel", "--mels", "8", "--win", "64", "--local-hop", "16", "--local-interp", "linear", "--local-crop",
                        "sample", "--local-upsample", "2"])
    assert (a.local_mel, a.mels, a.win, a.local_hop, a.local_interp, a.local_crop, a.local_upsample) == (True, 8, 64, 16, "linear",
                                                                                                         "sample", 2)
    b = cli_args.parse([])
    assert (b.local_mel, b.mels, b.win, b.from_wav) == (False, None, None, None) and "local_mel" not in vars(b)
    assert "--local-crop {frame,sample} goes with --local-dir" in _error(["--local-crop", "sample"], capsys)


def test_generate_checks_from_wav_before_a_model_is_built(tmp_path):
    import json
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import local as cli_local
    model = tmp_path / "model"
    cli_local.ensure_config(str(model), 8, 16)                              # a checkpoint trained on feature files
    with pytest.raises(SystemExit, match="needs a checkpoint trained with train --local-mel"):
        cli_generate.main(["-m", str(model), "--fast", "--from-wav", "f.wav"])
    with pytest.raises(SystemExit, match="--chunk-frames streams the columns"):
        cli_generate.main(["-m", str(model), "--fast", "--chunk-frames", "4"])
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    with pytest.raises(SystemExit, match="--local-mel needs a checkpoint trained with train --local-mel"):
        cli_evaluate.main(["-m", str(model), "-w", str(tmp_path), "--local-mel"])
    assert json.loads((model / "local.json").read_text()) == {"channels": 8, "hop": 16}


def test_local_json_mel_round_trip_and_the_messages_on_mismatch(tmp_path):
    import json
    from wavenet_amd.train_audio import local as L
    plain, mel = str(tmp_path / "plain"), str(tmp_path / "mel")
    assert L.ensure_config(plain, 8, 16) == (8, 16)
    before = open(os.path.join(plain, "local.json"), "rb").read()
    assert before == json.dumps({"channels": 8, "hop": 16}).encode()        # byte for byte what it always was
    assert L.ensure_config(plain, 8, 16) == (8, 16) and L.load_mel(plain) is None
    assert open(os.path.join(plain, "local.json"), "rb").read() == before
    with pytest.raises(SystemExit, match=r'trained on feature files \(no "mel"\), the command line gives --local-mel --win 64'):
        L.ensure_config(plain, 8, 16, mel={"win": 64})
    assert L.ensure_config(mel, 8, 16, "linear", mel={"win": 64}) == (8, 16)
    assert json.load(open(os.path.join(mel, "local.json"))) == {"channels": 8, "hop": 16, "interp": "linear", "mel": {"win": 64}}
    assert L.load_mel(mel) == {"win": 64} and L.load_interp(mel) == "linear"
    assert L.ensure_config(mel, 8, 16, mel={"win": 64}) == (8, 16)          # resumed with the same values
    assert L.ensure_config(mel, 8, 16) == (8, 16)                           # resumed on feature files: accepted, they win
    with pytest.raises(SystemExit, match=r"trained with --local-mel --win 64, the command line gives --local-mel --win 128"):
        L.ensure_config(mel, 8, 16, mel={"win": 128})
    with pytest.raises(SystemExit, match=r"trained on 8 feature channels at hop 16, the command line gives 12 at hop 16"):
        L.ensure_config(mel, 12, 16, mel={"win": 64})
    open(os.path.join(mel, "local.json"), "w").write(json.dumps({"channels": 8, "hop": 16, "mel": 64}))
    with pytest.raises(Exception, match='"mel" must be'):
        L.load_mel(mel)
    assert L.load_mel(str(tmp_path / "none")) is None
