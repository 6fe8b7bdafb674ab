"""Log-mel features on the device (wn_logmel, features.LogMel) against the numpy definition, and the determinism contract: a
column's bits depend on its own samples only -- not on tile mates, batch mates, the call, the chunking, or tokens versus floats."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import logmel_ref as L
from gpu_util import to_np
from wavenet_amd import _lib, _logmel, data, features
from wavenet_amd.features import LogMel, mel_stream_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SIG = {}


def sig(n):
    if n not in _SIG:
        _SIG[n] = L.chirp_signal(n).astype(np.float32)
    return _SIG[n]


def tokens(n):
    return data.mulaw_encode(L.chirp_signal(n), 256)


def same_bits(a, b):
    a, b = [v if isinstance(v, np.ndarray) else to_np(v) for v in (a, b)]
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("win,hop,n_mels,n", L.SHAPES)
def test_every_cell_is_within_four_float32_restatement_errors_of_the_definition(win, hop, n_mels, n):
    """Bar per shape: 4 x the error of tests/logmel_ref.py (float32 sums in numpy) against features.log_mel on the same input,
    at least 16 float32 spacings at the floor.  Every cell counts, the ones on the floor included."""
    x = sig(n)
    want = features.log_mel(x, L.RATE, n_mels, hop, win)
    bar, ref_err = L.bar(x, win, hop, n_mels)
    got = to_np(LogMel(L.RATE, n_mels, hop, win)(x))
    assert got.shape == want.shape == (n_mels, features.frame_count(n, hop))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("logmel %d/%d/%d/%d: device %.3g, float32 restatement %.3g, bar %.3g" % (win, hop, n_mels, n, err, ref_err, bar))
    assert np.isfinite(got).all()
    assert err <= bar, (err, bar)


def test_the_longest_window_on_a_segment_above_the_default_lds_limit():
    """win 4096 / hop 512: K = 4096 taps, 2,049 bins, and a 32-frame segment of 97 KB -- above what a launch may ask for
    without the kernel's limit being raised, which the call then does.  Same bar as above; 40 frames, two tiles."""
    win, hop, n_mels, n = 4096, 512, 8, 20000
    x = sig(n)
    bar, ref_err = L.bar(x, win, hop, n_mels)
    got = to_np(LogMel(L.RATE, n_mels, hop, win)(x))
    err = float(np.abs(got.astype(np.float64) - features.log_mel(x, L.RATE, n_mels, hop, win)).max())
    print("logmel %d/%d/%d/%d: device %.3g, float32 restatement %.3g, bar %.3g" % (win, hop, n_mels, n, err, ref_err, bar))
    assert got.shape == (n_mels, 40) and err <= bar, (err, bar)


@pytest.mark.parametrize("win,hop,n_mels,n", [(64, 16, 8, 700), (96, 40, 13, 1001)])
def test_tokens_and_their_decoded_floats_give_the_same_bits(win, hop, n_mels, n):
    tok = torch.as_tensor(tokens(n)).cuda()
    mel = LogMel(L.RATE, n_mels, hop, win)
    assert same_bits(mel(tok, 256), mel(data.mulaw_decode_device(tok, 256)))


def test_a_batch_is_its_single_calls_and_a_column_range_is_those_columns():
    mel = LogMel(L.RATE, 8, 16, 64)
    clips = [sig(700), sig(3000), sig(1001)]
    before = mel.launches
    outs = mel.batch(clips)
    assert mel.launches == before + 1
    singles = [mel(c) for c in clips]
    for o, s in zip(outs, singles):
        assert same_bits(o, s)
    full, total = singles[1], features.frame_count(3000, 16)
    for a, b in [(0, 5), (70, 110), (total - 3, total)]:
        assert same_bits(mel.frames(clips[1], a, b - a), full[:, a:b].contiguous())


@pytest.mark.parametrize("win,hop", [(64, 16), (96, 40)])
@pytest.mark.parametrize("chunk", [1, 37, "hop", 1000, "all"])
def test_streaming_is_the_one_shot_call_whatever_the_chunking(win, hop, chunk):
    n = 1001
    x = sig(n)
    mel = LogMel(L.RATE, 8, hop, win)
    want = mel(x)
    step = {"hop": hop, "all": n}.get(chunk, chunk)
    an, cols, fed = mel.stream(), [], 0
    for at in range(0, n, step):
        part = an.feed(x[at:at + step])
        fed = min(n, at + step)
        cols.append(part)
        assert sum(c.shape[1] for c in cols) == mel_stream_frames(fed, hop, win)
        assert an.tail.numel() <= win                          # only what later columns read is kept
    cols.append(an.flush())
    assert sum(c.shape[1] for c in cols) == mel_stream_frames(n, hop, win, True) == want.shape[1]
    assert same_bits(torch.cat(cols, dim=1), want)


@pytest.mark.parametrize("kw,word", [(dict(win=63), "63"), (dict(win=8), "win = 8"), (dict(win=8192), "8192"),
                                     (dict(n_mels=300), "300")])
def test_unsupported_shapes_are_refused_by_name(kw, word):
    with pytest.raises(ValueError, match=word):
        LogMel(L.RATE, **dict(dict(n_mels=8, hop=16, win=64), **kw))


def test_a_clip_of_half_a_window_is_refused_before_device_work():
    mel = LogMel(L.RATE, 8, 16, 64)
    before = mel.launches
    with pytest.raises(ValueError, match="32 samples"):
        mel(sig(700)[:32])
    assert mel.launches == before


def test_a_frame_past_an_unflagged_edge_is_earg_through_the_raw_abi():
    mel = LogMel(L.RATE, 8, 16, 64)
    x = torch.as_tensor(sig(700)).cuda()
    out = torch.full((8, 4), 7.0, device="cuda")
    lib = _logmel.lib()

    def call(origin, first, count, flags):
        clip = _logmel.WnLogmelClip(x=x.data_ptr(), n=700, origin=origin, out=out.data_ptr(), out_stride=4, first=first, count=count,
                                 flags=flags)
        return lib.wn_logmel(C.byref(clip), 1, None, 0, _lib.ptr(mel.basis), _lib.ptr(mel.fbT), 64, 16, 8, _lib.stream_ptr())

    assert call(0, 0, 4, _logmel.WN_LOGMEL_REFLECT_RIGHT) == _logmel.WNL_EARG              # frame 0 reads sample -32
    assert b"sample -32" in lib.wn_logmel_last_error() and b"left" in lib.wn_logmel_last_error()
    assert call(0, 40, 4, _logmel.WN_LOGMEL_REFLECT_LEFT) == _logmel.WNL_EARG              # frame 43 reads sample 719 of 700
    assert b"sample 719" in lib.wn_logmel_last_error() and b"right" in lib.wn_logmel_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())                              # nothing ran
    assert call(32, 0, 4, 0) == _logmel.WNL_OK                                          # the middle of a longer signal: no flag needed
    assert same_bits(out, mel.frames(x, 2, 4))


# ---- the command line: features --device, train --local-mel, generate --from-wav, evaluate --local-mel ---------------------------
# two layers of 32 channels: the widths whose training step is bit-reproducible from run to run (below 32 channels the embedding
# gradient is summed with float atomics, and a run does not reproduce ITSELF to the last bit, whatever its features come from)
CFG = {"quantization_steps": 256, "sampling_rate": 8000, "causal_conv_channels": [32], "residual_conv_channels": [32] * 2,
       "residual_num_blocks": 1, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
MEL = ["--mels", "8", "--win", "64", "--local-hop", "16"]
LOOP = ["--seed", "1", "--lr", "0.003", "--batch-size", "2", "--train-width", "48", "--repeat", "3", "--max-epoch", "2"]


def _write_wav(path, n):
    from scipy.io import wavfile
    wavfile.write(str(path), 8000, np.round(L.chirp_signal(n)[:n - n // 5] * 32767).astype(np.int16))     # (no silent tail to trim)


def _train(tmp, name, wav, extra):
    import json
    from wavenet_amd.train_audio import train as cli_train
    model = tmp / name
    model.mkdir()
    (model / "wavenet.json").write_text(json.dumps(CFG))
    cli_train.main(["-w", str(wav), "-m", str(model)] + LOOP + extra)
    with np.load(str(model / "wavenet.model.npz")) as z:
        return model, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def audio(tmp_path_factory):
    """One wav file, its feature file from ``features --device``, and a checkpoint trained on it with ``train --local-mel``."""
    from wavenet_amd.train_audio import features as cli_features
    tmp = tmp_path_factory.mktemp("logmel_cli")
    wav = tmp / "wav"
    wav.mkdir()
    _write_wav(wav / "f.wav", 3000)
    feat = tmp / "feat"
    cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "16", "--mels", "8", "--win", "64", "--device"])
    model, weights = _train(tmp, "model_mel", wav, ["--local-mel"] + MEL)
    return dict(tmp=tmp, wav=wav, feat=feat, model=model, weights=weights)


def test_features_device_writes_the_kernels_columns_within_the_bar_of_the_numpy_files(tmp_path):
    from wavenet_amd.train_audio import features as cli_features
    wav = tmp_path / "wav"
    wav.mkdir()
    _write_wav(wav / "a.wav", 700)
    _write_wav(wav / "b.wav", 1001)
    args = ["-w", str(wav), "--hop", "16", "--mels", "8", "--win", "64"]
    cli_features.main(args + ["-o", str(tmp_path / "dev"), "--device"])
    cli_features.main(args + ["-o", str(tmp_path / "host")])
    for name in ("a", "b"):
        tok, rate = data.load_audio_file(str(wav / (name + ".wav")))
        got = np.load(str(tmp_path / "dev" / (name + ".npy")))
        assert got.dtype == np.float32 and same_bits(got, LogMel(rate, 8, 16, 64)(tok, 256))
        bar, _ = L.bar(data.mulaw_decode(tok, 256).astype(np.float32), 64, 16, 8)
        host = np.load(str(tmp_path / "host" / (name + ".npy")))
        assert np.abs(got.astype(np.float64) - host).max() <= bar


@pytest.mark.parametrize("extra", [[], ["--local-interp", "linear"], ["--local-crop", "sample"]], ids=["repeat", "linear", "sample"])
def test_training_from_audio_ends_with_the_weights_of_training_from_its_feature_files(audio, tmp_path, extra):
    import json
    if extra:
        model_a, wa = _train(tmp_path, "a", audio["wav"], ["--local-mel"] + MEL + extra)
    else:
        model_a, wa = audio["model"], audio["weights"]
    model_b, wb = _train(tmp_path, "b", audio["wav"], ["--local-dir", str(audio["feat"]), "--local-hop", "16"] + extra)
    assert sorted(wa) == sorted(wb) and "local_condition_projection/W" in wa
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    ja, jb = json.loads((model_a / "local.json").read_text()), json.loads((model_b / "local.json").read_text())
    assert ja.pop("mel") == {"win": 64} and "mel" not in jb and ja == jb


def test_copy_synthesis_is_generation_from_the_files_features(audio, tmp_path, monkeypatch):
    from wavenet_amd.train_audio import generate as cli_generate
    f_wav, f_npy, model = str(audio["wav"] / "f.wav"), str(audio["feat"] / "f.npy"), str(audio["model"])
    cols = np.load(f_npy)

    def run(name, extra):
        out = tmp_path / name
        cli_generate.main(["-m", model, "-o", str(out), "--fast", "--seed", "3", "-s", "0.02"] + extra)
        return (out / "generated.wav").read_bytes()

    want = run("npy", ["--local", f_npy])
    assert run("wav", ["--from-wav", f_wav]) == want
    assert run("one_push", ["--from-wav", f_wav, "--chunk-frames", str(cols.shape[1])]) == run("npy_push", ["--local", f_npy, "--chunk-frames", str(cols.shape[1])]) == want
    taken = []
    take = cli_generate.MelColumns.take
    monkeypatch.setattr(cli_generate.MelColumns, "take", lambda self, k, host=False: taken.append(to_np(take(self, k))) or (
        taken[-1] if host else torch.as_tensor(taken[-1]).cuda()))
    assert len(run("chunks", ["--from-wav", f_wav, "--chunk-frames", "3"])) == len(want)
    pushed = np.concatenate(taken, axis=1)
    assert len(taken) > 2 and same_bits(pushed, cols[:, :pushed.shape[1]])


def test_scoring_from_audio_is_scoring_under_the_files_features(audio):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    got = cli_evaluate.main(["-w", str(audio["wav"]), "-m", str(audio["model"]), "--local-mel"])
    want = cli_evaluate.main(["-w", str(audio["wav"]), "-m", str(audio["model"]), "--local-dir", str(audio["feat"])])
    assert got == want and got["total"]["samples"] > 0
    with pytest.raises(SystemExit, match="--local-dir FEAT_DIR or --local-mel"):
        cli_evaluate.main(["-w", str(audio["wav"]), "-m", str(audio["model"])])
