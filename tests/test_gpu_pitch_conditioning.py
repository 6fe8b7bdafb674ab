"""Pitch as conditioning channels on the device: ``Pitch.stream`` and ``Pitch.channels``, ``acoustic.MelPitch`` against its two
analysers (bit for bit) and against the float64 definition, and the command lines -- train, features, evaluate, generate -- on a
checkpoint whose local.json has "pitch"."""
import argparse
import json
import math

import numpy as np
import pytest
import torch

import logmel_ref as L
import pitch_cond_ref as PC
import pitch_ref as P
from gpu_util import to_np
from test_gpu_logmel import _train
from wavenet_amd import acoustic, data, features, pitch

pytestmark = pytest.mark.gpu
CHUNKINGS = ["1", "7", "hop", "3hops+5", "all"]

_REF = {}


def ref():
    """Computed once and left unchanged: the signals (float32), the analysers, and the one-shot outputs of each signal."""
    if not _REF:
        sig = {k: v.astype(np.float32) for k, v in PC.signals().items()}
        both = acoustic.MelPitch(PC.RATE, PC.MELS, PC.HOP, PC.WIN, PC.FMIN, PC.FMAX, PC.THRESHOLD)
        assert (both.pitch.tau_min, both.pitch.tau_max, both.pitch.span) == (PC.TAU_MIN, PC.TAU_MAX, PC.SPAN)
        tok = torch.as_tensor(data.mulaw_encode(PC.signals()["late"], 256)).cuda()
        _REF.update(sig=sig, both=both, mel=both.mel, pitch=both.pitch, tok=tok, tok_rows=both.pitch(tok, 256), tok_out=both(tok, 256),
                    rows={k: both.pitch(x) for k, x in sig.items()}, out={k: both(x) for k, x in sig.items()})
    return _REF


def feed_all(stream, x, sizes, count_of):
    cols, fed = [], 0
    for size in sizes:
        cols.append(stream.feed(x[fed:fed + size]))
        fed += size
        assert sum(c.shape[1] for c in cols) == count_of(fed, False)
    cols.append(stream.flush())
    assert fed == len(x) and sum(c.shape[1] for c in cols) == count_of(fed, True)
    return torch.cat(cols, dim=1)


# ---- Pitch.stream, Pitch.channels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunking", CHUNKINGS)
def test_the_pitch_stream_is_the_one_shot_call_whatever_the_chunking_from_floats_and_from_tokens(chunking):
    r = ref()
    p = r["pitch"]
    count = lambda fed, final: pitch.pitch_stream_frames(fed, PC.HOP, PC.SPAN, final)
    for name in ("late", "tone"):
        x = r["sig"][name]
        got = feed_all(p.stream(), x, PC.chunkings(x.size)[chunking], count)
        assert torch.equal(got, r["rows"][name]), name
    tok = r["tok"]
    assert torch.equal(r["tok_rows"], p(data.mulaw_decode_device(tok, 256)))   # tokens and their decoded floats: the same bits
    got = feed_all(p.stream(256), tok, PC.chunkings(tok.numel())[chunking], count)
    assert torch.equal(got, r["tok_rows"])
    assert int((got[0] > 0).sum()) >= 20 and int((got[0] == 0).sum()) >= 20


def test_the_channel_map_on_the_devices_own_rows_against_the_definition():
    """Rows 0 and 2 are exact; row 1 is within max(4 x |float32 numpy restatement - definition|, 16 float32 spacings at 1.0)."""
    r = ref()
    p = r["pitch"]
    for name, rows in r["rows"].items():
        got = to_np(p.channels(rows))
        rows = to_np(rows)
        want = pitch.pitch_channels(rows, PC.FMIN, PC.FMAX)
        assert got.shape == want.shape == (3, rows.shape[1]) and got.dtype == np.float32
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2].astype(np.float64), want[2])
        ref_err = float(np.abs(PC.channels_f32(rows, PC.FMIN, PC.FMAX)[1].astype(np.float64) - want[1]).max())
        bar = max(4.0 * ref_err, 16 * PC.SPACING)
        err = float(np.abs(got[1].astype(np.float64) - want[1]).max())
        print("channels of %s: device %.3g, float32 restatement %.3g, bar %.3g" % (name, err, ref_err, bar))
        assert err <= bar, (name, err, bar)
        assert (got[1][rows[0] == 0] == 0).all()
    # a column's bits depend on its own column: a slice of the rows gives that slice
    rows = r["rows"]["late"]
    assert torch.equal(p.channels(rows[:, 70:90].contiguous()), p.channels(rows)[:, 70:90])


# ---- MelPitch ---------------------------------------------------------------------------------------------------------------------------------
def test_mel_pitch_is_the_concatenation_of_its_analysers_in_every_form_of_the_call():
    r = ref()
    both, mel, p = r["both"], r["mel"], r["pitch"]
    for name, x in r["sig"].items():
        assert torch.equal(r["out"][name], torch.cat([mel(x), p.channels(p(x))])), name
        assert r["out"][name].shape == (PC.MELS + 3, features.frame_count(x.size, PC.HOP))
    clips = [r["sig"]["late"], r["sig"]["tone"], r["sig"]["noise"]]          # 2,000, 700 and 1,001 samples
    before = (mel.launches, p.launches)
    outs = both.batch(clips)
    assert (mel.launches, p.launches) == (before[0] + 1, before[1] + 1)
    for o, name in zip(outs, ("late", "tone", "noise")):
        assert torch.equal(o, r["out"][name]), name
    full, total = r["out"]["late"], r["out"]["late"].shape[1]
    for a, b in [(0, 3), (60, 79), (total - 3, total)]:
        assert torch.equal(both.frames(r["sig"]["late"], a, b - a), full[:, a:b])
    assert torch.equal(r["tok_out"], both(data.mulaw_decode_device(r["tok"], 256)))       # tokens = floats
    assert torch.equal(r["tok_out"], torch.cat([mel(r["tok"], 256), p.channels(r["tok_rows"])]))
    with pytest.raises(ValueError, match="LogMel: a clip of 32 samples"):
        both(r["sig"]["tone"][:32])


@pytest.mark.parametrize("chunking", CHUNKINGS)
def test_the_joint_stream_is_the_one_shot_call_whatever_the_chunking(chunking):
    r = ref()
    count = lambda fed, final: acoustic.mel_pitch_stream_frames(fed, PC.HOP, PC.WIN, PC.SPAN, final)
    for name in ("late", "noise"):
        x = r["sig"][name]
        got = feed_all(r["both"].stream(), x, PC.chunkings(x.size)[chunking], count)
        assert torch.equal(got, r["out"][name]), name
    tok = r["tok"]
    assert torch.equal(feed_all(r["both"].stream(256), tok, PC.chunkings(tok.numel())[chunking], count), r["tok_out"])


@pytest.mark.parametrize("name", ["tone", "noise", "silence", "late"])
def test_mel_pitch_against_the_float64_definition(name):
    """The mel rows hold the log-mel test's bar (4 x the float32 restatement's error, at least 16 spacings at the floor).  The
    pitch rows hold the pitch test's end-to-end rule: at most 1 frame in 50 decides voicing or the lag otherwise; on the others
    F0 is within ``pitch_ref.f0_bar``, carried through the map (d lf / d f0 = 1 / (f0 ln 2 log2(fmax / fmin))) plus the map's
    own float32 bar, and the aperiodicity within the curve's bar."""
    r = ref()
    x, got = r["sig"][name], to_np(r["out"][name])
    want = acoustic.mel_pitch(x, PC.RATE, PC.MELS, PC.HOP, PC.WIN, PC.FMIN, PC.FMAX, PC.THRESHOLD)
    assert got.shape == want.shape and np.isfinite(got).all()
    F = PC.MELS
    mel64 = features.log_mel(x, PC.RATE, F, PC.HOP, PC.WIN)
    assert np.array_equal(want[:F], mel64.astype(np.float64))
    ref_err = float(np.abs(L.log_mel_f32(x, PC.RATE, F, PC.HOP, PC.WIN).astype(np.float64) - mel64).max())
    mel_bar = max(4.0 * ref_err, 16 * L.FLOOR_SPACING)
    mel_err = float(np.abs(got[:F].astype(np.float64) - want[:F]).max())
    print("%s: mel rows device %.3g, float32 restatement %.3g, bar %.3g" % (name, mel_err, ref_err, mel_bar))
    assert mel_err <= mel_bar, (mel_err, mel_bar)
    # the pitch rows
    out, curve = r["pitch"].analyse(x)
    assert torch.equal(out, r["rows"][name])
    out, curve = to_np(out), to_np(curve)
    c64 = pitch.yin_curve_lags(x, PC.HOP, PC.WIN, PC.TAU_MAX)
    t64, o64 = pitch.yin_select(c64, PC.TAU_MIN, PC.THRESHOLD, PC.RATE)
    tdev, _ = pitch.yin_select(curve, PC.TAU_MIN, PC.THRESHOLD, PC.RATE, np.float32)
    flips = (tdev != t64) | ((out[0] > 0) != (o64[0] > 0))
    print("%s: %d of %d frames decide otherwise than the definition" % (name, flips.sum(), flips.size))
    assert 50 * int(flips.sum()) <= flips.size
    keep = ~flips
    assert np.array_equal(got[F, keep], want[F, keep])                       # voiced
    fbar, _, _ = P.f0_bar(curve, PC.TAU_MIN, PC.RATE)
    chan_ref = float(np.abs(PC.channels_f32(out, PC.FMIN, PC.FMAX)[1].astype(np.float64)
                            - pitch.pitch_channels(out, PC.FMIN, PC.FMAX)[1]).max())
    chan_bar = max(4.0 * chan_ref, 16 * PC.SPACING)
    k = np.flatnonzero(keep & (o64[0] > 0))
    if k.size:
        slope = 1.0 / (np.minimum(out[0, k].astype(np.float64), o64[0, k]) * math.log(2.0) * math.log2(PC.FMAX / PC.FMIN))
        err = np.abs(got[F + 1, k].astype(np.float64) - want[F + 1, k])
        print("%s: log-F0 largest error %.3g over %d voiced frames, largest error / bar %.3g"
              % (name, err.max(), k.size, (err / (fbar[k] * slope + chan_bar)).max()))
        assert (err <= fbar[k] * slope + chan_bar).all()
    assert (got[F + 1, keep & (o64[0] == 0)] == 0).all()
    curve_bar, _ = P.bar(x, PC.HOP, PC.WIN, PC.TAU_MAX)
    assert np.abs(got[F + 2, keep].astype(np.float64) - want[F + 2, keep]).max() <= curve_bar       # (min(., 1) widens nothing)
    if name in ("tone", "late"):
        assert k.size >= 20


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
# the tiny model of tests/test_gpu_logmel.py's command-line tests (8,000 Hz, two layers of 32 channels), 8 mels at hop 16 and window
# 64; F0 between 200 and 2,000 Hz: lags 4 .. 40 again, and fmax / fmin = 10
MEL = ["--mels", "8", "--win", "64", "--local-hop", "16"]
F0 = ["--f0-min", "200", "--f0-max", "2000"]
BAND = {"fmin": 200.0, "fmax": 2000.0, "threshold": 0.15}
F = 8


def _write_wav(path, n, f):
    """A harmonic tone over the first 60 %, then noise to the end (nothing for the loader to trim)."""
    from scipy.io import wavfile
    x = P.harmonic_tone(f, 8000, n)
    x[int(0.6 * n):] = 0.2 * np.random.RandomState(n).randn(n - int(0.6 * n))
    wavfile.write(str(path), 8000, np.round(np.clip(x, -1.0, 1.0) * 32767).astype(np.int16))


@pytest.fixture(scope="module")
def audio(tmp_path_factory):
    """Two wav files, their (F + 3, frames) files from ``features --device --pitch``, and a checkpoint trained on them with
    ``train --local-mel --local-pitch``."""
    from wavenet_amd.train_audio import features as cli_features
    tmp = tmp_path_factory.mktemp("pitch_cli")
    wav = tmp / "wav"
    wav.mkdir()
    _write_wav(wav / "a.wav", 3000, 500.0)
    _write_wav(wav / "b.wav", 2200, 400.0)
    feat = tmp / "feat"
    cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "16", "--mels", "8", "--win", "64", "--device", "--pitch"] + F0)
    model, weights = _train(tmp, "model_pitch", wav, ["--local-mel", "--local-pitch"] + MEL + F0)
    return dict(tmp=tmp, wav=wav, feat=feat, model=model, weights=weights)


def test_features_pitch_writes_mel_pitch_columns_on_the_device_and_the_definition_on_the_host(audio, tmp_path):
    from wavenet_amd.train_audio import features as cli_features
    from wavenet_amd.train_audio import local as cli_local
    cli_features.main(["-w", str(audio["wav"]), "-o", str(tmp_path / "host"), "--hop", "16", "--mels", "8", "--win", "64", "--pitch"] + F0)
    for name in ("a", "b"):
        tok, rate = data.load_audio_file(str(audio["wav"] / (name + ".wav")))
        got = np.load(str(audio["feat"] / (name + ".npy")))
        both = acoustic.MelPitch(rate, 8, 16, 64, 200.0, 2000.0, 0.15)
        assert got.dtype == np.float32 and got.shape == (F + 3, features.frame_count(tok.size, 16))
        assert np.array_equal(got.view(np.uint32), to_np(both(tok, 256)).view(np.uint32))
        assert np.array_equal(got.view(np.uint32), cli_local.mel_features(tok, rate, F + 3, 16, 64, 256, pitch=BAND).view(np.uint32))
        assert 10 <= got[F].sum() <= got.shape[1] - 10                       # voiced and unvoiced columns
        host = np.load(str(tmp_path / "host" / (name + ".npy")))
        want = acoustic.mel_pitch(data.mulaw_decode(tok, 256), rate, 8, 16, 64, 200.0, 2000.0, 0.15)
        assert host.dtype == np.float32 and np.array_equal(host, want.astype(np.float32))
    assert json.loads((audio["model"] / "local.json").read_text()) == {"channels": F + 3, "hop": 16, "mel": {"win": 64}, "pitch": BAND}


@pytest.mark.parametrize("extra", [[], ["--corpus", "--local-crop", "sample"]], ids=["per-file", "corpus-sample"])
def test_training_from_audio_ends_with_the_weights_of_training_from_its_feature_files(audio, tmp_path, extra):
    if extra:
        model_a, wa = _train(tmp_path, "a", audio["wav"], ["--local-mel", "--local-pitch"] + MEL + F0 + extra)
    else:
        model_a, wa = audio["model"], audio["weights"]
    model_b, wb = _train(tmp_path, "b", audio["wav"], ["--local-dir", str(audio["feat"]), "--local-hop", "16"] + extra)
    assert sorted(wa) == sorted(wb) and wa["local_condition_projection/W"].shape[1] == F + 3
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    ja, jb = json.loads((model_a / "local.json").read_text()), json.loads((model_b / "local.json").read_text())
    assert ja.pop("mel") == {"win": 64} and ja.pop("pitch") == BAND and ja == jb == {"channels": F + 3, "hop": 16}


def test_scoring_from_audio_is_scoring_under_the_files_features(audio):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    got = cli_evaluate.main(["-w", str(audio["wav"]), "-m", str(audio["model"]), "--local-mel"])
    want = cli_evaluate.main(["-w", str(audio["wav"]), "-m", str(audio["model"]), "--local-dir", str(audio["feat"])])
    assert got == want and len(got["files"]) == 2 and got["total"]["samples"] > 0


def test_copy_synthesis_streams_the_recordings_mel_and_pitch_columns_and_f0_scale_moves_the_voiced_ones(audio, tmp_path, monkeypatch):
    from wavenet_amd.train_audio import generate as cli_generate
    f_wav, f_npy, model = str(audio["wav"] / "a.wav"), str(audio["feat"] / "a.npy"), str(audio["model"])
    cols = np.load(f_npy)

    def run(name, extra):
        out = tmp_path / name
        cli_generate.main(["-m", model, "-o", str(out), "--fast", "--seed", "3", "-s", "0.02"] + extra)
        return (out / "generated.wav").read_bytes()

    want = run("npy", ["--local", f_npy])
    assert run("wav", ["--from-wav", f_wav]) == want
    assert run("one_push", ["--from-wav", f_wav, "--chunk-frames", str(cols.shape[1])]) == want
    assert run("scale_1", ["--from-wav", f_wav, "--f0-scale", "1.0"]) == want
    assert run("scale_1_npy", ["--local", f_npy, "--f0-scale", "1.0"]) == want
    # C = 2: the columns the streamed source hands out are the one-shot array's
    taken = []
    take = cli_generate.MelColumns.take
    monkeypatch.setattr(cli_generate.MelColumns, "take", lambda self, k, host=False: taken.append(to_np(take(self, k))) or (
        taken[-1] if host else torch.as_tensor(taken[-1]).cuda()))
    assert len(run("chunks", ["--from-wav", f_wav, "--chunk-frames", "2"])) == len(want)
    pushed = np.concatenate(taken, axis=1)
    assert len(taken) > 2 and pushed.shape[0] == F + 3
    assert np.array_equal(pushed.view(np.uint32), cols[:, :pushed.shape[1]].view(np.uint32))
    # --f0-scale 2: what the network is handed differs in row F + 1 of the voiced columns only, by float32(1 / log2(10))
    del taken[:]
    run("chunks_scaled", ["--from-wav", f_wav, "--chunk-frames", "2", "--f0-scale", "2.0"])
    streamed = np.concatenate(taken, axis=1)
    monkeypatch.setattr(cli_generate, "generate_audio", lambda net, params, **kw: kw["local"])
    base = cli_generate.main(["-m", model, "--fast", "--from-wav", f_wav])
    assert np.array_equal(base.view(np.uint32), cols.view(np.uint32))
    voiced = base[F] == 1
    moved = base.copy()
    moved[F + 1, voiced] = base[F + 1, voiced] + np.float32(1.0 / math.log2(10.0))
    assert 10 <= voiced.sum() <= voiced.size - 10 and not np.array_equal(moved, base)
    for source in (["--from-wav", f_wav], ["--local", f_npy]):
        got = cli_generate.main(["-m", model, "--fast", "--f0-scale", "2.0"] + source)
        assert np.array_equal(got.view(np.uint32), moved.view(np.uint32)), source
    assert np.array_equal(streamed.view(np.uint32), moved[:, :streamed.shape[1]].view(np.uint32))


def test_with_every_sample_given_copy_synthesis_on_a_pitch_checkpoint_measures_zero(audio):
    """The features the network sees (mel rows and pitch channels) and the columns the metrics compare (pure log-mel rows, pitch
    rows) sit on one grid: the resynthesis is the file, and every distance is exactly 0."""
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import model as cli_model
    params, net = cli_model.build(argparse.Namespace(model_dir=str(audio["model"]), gpu_device=0, fast=True, seed=None))
    assert net.local == (F + 3, 16) and net.local_mel == {"win": 64} and net.local_pitch == BAND
    table = cli_evaluate.copy_synthesis_dir(net, params, str(audio["wav"]), seed=1, forced=True, verbose=False)
    assert [r["file"] for r in table["files"]] == ["a.wav", "b.wav"]
    for r in table["files"] + [table["total"]]:
        assert r["log_mel_distance_db"] == 0.0 and r["vuv_error"] == 0.0
        assert r["voiced_frames"] > 0 and r["f0_rmse_cents"] == 0.0 and r["f0_gross_error"] == 0.0
        assert math.isfinite(r["nats_per_sample"])
    drawn = cli_evaluate.copy_synthesis_dir(net, params, str(audio["wav"]), seed=1, verbose=False)      # (and drawn, it is not)
    assert drawn["total"]["log_mel_distance_db"] > 0.0
