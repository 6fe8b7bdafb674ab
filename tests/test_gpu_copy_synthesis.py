"""Copy synthesis on a small model: ``metrics.copy_synthesis`` with every sample given (which pins the alignment rule and the
exclusion of the window's columns) and with none, ``evaluate --copy-synthesis --json`` and ``generate --from-wav --best-of K
--rank mel``."""
import json
import math
import os

import numpy as np
import pytest
import torch

import local_cond_ref as LR
import pitch_ref as P
from gpu_util import to_np
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, data, features, metrics, sampling
from wavenet_amd.faster_wavenet import silence_window
from wavenet_amd.features import LogMel
from wavenet_amd.pitch import Pitch
from wavenet_amd.train_audio import local as cli_local

pytestmark = pytest.mark.gpu

# 2 x 3 layers of 32 channels, 8 mel channels at hop 16, window 64; at 1,600 Hz the pitch lags are 3 .. 27
SPEC = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 3, residual_num_blocks=2,
            softmax_conv_channels=[64, 256])
RATE, MELS, HOP, WIN, Q = 1600, 8, 16, 64, 256
LENGTHS = (875, 825, 500)                      # with the silent fifth cut: 700, 660 and 400 samples
KEYS = ("log_mel_distance_db", "f0_rmse_cents", "f0_gross_error", "vuv_error", "voiced_frames", "nats_per_sample")


def _signal(n, seed):
    """The pitch tests' signal without its silent tail (nothing for the loader to trim)."""
    return P.chirp_signal(n, 3, 27, seed=seed)[:n - n // 5]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """The network, its checkpoint with "mel" in local.json, three recordings (one shorter) and their tokens and features."""
    from scipy.io import wavfile
    tmp = tmp_path_factory.mktemp("copy_synthesis")
    p = R.make_params(**SPEC)
    V, _ = LR.init_local(p, feats=MELS)
    net = FasterWaveNet(Params(p), seed=0, local_channels=MELS, local_hop=HOP)
    net.load_state_dict(LR.state_dict(R.init_weights(p, 1234), V))
    net.to_gpu()
    model, wav = tmp / "model", tmp / "wav"
    model.mkdir()
    wav.mkdir()
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(SPEC, sampling_rate=RATE)))
    (model / "local.json").write_text(json.dumps({"channels": MELS, "hop": HOP, "mel": {"win": WIN}}))
    names, tokens = [], []
    for i, n in enumerate(LENGTHS):
        name = "f%d.wav" % i
        wavfile.write(str(wav / name), RATE, np.round(_signal(n, i) * 32767).astype(np.int16))
        t, rate = data.load_audio_file(str(wav / name), quantization_steps=Q)
        assert rate == RATE and n - n // 5 - 8 <= t.size <= n - n // 5          # (the loader trims a few quiet samples at most)
        names.append(name)
        tokens.append(np.asarray(t, dtype=np.int32))
    feats = [cli_local.mel_features(t, RATE, MELS, HOP, WIN, Q) for t in tokens]
    W = net.input_width
    assert W == 16
    return dict(net=net, model=model, wav=wav, names=names, tokens=tokens, feats=feats, W=W, mel=LogMel(RATE, MELS, HOP, WIN),
                pitch=Pitch(RATE, HOP, WIN), tmp=tmp)


def _uniforms(s, seed):
    rs = np.random.RandomState(seed)
    return [rs.random_sample(t.size - s["W"]) for t in s["tokens"]]


def test_with_every_sample_given_the_resynthesis_is_the_file_and_every_distance_is_zero(setup):
    s = setup
    net, W = s["net"], s["W"]
    assert (s["pitch"].tau_min, s["pitch"].tau_max) == (3, 27)
    forced = [t[W:] for t in s["tokens"]]
    u = _uniforms(s, 1)
    rows = metrics.copy_synthesis(net, s["tokens"], s["feats"], None, u, s["mel"], s["pitch"], forced=forced)
    direct = net.generate_batch([f.size for f in forced], u, initial_tokens=np.stack([t[:W] for t in s["tokens"]]),
                                local=list(s["feats"]), return_chosen=True, forced=forced)
    voiced = 0
    for r, t, ch in zip(rows, s["tokens"], direct[1]):
        assert np.array_equal(r["emitted"], t[W:]) and r["samples"] == t.size
        assert r["log_mel_distance_db"] == 0.0 and r["vuv_error"] == 0.0
        assert r["f0_rmse_cents"] == (0.0 if r["voiced_frames"] else None) and r["f0_gross_error"] == (0.0 if r["voiced_frames"] else None)
        assert r["nats_per_sample"] == sampling.chosen_nll(ch) and math.isfinite(r["nats_per_sample"])
        # the alignment rule: mel column k is compared from ceil((W + win / 2) / hop) = 3 on, pitch column k from
        # ceil((W + S / 2) / hop) = 4 on (S = 64 + 27), up to the file's last column
        cols = features.frame_count(t.size, HOP)
        assert r["mel_columns"] == cols - 3 and r["pitch_columns"] == cols - 4
        voiced += r["voiced_frames"]
    assert voiced > 0                                                        # the F0 figures were formed over something


def test_the_window_columns_are_left_out(setup):
    """Only the window differs between the two signals: every compared column is the same, the columns before are not."""
    s = setup
    t = s["tokens"][0]
    other = t.copy()
    other[:s["W"]] = (other[:s["W"]] + 97) % Q
    a, b = s["mel"].batch([t, other], Q)
    k = metrics.first_free_column(s["W"], WIN, HOP)
    assert metrics.log_mel_distance(a[:, k:], b[:, k:])[0] == 0.0 and metrics.log_mel_distance(a[:, k - 1:k], b[:, k - 1:k])[0] > 0.0
    a, b = s["pitch"].batch([t, other], Q)
    k = metrics.first_free_column(s["W"], s["pitch"].span, HOP)
    assert torch.equal(a[:, k:], b[:, k:]) and not torch.equal(a[:, :k], b[:, :k])


def test_without_given_samples_a_seed_gives_the_same_table_twice_and_the_tokens_of_a_direct_run(setup):
    s = setup
    net, W = s["net"], s["W"]
    u = _uniforms(s, 2)
    run = lambda: metrics.copy_synthesis(net, s["tokens"], s["feats"], None, u, s["mel"], s["pitch"], temperature=0.9, top_k=40)
    a, b = run(), run()
    direct = net.generate_batch([t.size - W for t in s["tokens"]], u, initial_tokens=np.stack([t[:W] for t in s["tokens"]]),
                                local=list(s["feats"]), temperature=0.9, top_k=40)
    for ra, rb, d, t in zip(a, b, direct, s["tokens"]):
        assert np.array_equal(ra["emitted"], to_np(d)) and np.array_equal(ra["emitted"], rb["emitted"])
        assert not np.array_equal(ra["emitted"], t[W:])
        for k in KEYS:
            assert ra[k] == rb[k] and (ra[k] is None or math.isfinite(ra[k])), k
        assert ra["log_mel_distance_db"] > 0.0
    print({k: [r[k] for r in a] for k in KEYS})


def test_evaluate_copy_synthesis_writes_the_table_and_its_column_weighted_total(setup, tmp_path):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    s = setup
    out = tmp_path / "table.json"
    table = cli_evaluate.main(["-w", str(s["wav"]), "-m", str(s["model"]), "--copy-synthesis", "--seed", "3", "--json", str(out)])
    assert json.loads(out.read_text()) == table and sorted(table) == ["files", "total"]
    assert [r["file"] for r in table["files"]] == s["names"]
    for r, t in zip(table["files"], s["tokens"]):
        assert list(r) == ["file", "samples"] + list(KEYS) and r["samples"] == t.size
    assert list(table["total"]) == ["samples"] + list(KEYS) and table["total"]["samples"] == sum(t.size for t in s["tokens"])
    # the same run through the function: the seed, then every file's uniforms in order
    np.random.seed(3)
    u = [np.random.random_sample(t.size - s["W"]) for t in s["tokens"]]
    want = metrics.copy_synthesis(s["net"], s["tokens"], s["feats"], None, u, s["mel"], s["pitch"])
    for r, w in zip(table["files"], want):
        assert all(r[k] == w[k] for k in KEYS)
    mel_cols = [features.frame_count(t.size, HOP) - 3 for t in s["tokens"]]
    pit_cols = [features.frame_count(t.size, HOP) - 4 for t in s["tokens"]]
    rows = table["files"]
    assert abs(table["total"]["log_mel_distance_db"] - sum(r["log_mel_distance_db"] * c for r, c in zip(rows, mel_cols)) / sum(mel_cols)) < 1e-9
    assert abs(table["total"]["vuv_error"] - sum(r["vuv_error"] * c for r, c in zip(rows, pit_cols)) / sum(pit_cols)) < 1e-9
    assert table["total"]["voiced_frames"] == sum(r["voiced_frames"] for r in rows)
    # --seconds caps every file
    capped = cli_evaluate.main(["-w", str(s["wav"]), "-m", str(s["model"]), "--copy-synthesis", "--seed", "3", "--seconds", "0.15"])
    assert [r["samples"] for r in capped["files"]] == [240, 240, 240]
    # a checkpoint without "mel" stops with its message
    bare = tmp_path / "bare"
    bare.mkdir()
    (bare / "wavenet.json").write_text((s["model"] / "wavenet.json").read_text())
    (bare / "local.json").write_text(json.dumps({"channels": MELS, "hop": HOP}))
    with pytest.raises(SystemExit, match="--copy-synthesis .* needs the mel parameters .* has no \"mel\""):
        cli_evaluate.main(["-w", str(s["wav"]), "-m", str(bare), "--copy-synthesis"])


def test_generate_rank_mel_writes_the_candidate_closest_to_the_recording_and_rank_likelihood_todays_bytes(setup, tmp_path):
    from wavenet_amd.train_audio import generate as cli_generate
    s = setup
    net, W = s["net"], s["W"]
    f_wav, cols = str(s["wav"] / s["names"][2]), s["feats"][2]
    base = ["-m", str(s["model"]), "--fast", "--seed", "5", "--from-wav", f_wav, "--best-of", "3"]

    def run(name, extra):
        out = tmp_path / name
        fn, tokens = cli_generate.main(base + ["-o", str(out), "--report", str(out) + ".json"] + extra)
        return open(fn, "rb").read(), np.asarray(tokens), json.loads(open(str(out) + ".json").read())

    # the three candidates of a direct run with the same seed
    n = cols.shape[1] * HOP - W + 1
    np.random.seed(5)
    u = np.random.random_sample((3, n))
    silence = silence_window(Q, W)
    rows, chosen = net.generate_batch(n, u, initial_tokens=silence, local=cols, return_chosen=True)
    rows = to_np(rows)
    got = s["mel"].batch([np.concatenate([silence, r]).astype(np.int32) for r in rows], Q)
    k0 = metrics.first_free_column(W, WIN, HOP)
    dist = []
    for g in got:
        m = min(g.shape[1], cols.shape[1])
        dist.append(metrics.log_mel_distance(cols[:, k0:m], g[:, k0:m])[0])
    nlls = [sampling.chosen_nll(c) for c in chosen]
    print("distances", dist, "nats", nlls)
    assert len(set(dist)) == 3 and all(d > 0 for d in dist)

    mel_bytes, mel_tokens, mel_report = run("mel", ["--rank", "mel"])
    best = int(np.argmin(dist))
    assert np.array_equal(mel_tokens, rows[best])
    assert mel_report["rank"] == "mel" and mel_report["files"][0]["kept"] == best
    assert mel_report["files"][0]["log_mel_distance_db"] == dist[best] and mel_report["files"][0]["candidates"] == nlls
    like_bytes, like_tokens, like_report = run("like", ["--rank", "likelihood"])
    none_bytes, none_tokens, none_report = run("none", [])
    assert like_bytes == none_bytes and like_report == none_report and "rank" not in none_report
    assert "log_mel_distance_db" not in none_report["files"][0]
    assert np.array_equal(none_tokens, rows[sampling.pick_best(nlls)])
    data.save_audio_file(str(tmp_path / "want.wav"), rows[best], Q, format="16bit_pcm", sampling_rate=RATE)
    assert mel_bytes == open(str(tmp_path / "want.wav"), "rb").read()
