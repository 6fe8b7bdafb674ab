"""Pitch as conditioning channels, the parts that need no GPU: the look-ahead arithmetic of the streams, the channel map and
``scale_f0`` on values worked out by hand, the stream logic with the launches replaced by the numpy definitions, the "pitch" key
of local.json, and what the command lines parse to and refuse before a model is built."""
import json
import math

import numpy as np
import pytest
import torch

import pitch_cond_ref as PC
import pitch_ref as P
from wavenet_amd import acoustic, features, pitch
from wavenet_amd.train_audio import local as cli_local


# ---- the look-ahead arithmetic --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [1, 16, 256])
@pytest.mark.parametrize("span,win", [(104, 64), (91, 64), (21, 16)])
def test_the_stream_counts_are_a_brute_force_count_from_the_reach_formula(hop, span, win):
    for total in range(0, 3 * span + 1):
        # column k reads samples up to k hop - span // 2 + span - 1: it is out when that sample has been fed
        brute_p = sum(1 for k in range(total + 1) if k * hop - span // 2 + span - 1 <= total - 1)
        assert pitch.pitch_stream_frames(total, hop, span) == brute_p, (total, hop, span)
        assert pitch.pitch_stream_frames(total, hop, span, True) == features.frame_count(total, hop) == -(-total // hop)
        # the mel columns are held to "up to k hop + win / 2" (features.mel_stream_frames); a joint column needs both
        brute_m = sum(1 for k in range(total + 1) if k * hop + win // 2 <= total - 1)
        assert features.mel_stream_frames(total, hop, win) == brute_m
        assert acoustic.mel_pitch_stream_frames(total, hop, win, span) == min(brute_m, brute_p)
        assert acoustic.mel_pitch_stream_frames(total, hop, win, span, True) == features.frame_count(total, hop)
        assert brute_p <= brute_m                                            # the pitch look-ahead is the larger one
        assert brute_p <= features.frame_count(total, hop)


# ---- the channel map ------------------------------------------------------------------------------------------------------------------
def test_pitch_channels_on_values_worked_out_by_hand():
    assert pitch.PITCH_CHANNELS == 3
    rows = np.array([[40.0, 400.0, 0.0, 0.0, 126.49110640673517, 39.0, 410.0],
                     [0.01, 0.14, 0.5, 1.7, 0.0, 0.1, 0.1]])
    got = pitch.pitch_channels(rows, 40.0, 400.0)
    assert got.shape == (3, 7) and got.dtype == np.float64
    # fmin is 0 exactly; fmax is 1 to the roundings of the formula (log2(400) - log2(40) and log2(10) are rounded apart)
    assert got[1, 0] == 0.0 and abs(got[1, 1] - 1.0) <= 4 * 2.0 ** -52
    assert abs(got[1, 4] - 0.5) < 1e-15                                      # the geometric middle
    assert got[1, 5] < 0.0 and got[1, 6] > 1.0                               # no clamp: the value follows F0 out of the band
    assert np.array_equal(got[:, 2], [0.0, 0.0, 0.5]) and np.array_equal(got[:, 3], [0.0, 0.0, 1.0])      # unvoiced: (0, 0, min(c, 1))
    assert np.array_equal(got[0], (rows[0] > 0).astype(np.float64))
    assert np.array_equal(got[2], np.minimum(rows[1], 1.0))
    assert pitch.pitch_channels(np.zeros((2, 0)), 40.0, 400.0).shape == (3, 0)
    with pytest.raises(ValueError, match=r"pitch_channels: rows of shape \(3, 7\); it takes \(2, n\)"):
        pitch.pitch_channels(np.zeros((3, 7)), 40.0, 400.0)
    with pytest.raises(ValueError, match=r"pitch_channels: rows of shape \(7,\)"):
        pitch.pitch_channels(np.zeros(7), 40.0, 400.0)
    with pytest.raises(ValueError, match="pitch_channels: fmin = 0.0; it takes fmin > 0"):
        pitch.pitch_channels(rows, 0.0, 400.0)
    with pytest.raises(ValueError, match="pitch_channels: fmax = 40.0; it takes fmax > fmin = 40.0"):
        pitch.pitch_channels(rows, 40.0, 40.0)


def test_the_float32_constants_are_the_documented_ones():
    lo, k = pitch.channel_constants(40.0, 400.0)
    assert lo.dtype == k.dtype == np.float32
    assert lo == np.float32(math.log2(40.0)) and k == np.float32(1.0 / math.log2(10.0))


def test_the_float32_restatement_decides_voicing_as_the_definition_on_the_test_signals():
    """What the GPU test's "at most 1 frame in 50" allows for is float32 sums; on these signals the float32 restatement
    (tests/pitch_ref.py) flips no decision at all, so the allowance is not used up by the signals themselves."""
    voiced = 0
    for name, x in PC.signals().items():
        x32 = x.astype(np.float32)
        c64 = pitch.yin_curve_lags(x32, PC.HOP, PC.WIN, PC.TAU_MAX)
        t64, o64 = pitch.yin_select(c64, PC.TAU_MIN, PC.THRESHOLD, PC.RATE)
        t32, o32 = pitch.yin_select(P.yin_curve_f32(x32, PC.HOP, PC.WIN, PC.TAU_MAX), PC.TAU_MIN, PC.THRESHOLD, PC.RATE, np.float32)
        flips = (t32 != t64) | ((o32[0] > 0) != (o64[0] > 0))
        assert not flips.any(), (name, np.flatnonzero(flips))
        voiced += int((o64[0] > 0).sum())
        if name in ("noise", "silence"):
            assert not (o64[0] > 0).any(), name
        if name == "late":                                                   # unvoiced, then voiced: both kinds of column
            assert not (o64[0, :40] > 0).any() and (o64[0, 80:110] > 0).all()
    assert voiced > 60


# ---- scale_f0 ---------------------------------------------------------------------------------------------------------------------------
def test_scale_f0_moves_the_voiced_columns_and_keeps_every_other_bit():
    rows = np.array([[50.0, 0.0, 200.0, 0.0, 399.0], [0.01, 0.7, 0.1, 1.2, 0.05]])
    ch = pitch.pitch_channels(rows, 40.0, 400.0)
    for scale in (2.0, 0.5, 1.3):
        got = pitch.scale_f0(ch, scale, 40.0, 400.0)
        want = pitch.pitch_channels(np.stack([rows[0] * scale, rows[1]]), 40.0, 400.0)
        v = rows[0] > 0
        assert np.abs(got[1, v] - want[1, v]).max() < 1e-12
        assert np.array_equal(got[:, ~v].view(np.uint64), ch[:, ~v].view(np.uint64))
        assert np.array_equal(got[[0, 2]].view(np.uint64), ch[[0, 2]].view(np.uint64))
        assert got is not ch and np.array_equal(ch, pitch.pitch_channels(rows, 40.0, 400.0))      # the input is left alone
    same = pitch.scale_f0(ch, 1.0, 40.0, 400.0)
    assert np.array_equal(same.view(np.uint64), ch.view(np.uint64))
    # float32 arrays and tensors: the shift is rounded to the array's type, and the two agree to the bit
    c32 = ch.astype(np.float32)
    g32 = pitch.scale_f0(c32, 2.0, 40.0, 400.0)
    t32 = pitch.scale_f0(torch.as_tensor(c32), 2.0, 40.0, 400.0)
    assert g32.dtype == np.float32 and t32.dtype == torch.float32
    assert np.array_equal(g32.view(np.uint32), t32.numpy().view(np.uint32))
    v = rows[0] > 0
    assert np.array_equal(g32[1, v], c32[1, v] + np.float32(1.0 / math.log2(10.0)))
    assert np.array_equal(g32[:, ~v].view(np.uint32), c32[:, ~v].view(np.uint32))
    assert torch.equal(pitch.scale_f0(torch.as_tensor(c32), 1.0, 40.0, 400.0), torch.as_tensor(c32))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scale_f0: scale = .*; it takes a finite scale > 0"):
            pitch.scale_f0(ch, bad, 40.0, 400.0)
    with pytest.raises(ValueError, match="scale_f0: fmax = 30.0; it takes fmax > fmin = 40.0"):
        pitch.scale_f0(ch, 2.0, 40.0, 30.0)
    with pytest.raises(ValueError, match=r"scale_f0: channels of shape \(2, 5\); it takes \(3, n\)"):
        pitch.scale_f0(rows, 2.0, 40.0, 400.0)


# ---- the streams, with the launches replaced by the definitions ---------------------------------------------------------------------------
def _pitch_cpu(log=None):
    p = pitch.Pitch(PC.RATE, PC.HOP, PC.WIN, PC.FMIN, PC.FMAX, PC.THRESHOLD, device="cpu")
    assert (p.tau_min, p.tau_max, p.span) == (PC.TAU_MIN, PC.TAU_MAX, PC.SPAN)
    p._launch = PC.numpy_pitch_launch(p, log)
    return p


@pytest.mark.parametrize("name", ["tone", "late"])
@pytest.mark.parametrize("chunking", ["1", "7", "hop", "3hops+5", "all"])
def test_the_pitch_stream_emits_the_counts_of_the_formula_keeps_the_tail_it_needs_and_adds_up_to_the_one_shot_call(name, chunking):
    x = PC.signals()[name].astype(np.float32)
    n = x.size
    log = []
    p = _pitch_cpu(log)
    want = p(x)
    assert want.shape == (2, features.frame_count(n, PC.HOP)) and log.pop() == (n, 0, want.shape[1], True, True)
    st, cols, fed = p.stream(), [], 0
    assert isinstance(st, pitch.PitchStream)
    for size in PC.chunkings(n)[chunking]:
        got = st.feed(x[fed:fed + size])
        fed += size
        cols.append(got)
        assert got.shape[0] == 2 and got.dtype == torch.float32
        assert sum(c.shape[1] for c in cols) == st.emitted == pitch.pitch_stream_frames(fed, PC.HOP, PC.SPAN)
        # only what a later column reads is kept: from emitted * hop - span // 2 on
        assert st.start == max(0, st.emitted * PC.HOP - PC.SPAN // 2) and st.tail.numel() == fed - st.start
        assert st.tail.numel() < PC.SPAN + max(size, PC.HOP)
    assert fed == n
    cols.append(st.flush())
    assert sum(c.shape[1] for c in cols) == pitch.pitch_stream_frames(n, PC.HOP, PC.SPAN, True) == want.shape[1]
    assert torch.equal(torch.cat(cols, dim=1), want)
    # the start flag only while the tail still begins at the signal's first sample, the end flag only in flush
    emitted = 0
    for size_, origin, count, start, end in log:
        assert start == (emitted * PC.HOP - origin == 0)                     # origin = emitted * hop - (signal index of tail[0])
        emitted += count
    assert [end for _, _, _, _, end in log] == [False] * (len(log) - 1) + [True]
    with pytest.raises(ValueError, match="Pitch.stream: feed after flush"):
        st.feed(x[:3])
    with pytest.raises(ValueError, match="Pitch.stream: flush twice"):
        st.flush()


def test_a_pitch_stream_that_was_fed_nothing_flushes_nothing():
    p = _pitch_cpu()
    st = p.stream()
    assert st.flush().shape == (2, 0) and p.launches == 0
    st = p.stream()
    assert st.feed(np.zeros(0, np.float32)).shape == (2, 0) and st.flush().shape == (2, 0) and p.launches == 0
    st = p.stream()                                                          # one sample: one column, made in flush
    assert st.feed(np.full(1, 0.25, np.float32)).shape == (2, 0)
    assert torch.equal(st.flush(), p(np.full(1, 0.25, np.float32)))


def _mel_pitch_cpu():
    both = acoustic.MelPitch(PC.RATE, PC.MELS, PC.HOP, PC.WIN, PC.FMIN, PC.FMAX, PC.THRESHOLD, device="cpu")
    both.pitch._launch = PC.numpy_pitch_launch(both.pitch)
    both.mel._launch = PC.numpy_mel_launch(both.mel)
    return both


def test_mel_pitch_has_the_attributes_of_its_two_analysers_and_is_their_concatenation():
    both = _mel_pitch_cpu()
    assert (both.hop, both.win, both.n_mels, both.n_channels) == (PC.HOP, PC.WIN, PC.MELS, PC.MELS + 3)
    assert both.device == torch.device("cpu") and isinstance(both.mel, features.LogMel) and isinstance(both.pitch, pitch.Pitch)
    x = PC.signals()["late"].astype(np.float32)
    got = both(x)
    assert got.shape == (PC.MELS + 3, features.frame_count(x.size, PC.HOP))
    assert torch.equal(got, torch.cat([both.mel(x), both.pitch.channels(both.pitch(x))]))
    want = acoustic.mel_pitch(x, PC.RATE, PC.MELS, PC.HOP, PC.WIN, PC.FMIN, PC.FMAX, PC.THRESHOLD)
    assert want.shape == got.shape and np.abs(got.numpy() - want).max() < 1e-5
    assert np.array_equal(got.numpy()[PC.MELS], want[PC.MELS]) and 0 < want[PC.MELS].sum() < want.shape[1]
    # a batch is one launch per analyser; a range is a slice
    clips = [x, PC.signals()["tone"].astype(np.float32), x[:333]]
    before = (both.mel.launches, both.pitch.launches)
    outs = both.batch(clips)
    assert (both.mel.launches, both.pitch.launches) == (before[0] + 1, before[1] + 1)
    for o, c in zip(outs, clips):
        assert torch.equal(o, both(c))
    assert torch.equal(both.frames(x, 70, 9), got[:, 70:79])
    assert both.batch([]) == []
    # the analysers' own refusals, under their own names
    with pytest.raises(ValueError, match="LogMel: a clip of 32 samples"):
        both(x[:32])
    with pytest.raises(ValueError, match="LogMel: integer input"):
        both(np.zeros(100, np.int32))
    with pytest.raises(ValueError, match="LogMel.frames: columns 120 .. 129 of a clip that has 125"):
        both.frames(x, 120, 10)
    with pytest.raises(ValueError, match="Pitch: tau_max = 2667"):
        acoustic.MelPitch(16000, 8, 256, 1024, fmin=6.0, device="cpu")
    with pytest.raises(ValueError, match="LogMel: win = 63"):
        acoustic.MelPitch(16000, 8, 16, 63, device="cpu")


@pytest.mark.parametrize("chunking", ["1", "7", "hop", "3hops+5", "all"])
def test_the_joint_stream_hands_out_what_both_analysers_have_and_adds_up_to_the_one_shot_call(chunking):
    x = PC.signals()["late"].astype(np.float32)[:900]
    n = x.size
    both = _mel_pitch_cpu()
    want = both(x)
    st, cols, fed = both.stream(), [], 0
    for size in PC.chunkings(n)[chunking]:
        got = st.feed(x[fed:fed + size])
        fed += size
        cols.append(got)
        assert got.shape[0] == PC.MELS + 3
        assert sum(c.shape[1] for c in cols) == st.emitted == acoustic.mel_pitch_stream_frames(fed, PC.HOP, PC.WIN, PC.SPAN)
        # the surplus mel columns wait inside the stream
        assert sum(c.shape[1] for c in st._mels) == features.mel_stream_frames(fed, PC.HOP, PC.WIN) - st.emitted
        assert not st._pits
    cols.append(st.flush())
    assert sum(c.shape[1] for c in cols) == want.shape[1] == acoustic.mel_pitch_stream_frames(n, PC.HOP, PC.WIN, PC.SPAN, True)
    assert not st._mels and not st._pits
    out = torch.cat(cols, dim=1)
    assert torch.equal(out[PC.MELS:], want[PC.MELS:])                        # the pitch rows: bit for bit also with numpy launches
    assert (out[:PC.MELS] - want[:PC.MELS]).abs().max() < 1e-5               # (numpy's matrix product is not held to bits per column)
    with pytest.raises(ValueError, match="MelPitch.stream: feed after flush"):
        st.feed(x[:3])
    with pytest.raises(ValueError, match="MelPitch.stream: flush twice"):
        st.flush()


# ---- local.json -----------------------------------------------------------------------------------------------------------------------------
PITCH = {"fmin": 40.0, "fmax": 400.0, "threshold": 0.15}


def test_the_pitch_key_is_written_only_with_the_flag_and_read_back(tmp_path):
    plain, both = str(tmp_path / "plain"), str(tmp_path / "both")
    assert cli_local.ensure_config(plain, 8, 16, mel={"win": 64}) == (8, 16)
    # byte for byte the file of a call that knows nothing of the key
    assert open(plain + "/local.json").read() == '{"channels": 8, "hop": 16, "mel": {"win": 64}}'
    assert cli_local.load_pitch(plain) is None and cli_local.mel_count(plain) == 8
    assert cli_local.ensure_config(both, 11, 16, mel={"win": 64}, pitch=PITCH) == (11, 16)
    assert json.loads(open(both + "/local.json").read()) == {"channels": 11, "hop": 16, "mel": {"win": 64}, "pitch": PITCH}
    assert cli_local.load_pitch(both) == PITCH and cli_local.mel_count(both) == 8 and cli_local.load_config(both) == (11, 16)
    assert cli_local.load_pitch(str(tmp_path / "none")) is None and cli_local.mel_count(str(tmp_path / "none")) is None
    assert cli_local.analysis_settings({"win": 64}, None) == {"win": 64}
    assert cli_local.analysis_settings({"win": 64}, PITCH) == {"win": 64, "pitch": PITCH}
    assert cli_local.analysis_settings(None, None) is None
    assert cli_local.PITCH_CHANNELS == pitch.PITCH_CHANNELS and cli_local.DEFAULT_PITCH == {"fmin": 60.0, "fmax": 500.0, "threshold": 0.15}
    # a file written by hand with a malformed entry is refused by name
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "local.json").write_text(json.dumps({"channels": 11, "hop": 16, "mel": {"win": 64}, "pitch": {"fmin": 40.0}}))
    with pytest.raises(Exception, match="local.json: \"pitch\" must be"):
        cli_local.load_pitch(str(bad))
    with pytest.raises(SystemExit, match="--local-pitch goes with --local-mel"):
        cli_local.ensure_config(str(tmp_path / "x"), 11, 16, pitch=PITCH)


def test_a_resumed_run_must_find_the_same_pitch_values_and_mel_count(tmp_path):
    plain, both = str(tmp_path / "plain"), str(tmp_path / "both")
    cli_local.ensure_config(plain, 8, 16, mel={"win": 64})
    cli_local.ensure_config(both, 11, 16, mel={"win": 64}, pitch=PITCH)
    assert cli_local.ensure_config(both, 11, 16, mel={"win": 64}, pitch=PITCH) == (11, 16)         # the same values: goes on
    assert cli_local.ensure_config(plain, 8, 16, mel={"win": 64}) == (8, 16)
    with pytest.raises(SystemExit, match=r"plain.local\.json: this checkpoint was trained without --local-pitch \(no \"pitch\"\), the "
                                         r"command line gives --local-mel with --local-pitch --f0-min 40.0 --f0-max 400.0 "
                                         r"--f0-threshold 0.15: a resumed run must find the same values"):
        cli_local.ensure_config(plain, 11, 16, mel={"win": 64}, pitch=PITCH)
    with pytest.raises(SystemExit, match=r"both.local\.json: this checkpoint was trained with --local-pitch --f0-min 40.0 --f0-max 400.0 "
                                         r"--f0-threshold 0.15, the command line gives --local-mel without --local-pitch"):
        cli_local.ensure_config(both, 8, 16, mel={"win": 64})
    for key, value, word in (("fmin", 50.0, "--f0-min 50.0"), ("fmax", 300.0, "--f0-max 300.0"), ("threshold", 0.2, "--f0-threshold 0.2")):
        with pytest.raises(SystemExit, match=r"trained with --local-pitch --f0-min 40.0 --f0-max 400.0 --f0-threshold 0.15, the "
                                             r"command line gives --local-mel with --local-pitch .*%s" % word):
            cli_local.ensure_config(both, 11, 16, mel={"win": 64}, pitch=dict(PITCH, **{key: value}))
    with pytest.raises(SystemExit, match=r"both.local\.json: this checkpoint was trained with --local-pitch on 8 mel channels \(and 3 "
                                         r"pitch channels\), the command line gives --mels 13: a resumed run must find the same value"):
        cli_local.ensure_config(both, 16, 16, mel={"win": 64}, pitch=PITCH)
    with pytest.raises(SystemExit, match="trained with --local-mel --win 64, the command line gives --local-mel --win 128"):
        cli_local.ensure_config(both, 11, 16, mel={"win": 128}, pitch=PITCH)                         # the older checks still come first
    # feature files on such a checkpoint (no --local-mel): the channel count is all that is compared, as before
    assert cli_local.ensure_config(both, 11, 16) == (11, 16)


# ---- the command lines ------------------------------------------------------------------------------------------------------------------------
def _no_model(monkeypatch):
    from wavenet_amd.train_audio import model as cli_model

    def build(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli_model, "build", build)


def test_without_the_new_flags_the_parsers_give_the_namespace_they_gave():
    from wavenet_amd.train_audio import args as cli_args
    from wavenet_amd.train_audio import features as cli_features
    new = {"local_pitch": True, "f0_min": 50.0, "f0_max": 450.0, "f0_threshold": 0.2}
    flags = ["--local-pitch", "--f0-min", "50", "--f0-max", "450", "--f0-threshold", "0.2"]
    for argv in (["--local-mel"], ["--local-mel", "--mels", "8", "--corpus"]):
        without, with_flags = cli_args.parse(argv), cli_args.parse(argv + flags)
        assert not set(new) & set(vars(without)) and "f0_scale" not in vars(without)
        assert (without.local_pitch, without.f0_min, without.f0_max, without.f0_threshold, without.f0_scale) == (False, None, None, None, 1.0)
        assert {k: v for k, v in vars(with_flags).items() if k not in new} == vars(without)
        assert {k: getattr(with_flags, k) for k in new} == new
    for argv in ([], ["--fast", "--from-wav", "f.wav"], ["--fast", "--local", "f.npy", "--chunk-frames", "4"]):
        without, with_flag = cli_args.parse(argv), cli_args.parse(argv + ["--f0-scale", "2"])
        assert {k: v for k, v in vars(with_flag).items() if k != "f0_scale"} == vars(without) and with_flag.f0_scale == 2.0
    assert vars(cli_features.build_parser().parse_args([])) == {
        "wav_dir": "wav", "output_dir": "features", "hop": 256, "mels": 80, "win": 1024, "quantization_steps": 256, "device": False}
    args = cli_features.build_parser().parse_args(["--pitch", "--f0-min", "40"])
    assert cli_features.pitch_settings(args) == {"fmin": 40.0, "fmax": 500.0, "threshold": 0.15}
    assert cli_features.pitch_settings(cli_features.build_parser().parse_args([])) is None
    with pytest.raises(SystemExit, match="--f0-min, --f0-max and --f0-threshold go with --pitch"):
        cli_features.pitch_settings(cli_features.build_parser().parse_args(["--f0-max", "300"]))


@pytest.mark.parametrize("argv,word", [
    (["--local-pitch"], "--local-pitch .* goes with --local-mel, not with --local-dir"),
    (["--local-pitch", "--local-dir", "feat"], "--local-pitch .* goes with --local-mel, not with --local-dir"),
    (["--local-mel", "--f0-min", "50"], "--f0-min, --f0-max and --f0-threshold go with --local-pitch"),
])
def test_train_refuses_pitch_flags_that_do_not_go_together_when_it_parses(tmp_path, monkeypatch, capsys, argv, word):
    import re
    from wavenet_amd.train_audio import train as cli_train
    _no_model(monkeypatch)
    with pytest.raises(SystemExit):
        cli_train.main(["-w", str(tmp_path), "-m", str(tmp_path / "model")] + argv)
    assert re.search(word, capsys.readouterr().err)


@pytest.mark.parametrize("argv,word", [
    (["--f0-max", "5000"], r"--local-pitch: pitch_lags: tau_min = floor\(8000 / 5000.0\) = 1 < 2"),
    (["--f0-min", "3"], "--local-pitch: Pitch: tau_max = 2667; the device kernel takes"),
    (["--f0-min", "500", "--f0-max", "400"], "--local-pitch: pitch_lags: rate = 8000, fmin = 500.0, fmax = 400.0"),
    (["--local-hop", "40000"], "--local-pitch: Pitch: .* bytes of LDS"),
    (["--f0-threshold", "0"], "--local-pitch: Pitch: threshold = 0.0"),
])
def test_train_tries_the_pitch_trackers_refusals_before_a_model_is_built(tmp_path, monkeypatch, argv, word):
    from wavenet_amd.train_audio import train as cli_train
    _no_model(monkeypatch)
    base = ["-w", str(tmp_path), "-m", str(tmp_path / "model"), "--local-mel", "--local-pitch"]       # (a new model: 8,000 Hz)
    with pytest.raises(SystemExit, match=word):
        cli_train.main(base + argv)
    with pytest.raises(SystemExit, match="train: --f0-scale belongs to generate"):
        cli_train.main(base + ["--f0-scale", "2"])
    with pytest.raises(AssertionError, match="a model was built"):           # everything checked: the model comes next
        cli_train.main(base)


def test_generate_refuses_f0_scale_before_a_model_is_built(tmp_path, monkeypatch):
    from wavenet_amd.train_audio import generate as cli_generate
    _no_model(monkeypatch)
    model = tmp_path / "model"
    model.mkdir()
    base = ["-m", str(model), "-o", str(tmp_path / "out"), "--fast"]
    (model / "local.json").write_text(json.dumps({"channels": 8, "hop": 16, "mel": {"win": 64}}))
    with pytest.raises(SystemExit, match="--f0-scale moves the pitch channels of a checkpoint trained with train --local-mel "
                                         "--local-pitch .*local.json has no \"pitch\""):
        cli_generate.main(base + ["--from-wav", "f.wav", "--f0-scale", "2"])
    with pytest.raises(SystemExit, match="has no \"pitch\""):                 # also at 1: the flag asks for such a checkpoint
        cli_generate.main(base + ["--local", "f.npy", "--f0-scale", "1"])
    (model / "local.json").write_text(json.dumps({"channels": 11, "hop": 16, "mel": {"win": 64}, "pitch": PITCH}))
    for bad in ("0", "-2", "nan", "inf"):
        with pytest.raises(SystemExit, match="--f0-scale S needs a finite S > 0, got %s" % bad):
            cli_generate.main(base + ["--from-wav", "f.wav", "--f0-scale", bad])
    with pytest.raises(SystemExit, match="--f0-scale does not go with --rank mel: the recording is no target for a shifted voice"):
        cli_generate.main(base + ["--from-wav", "f.wav", "--best-of", "2", "--rank", "mel", "--f0-scale", "2"])
    with pytest.raises(SystemExit, match="--f0-scale does not go with --keep"):
        cli_generate.main(base + ["--keep", "k.wav", "--local", "f.npy", "--f0-scale", "2"])
    assert cli_generate.f0_scale_job(cli_generate._args.parse(base + ["--local", "f.npy", "--f0-scale", "2"])) == (2.0, 40.0, 400.0, 8)
    assert cli_generate.f0_scale_job(cli_generate._args.parse(base + ["--local", "f.npy"])) is None


def test_scaled_f0_touches_rows_f_to_f_plus_2_only():
    from wavenet_amd.train_audio import generate as cli_generate
    rs = np.random.RandomState(0)
    feats = rs.randn(11, 6).astype(np.float32)
    feats[8] = [1, 0, 1, 1, 0, 0]
    f0 = (2.0, 40.0, 400.0, 8)
    got = cli_generate.scaled_f0(feats, f0)
    want = feats.copy()
    want[9, feats[8] == 1] += np.float32(1.0 / math.log2(10.0))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got is not feats
    assert torch.equal(cli_generate.scaled_f0(torch.as_tensor(feats), f0), torch.as_tensor(want))
    assert cli_generate.scaled_f0(feats, None) is feats and cli_generate.scaled_f0(feats, (1.0, 40.0, 400.0, 8)) is feats
