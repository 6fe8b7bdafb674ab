"""The host side of the rate converter: the numpy definition against the double sum and scipy, the filter it designs, the
streaming arithmetic, float32 against float64 PCM, the ABI's names and refusals (no GPU needed), and the flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_ref as R
from wavenet_amd import _resample, data, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(zip(R.RATIOS, R.LENGTHS))
IDS = ["%d-%d" % r for r in R.RATIOS]


@pytest.mark.parametrize("rates,n", CASES, ids=IDS)
def test_the_polyphase_form_is_the_double_sum_of_the_definition(rates, n):
    x = R.chirp_noise(n, rates[0])
    got, want = resample.resample(x, *rates), resample.resample_direct(x, *rates)
    L, M = resample.ratio(*rates)
    assert got.dtype == np.float64 and got.shape == want.shape == (-(-n * L // M),)
    assert np.abs(got - want).max() < 1e-13                          # the same products, summed in another order


@pytest.mark.parametrize("rates,n", CASES, ids=IDS)
def test_scipy_resample_poly_with_the_float64_taps_agrees(rates, n):
    signal = pytest.importorskip("scipy.signal")
    x = R.chirp_noise(n, rates[0])
    L, M = resample.ratio(*rates)
    want = signal.resample_poly(x, L, M, window=resample.prototype(L, M) / L)
    assert np.abs(resample.resample(x, *rates) - want).max() < 1e-9


def test_the_tables_are_the_float64_rows_rounded_once():
    for rates in R.RATIOS:
        L, M, P, T, taps = resample.resample_tables(*rates)
        K = max(L, M)
        assert (L, M) == resample.ratio(*rates) and P == 32 * K and T == 2 * (-(-P // L)) + 1
        h = resample.prototype(L, M)
        assert h.size == 2 * P + 1 and np.array_equal(h, h[::-1])
        Kt = (T - 1) // 2
        want = np.zeros((L, T))
        for phi in range(L):
            for t in range(T):
                i = phi + (t - Kt) * L
                if abs(i) <= P:
                    want[phi, t] = h[i + P]
        assert taps.dtype == np.float32 and taps.shape == (L, T) and np.array_equal(taps, want.astype(np.float32))
    assert resample.resample_tables(48000, 16000, zeros=16, rolloff=0.8, beta=6.0)[2:4] == (48, 97)      # constructor arguments


@pytest.mark.parametrize("K", [3, 441])
def test_the_filter_is_flat_to_0p8_and_80_db_down_from_the_lower_nyquist_frequency(K):
    """From the float64 taps, on 500 frequencies up to 0.8 x the lower rate's Nyquist frequency and 5,000 from 1.0 x up to the
    prototype's own Nyquist frequency (K x): the side lobes are 1 / 32 of that unit wide, the grid has 20 points per lobe
    up to 4 x."""
    L, M = (1, 3) if K == 3 else (160, 441)
    h = resample.prototype(L, M)
    nyq = 1.0 / (2 * K)                                              # the lower Nyquist frequency over the prototype's rate
    flat = R.response_db(h, L, np.linspace(0.0, 0.8, 500) * nyq)
    stop = R.response_db(h, L, np.concatenate([np.linspace(1.0, min(4.0, K), 3000), np.linspace(min(4.0, K), K, 2000)]) * nyq)
    edge = R.response_db(h, L, np.array([0.9]) * nyq)
    print("K = %d: pass band %.4f .. %.4f dB, %.2f dB at 0.9, stop band max %.1f dB" % (K, flat.min(), flat.max(), edge[0], stop.max()))
    assert np.abs(flat).max() <= 0.1
    assert abs(edge[0] + 6.0) < 0.1
    assert stop.max() <= -80.0


def test_unit_gain_at_0_hz_and_equal_rates_are_the_identity():
    for rates in R.RATIOS:
        L, M = resample.ratio(*rates)
        y = resample.resample(np.ones(4000), *rates)
        mid = y[y.size // 3:2 * y.size // 3]                         # away from the ends, where the zeros outside pull it down
        assert np.abs(mid - 1.0).max() < 1e-4, rates
        assert abs(resample.prototype(L, M).sum() / L - 1.0) < 1e-4
    x = R.chirp_noise(333)
    assert np.array_equal(resample.resample(x, 16000, 16000).view(np.uint64), x.view(np.uint64))
    x32 = x.astype(np.float32)
    rs = resample.Resampler(22050, 22050, device=None)
    assert rs.identity and np.array_equal(rs(x32).astype(np.float32).view(np.uint32), x32.view(np.uint32))
    assert np.array_equal(rs(R.pcm16(100), out="pcm16"), R.pcm16(100))


@pytest.mark.parametrize("rates", R.RATIOS, ids=IDS)
def test_stream_counts_are_the_brute_force_count(rates):
    L, M, P, T, _ = resample.resample_tables(*rates)
    for fed in range(0, 3 * P // L + 51):
        # output n exists once sample 0 .. are fed if n < ceil(fed L / M), and is complete when its last input has arrived
        total = -(-fed * L // M)
        brute = sum(1 for n in range(total) if (n * M + P) // L <= fed - 1)
        assert resample.resample_stream_counts(fed, L, M, P) == brute, (rates, fed)
        assert resample.resample_stream_counts(fed, L, M, P, True) == total
        assert brute <= total
        # every input below stream_keep_from(n) is read by no output from n on
        n = brute
        lows = [max(0, -(-(k * M - P) // L)) for k in range(n, n + 3)]
        assert resample.stream_keep_from(n, L, M, P) == min(lows)


@pytest.mark.parametrize("rates", R.RATIOS, ids=IDS)
@pytest.mark.parametrize("chunk", [1, 7, 160, 1001])
def test_a_host_stream_is_the_one_shot_call_whatever_the_chunking(rates, chunk):
    n = 1203
    x = R.pcm16(n, rates[0])
    rs = resample.Resampler(*rates, device=None)
    want = rs(x)
    st, parts, fed = rs.stream(), [], 0
    for part in [x[:0], x[:0]] + [x[at:at + chunk] for at in range(0, n, chunk)]:          # two empty feeds first
        parts.append(st.feed(part))
        fed += part.size
        assert sum(p.size for p in parts) == resample.resample_stream_counts(fed, rs.L, rs.M, rs.P)
        assert st.tail.size <= 2 * rs.P // rs.L + 2 + chunk          # only what later outputs read is kept
    parts.append(st.flush())
    got = np.concatenate(parts)
    assert fed == n and got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    first, count = 37, 200
    lo, hi = rs.reach(first, count)
    lo = max(lo, 0)
    assert np.array_equal(rs.block(x[lo:hi + 1], lo, first, count, start=lo == 0), want[first:first + count])


@pytest.mark.parametrize("rates", R.RATIOS, ids=IDS)
def test_float32_pcm_is_within_one_step_of_float64_pcm_and_so_are_the_tokens(rates):
    x = R.pcm16(3000, rates[0])
    a, b = resample.to_pcm16(R.resample_f32(x, *rates)), resample.to_pcm16(resample.resample(x, *rates))
    d = np.abs(a.astype(np.int64) - b)
    print("%d -> %d: %.2f %% of the PCM samples differ (by 1)" % (rates + (100.0 * (d > 0).mean(),)))
    assert d.max() <= 1
    for Q in (256, 1024):
        ta, tb = data.mulaw_encode_pcm16(a, Q), data.mulaw_encode_pcm16(b, Q)
        assert np.abs(ta.astype(np.int64) - tb).max() <= 1
        assert np.array_equal(tb, resample.resample_tokens(x, rates[0], rates[1], Q))


def test_to_pcm16_rounds_half_to_even_and_clips():
    y = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 40000.0, -40000.0, 32767.4, 32767.6]) / 32768.0
    assert resample.to_pcm16(y).tolist() == [0, 2, 2, 0, -2, 32767, -32768, 32767, 32767]
    assert resample.to_pcm16(y).dtype == np.int16


def test_a_full_scale_square_wave_overshoots_and_clips_to_the_end_tokens():
    x = R.square(1200)
    y = resample.resample(x, 48000, 16000)
    assert y.max() > 1.0 and y.min() < -1.0
    pcm = resample.to_pcm16(y)
    assert pcm.max() == 32767 and pcm.min() == -32768
    for Q in (256, 1024):
        tok = resample.resample_tokens(x, 48000, 16000, Q)
        ends = data.mulaw_encode_pcm16(np.array([-32768, 32767], np.int16), Q)       # the table's ends: 0, and Q - 2 (32767 / 32768 < 1)
        assert ends.tolist() == [0, Q - 2] and tok.min() == ends[0] and tok.max() == ends[1]
    f32 = resample.to_pcm16(R.resample_f32(x, 48000, 16000))
    assert f32.max() == 32767 and f32.min() == -32768


# ---- the library: names, refusals ------------------------------------------------------------------------------------------------
def test_header_map_and_binding_name_the_same_three_functions():
    hdr = open(os.path.join(ROOT, "include", "wavenet_resample.h")).read()
    declared = set(re.findall(r"\b(wn_resample[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_resample.EXPORTS) == {"wn_resample_abi_version", "wn_resample_last_error", "wn_resample"}
    assert "wn_resample*" in open(os.path.join(ROOT, "wavenet_amd", "csrc", "front", "resample_exports.map")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _resample.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in nm.splitlines() if ln.strip()} == declared
    assert _resample.lib().wn_resample_abi_version() == _resample.ABI_VERSION == int(
        re.search(r"#define WN_RESAMPLE_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("WN_RESAMPLE_MAX_CLIPS", "WN_RESAMPLE_TILE", "WN_RESAMPLE_IN_PCM16", "WN_RESAMPLE_IN_F32", "WN_RESAMPLE_OUT_F32",
                 "WN_RESAMPLE_OUT_PCM16", "WN_RESAMPLE_OUT_TOKENS", "WNR_EARG", "WNR_EHIP"):
        assert int(re.search(r"#define %s\s+(-?\d+)" % name, hdr).group(1)) == getattr(_resample, name), name
    assert (_resample.WN_RESAMPLE_TILE, _resample.WN_RESAMPLE_MAX_CLIPS) == (resample.RESAMPLE_TILE, resample.RESAMPLE_MAX_CLIPS)
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct WnResampleClip \{(.*?)\} WnResampleClip;", hdr, re.S).group(1), flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _resample.WnResampleClip._fields_]
    assert C.sizeof(_resample.WnResampleClip) == 6 * 8 + 2 * 4
    assert "getenv" not in open(os.path.join(ROOT, "wavenet_amd", "csrc", "front", "resample.hip")).read()


def test_wn_resample_refuses_every_bad_argument_by_name_without_a_gpu():
    lib = _resample.lib()
    EARG = _resample.WNR_EARG

    def clip(**kw):
        d = dict(x=64, n=4000, origin=0, out=64, first=0, count=100, flags=3)
        d.update(kw)
        return C.byref(_resample.WnResampleClip(**d))

    def call(cl, n_clips=1, in_kind=0, out_kind=0, taps=64, L=1, M=3, T=193, lut=None):
        return lib.wn_resample(cl, n_clips, in_kind, out_kind, taps, L, M, T, lut, None)

    assert call(None) == EARG and b"NULL" in lib.wn_resample_last_error()
    assert call(clip(), taps=None) == EARG and b"NULL" in lib.wn_resample_last_error()
    for kw, word in [(dict(L=0), b"L = 0"), (dict(L=1025), b"L = 1025"), (dict(M=0), b"M = 0"), (dict(M=1025), b"M = 1025"),
                     (dict(L=3, M=3), b"L == M = 3"), (dict(T=192), b"T = 192"), (dict(T=1), b"T = 1"), (dict(T=2049), b"T = 2049"),
                     (dict(n_clips=0), b"n_clips = 0"), (dict(n_clips=65), b"n_clips = 65"), (dict(in_kind=2), b"in_kind = 2"),
                     (dict(out_kind=3), b"out_kind = 3"), (dict(out_kind=-1), b"out_kind = -1"),
                     (dict(out_kind=2), b"out_kind = 2 (tokens) needs lut"),
                     (dict(L=2, M=1023, T=2047), b"bytes of LDS")]:
        assert call(clip(), **kw) == EARG, kw
        assert word in lib.wn_resample_last_error(), (kw, lib.wn_resample_last_error())
    for kw, word in [(dict(count=-1), b"count = -1"), (dict(first=-2), b"first = -2"), (dict(origin=-5, flags=2), b"origin = -5"),
                     (dict(origin=7), b"origin = 7 under WN_RESAMPLE_START"), (dict(flags=4), b"flags = 4"),
                     (dict(x=None), b"NULL buffer"), (dict(out=None), b"NULL buffer"),
                     # output 0 reads inputs -96 .. 96; outputs 0 .. 1333 are all of 4,000 samples, the last reads input 4095
                     (dict(flags=2), b"output 0 reads input -96, before the buffer"),
                     (dict(flags=1, first=1300, count=10), b"output 1309 reads input 4023, the buffer ends with 3999"),
                     (dict(flags=0, origin=1000, first=365, count=10), b"output 365 reads input 999, before the buffer (origin 1000)"),
                     (dict(flags=0, origin=1000, n=500, first=366, count=103), b"output 468 reads input 1500, the buffer ends with 1499")]:
        assert call(clip(**kw)) == EARG, kw
        assert word in lib.wn_resample_last_error(), (kw, lib.wn_resample_last_error())
    from wavenet_amd import _lib
    with pytest.raises(_lib.WaveNetHipError, match="T = 192"):
        _resample.check(call(clip(), T=192))
    assert call(clip(count=0, x=None, out=None)) == _resample.WNR_OK          # nothing to do: nothing is launched


def test_the_python_face_names_what_the_kernel_refuses_and_the_definition_serves_it():
    assert resample._device_refusal(1, 3, 193) is None and resample._device_refusal(160, 441, 179) is None
    assert "M = 1025" in resample._device_refusal(1, 1025, 65)
    assert "T = 2049" in resample._device_refusal(2, 3, 2049)
    assert "bytes of LDS" in resample._device_refusal(2, 1023, 2047)
    rs = resample.Resampler(48000, 16000, device=None)
    assert not rs.on_device and rs.refusal is None
    with pytest.raises(ValueError, match="out = 'wav'"):
        rs(np.zeros(10, np.float32), out="wav")
    with pytest.raises(ValueError, match="int16 PCM or floating point"):
        rs(np.zeros(10, np.int32))
    with pytest.raises(ValueError, match=r"outputs 0 .. 9 read inputs -96 .. 123, the buffer holds 0 .. 99"):
        rs.block(np.zeros(100, np.float32), 0, 0, 10)
    x = R.chirp_noise(900).astype(np.float32)
    assert np.array_equal(rs(x), resample.resample(x, 48000, 16000))
    assert np.array_equal(rs(x, out="tokens", quantization_steps=1024), resample.resample_tokens(x, 48000, 16000, 1024))
    outs = rs.batch([x, x[:100], x[:0]], out="pcm16")
    assert [o.size for o in outs] == [300, 34, 0] and np.array_equal(outs[1], resample.to_pcm16(resample.resample(x[:100], 48000, 16000)))


# ---- the loader and the command line -------------------------------------------------------------------------------------------------
def _wav(path, rate, samples):
    from scipy.io import wavfile
    wavfile.write(str(path), rate, samples)
    return str(path)


def test_load_audio_file_without_rate_is_what_it_was_and_with_rate_converts(tmp_path):
    pcm = R.pcm16(2400, 48000)
    f48 = _wav(tmp_path / "f48.wav", 48000, pcm)
    tok, rate = data.load_audio_file(f48)
    assert rate == 48000 and tok.dtype == np.int32
    assert np.array_equal(tok, data.trim_silence(data.mulaw_encode(pcm.astype(float) / 32768), 1, True))      # the function as it was
    same, r2 = data.load_audio_file(f48, rate=48000)                 # already at the rate: that path
    assert r2 == 48000 and np.array_equal(same, tok)
    got, r3 = data.load_audio_file(f48, rate=16000)                  # no device: the numpy definition
    assert r3 == 16000 and got.dtype == np.int32
    assert np.array_equal(got, data.trim_silence(resample.resample_tokens(pcm, 48000, 16000, 256), 1, True))
    stereo = _wav(tmp_path / "st.wav", 48000, np.stack([pcm, pcm[::-1]], axis=1))
    assert np.array_equal(data.load_audio_file(stereo, rate=16000)[0], got)                                  # the left channel
    flt = _wav(tmp_path / "fl.wav", 48000, (pcm / 32768.0).astype(np.float32))
    assert np.array_equal(data.load_audio_file(flt, rate=16000)[0], got)
    f8 = _wav(tmp_path / "u8.wav", 48000, (pcm // 256 + 128).astype(np.uint8))
    with pytest.raises(Exception, match=r"u8.wav holds uint8 samples: only 16-bit PCM and float"):
        data.load_audio_file(f8, rate=16000)
    f16 = _wav(tmp_path / "f16.wav", 16000, pcm[:800])
    many = data.load_audio_files([f48, f16, flt], 16000, 256, None)
    assert np.array_equal(many[0], got) and np.array_equal(many[2], got) and np.array_equal(many[1], data.load_audio_file(f16)[0])


def test_the_tool_writes_mono_16_bit_files_of_the_definition(tmp_path, capsys):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import resample as cli
    (tmp_path / "wav").mkdir()
    pcm = R.pcm16(1323, 44100)
    _wav(tmp_path / "wav" / "a.wav", 44100, pcm)
    _wav(tmp_path / "wav" / "b.wav", 16000, pcm[:50])
    written = cli.main(["-w", str(tmp_path / "wav"), "-o", str(tmp_path / "out"), "--rate", "16000"])
    assert [os.path.basename(w) for w in written] == ["a.wav", "b.wav"]
    rate, a = wavfile.read(written[0])
    assert rate == 16000 and a.dtype == np.int16 and a.ndim == 1
    assert np.array_equal(a, resample.to_pcm16(resample.resample(pcm, 44100, 16000)))
    assert np.array_equal(wavfile.read(written[1])[1], pcm[:50])
    assert "a.wav: 1323 samples at 44100 Hz -> 480 samples at 16000 Hz" in capsys.readouterr().out


def test_features_without_the_flag_takes_each_file_at_its_own_rate_and_with_it_at_the_given_one(tmp_path):
    from wavenet_amd import features
    from wavenet_amd.train_audio import features as cli
    (tmp_path / "wav").mkdir()
    pcm = R.pcm16(2400, 48000)
    _wav(tmp_path / "wav" / "a.wav", 48000, pcm)
    _wav(tmp_path / "wav" / "b.wav", 16000, pcm[:900])
    shape = ["--hop", "16", "--mels", "8", "--win", "64"]
    cli.main(["-w", str(tmp_path / "wav"), "-o", str(tmp_path / "plain")] + shape)
    cli.main(["-w", str(tmp_path / "wav"), "-o", str(tmp_path / "conv"), "--resample", "--rate", "16000"] + shape)
    for name, rate in (("a", 48000), ("b", 16000)):                  # as it was: the file's samples, the file's rate
        tok = data.load_audio_file(str(tmp_path / "wav" / (name + ".wav")))[0]
        want = features.log_mel(data.mulaw_decode(tok, 256), rate, 8, 16, 64)
        assert np.array_equal(np.load(str(tmp_path / "plain" / (name + ".npy"))), want)
    tok = data.load_audio_file(str(tmp_path / "wav" / "a.wav"), rate=16000)[0]
    assert np.array_equal(np.load(str(tmp_path / "conv" / "a.npy")), features.log_mel(data.mulaw_decode(tok, 256), 16000, 8, 16, 64))
    assert (tmp_path / "conv" / "b.npy").read_bytes() == (tmp_path / "plain" / "b.npy").read_bytes()


def test_parse_accepts_resample_with_the_flags_it_works_with_and_is_unchanged_without():
    from wavenet_amd.train_audio import args as cli_args
    combos = [["--speaker-prefix", "--condition-channels", "4"], ["--local-dir", "d", "--local-hop", "16"],
              ["--local-mel", "--mels", "8", "--win", "64", "--local-interp", "linear", "--local-crop", "sample"],
              ["--local-mel", "--local-upsample", "4", "--local-crop", "frame"], ["--ema-decay", "0.999", "--valid-wav-dir", "v"],
              ["--storage", "bf16"], ["--no-graph"], ["--corpus"], ["--fast", "--from-wav", "f.wav"], ["--fast", "--keep", "k.wav"],
              ["--prompt", "p.wav"], []]
    for argv in combos:
        without, with_flag = cli_args.parse(argv), cli_args.parse(argv + ["--resample"])
        assert with_flag.resample is True and without.resample is False and "resample" not in vars(without)
        assert dict(vars(with_flag), resample=None) == dict(vars(without), resample=None)
    assert vars(cli_args.parse([])) == {k: v for k, v in vars(cli_args.parse(["--resample"])).items() if k != "resample"}
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import features as cli_features
    for mod in (cli_evaluate, cli_features):
        assert "resample" not in vars(mod.build_parser().parse_args([]))
        assert mod.build_parser().parse_args(["--resample"]).resample is True
    with pytest.raises(SystemExit, match="--resample needs the rate"):
        cli_features.target_rate(cli_features.build_parser().parse_args(["--resample"]))
    with pytest.raises(SystemExit, match="go with --resample"):
        cli_features.target_rate(cli_features.build_parser().parse_args(["--rate", "16000"]))
    assert cli_features.target_rate(cli_features.build_parser().parse_args(["--resample", "--rate", "16000"])) == 16000
    assert cli_features.target_rate(cli_features.build_parser().parse_args([])) is None
