"""Sample-rate conversion on the device (wn_resample, resample.Resampler) against the numpy definition, and the determinism
contract: an output's bits depend on its own T input samples and the taps only -- not on tile mates, batch mates, the call, the
chunking of a stream, the buffer's origin, or int16 versus the same values as float32."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import resample_ref as R
from gpu_util import to_np
from wavenet_amd import _lib, _resample, data, resample
from wavenet_amd.resample import Resampler, resample_stream_counts

pytestmark = pytest.mark.gpu
TILE = _resample.WN_RESAMPLE_TILE
IDS = ["%d-%d" % r for r in R.RATIOS]
_RS, _X = {}, {}


def rs_of(rates):
    if rates not in _RS:
        _RS[rates] = Resampler(*rates, device="cuda")
    return _RS[rates]


def length_for(rates, outputs):
    """The shortest input with at least ``outputs`` outputs."""
    L, M = resample.ratio(*rates)
    return -(-outputs * M // L)


def pcm(rates, n):
    if (rates, n) not in _X:
        _X[rates, n] = R.pcm16(n, rates[0], seed=n)
    return _X[rates, n]


def same_bits(a, b):
    a, b = [v if isinstance(v, np.ndarray) else to_np(v) for v in (a, b)]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("rates", R.RATIOS, ids=IDS)
def test_every_output_is_within_four_float32_restatement_errors_of_the_definition(rates):
    """Bar per ratio: 4 x the error of tests/resample_ref.py (float32 products and sums in numpy) against resample.resample on
    the same input.  Two full tiles and a ragged rest of 37 outputs."""
    n = length_for(rates, 2 * TILE + 37)
    x = pcm(rates, n)
    want = resample.resample(x, *rates)
    bar, ref_err = R.bar(x, *rates)
    got = to_np(rs_of(rates)(x))
    assert got.dtype == np.float32 and got.shape == want.shape and got.size > 2 * TILE and got.size % TILE
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("resample %d -> %d, %d samples: device %.3g, float32 restatement %.3g, bar %.3g" % (rates + (n, err, ref_err, bar)))
    assert np.isfinite(got).all()
    assert err <= bar, (err, bar)
    zeros = to_np(rs_of(rates)(np.zeros(n, np.int16)))
    assert zeros.shape == want.shape and not zeros.view(np.uint32).any()                  # +0.0 everywhere


@pytest.mark.parametrize("rates", R.RATIOS, ids=IDS)
def test_int16_and_the_same_values_as_float32_give_the_same_bits(rates):
    x = pcm(rates, length_for(rates, TILE + 5))
    rs = rs_of(rates)
    assert same_bits(rs(x), rs((x.astype(np.float32) / np.float32(32768.0))))


@pytest.mark.parametrize("rates", R.RATIOS[:2] + R.RATIOS[4:], ids=IDS[:2] + IDS[4:])
def test_a_batch_is_its_single_calls_and_a_block_is_a_slice(rates):
    rs = rs_of(rates)
    lengths = [length_for(rates, 2 * TILE + 37), length_for(rates, TILE), 301]             # ragged; exactly a tile or just over; short
    clips = [pcm(rates, n) for n in lengths]
    before = rs.launches
    outs = rs.batch(clips)
    assert rs.launches == before + 1
    singles = [rs(c) for c in clips]
    for o, s, n in zip(outs, singles, lengths):
        assert same_bits(o, s) and o.numel() == rs.count(n)
    x, full = clips[0], singles[0]
    total = full.numel()
    # the start of the signal; a stretch across a tile border from a buffer that starts inside the signal (no flag needed);
    # the end of the signal from a buffer that holds only its tail
    for first, count in [(0, 50), (TILE - 20, 300), (total - 70, 70)]:
        lo, hi = rs.reach(first, count)
        lo, hi = max(lo, 0), min(hi, x.size - 1)
        part = rs.block(x[lo:hi + 1], lo, first, count, start=lo == 0, end=hi == x.size - 1)
        assert same_bits(part, full[first:first + count].contiguous()), (first, count)


@pytest.mark.parametrize("rates", R.RATIOS[:3], ids=IDS[:3])
@pytest.mark.parametrize("chunk", [1, 7, 160, 1001])
def test_streaming_is_the_one_shot_call_whatever_the_chunking(rates, chunk):
    n = 1203 if chunk > 1 else 500
    x = pcm(rates, n)
    rs = rs_of(rates)
    want = rs(x)
    st, parts, fed = rs.stream(), [], 0
    for part in [x[:0]] + [x[at:at + chunk] for at in range(0, n, chunk)]:                 # an empty feed first
        parts.append(st.feed(part))
        fed += part.size
        assert sum(p.numel() for p in parts) == resample_stream_counts(fed, rs.L, rs.M, rs.P)
        assert st.tail.numel() <= 2 * rs.P // rs.L + 2 + chunk                             # only what later outputs read is kept
    parts.append(st.flush())
    assert sum(p.numel() for p in parts) == resample_stream_counts(n, rs.L, rs.M, rs.P, True) == want.numel()
    assert same_bits(torch.cat(parts), want)


def test_a_stream_of_tokens_and_the_chain_into_the_mel_analyser():
    from wavenet_amd.features import LogMel
    rates, n = (48000, 16000), 6000
    x = pcm(rates, n)
    rs, mel = rs_of(rates), LogMel(16000, 8, 16, 64)
    st, parts = rs.stream(out="tokens", quantization_steps=256), []
    for at in range(0, n, 480):
        parts.append(st.feed(x[at:at + 480]))
    parts.append(st.flush())
    assert same_bits(torch.cat(parts), rs(x, out="tokens", quantization_steps=256))
    want = mel(rs(x))
    conv, an, cols = rs.stream(), mel.stream(), []
    for at in range(0, n, 480):
        cols.append(an.feed(conv.feed(x[at:at + 480])))                                    # device tensors all the way
    cols.append(an.feed(conv.flush()))
    cols.append(an.flush())
    assert same_bits(torch.cat(cols, dim=1), want)


def test_outputs_whose_n_times_m_passes_2_to_the_33_equal_the_same_phase_near_zero():
    """44100 -> 16000 (L = 160, M = 441): shifting the buffer by k M inputs and the outputs by k L leaves q - origin and phi of
    every output as they were, so the bits must be those of the small origin.  k = 200,000: n M reaches 1.4e10 > 2^33; a
    32-bit product would land on other samples."""
    rates = (44100, 16000)
    rs = rs_of(rates)
    x, small, k = pcm(rates, 4000), 100, 200000
    big = small + k * rs.M
    assert big % rs.M == small
    firsts = [n for n in range(0, 2000) if rs.reach(n, 1)[0] >= small and rs.reach(n, 1)[1] < small + x.size]
    first, count = firsts[0], len(firsts)
    assert count > 3 * TILE and (first + k * rs.L) * rs.M > 2 ** 33
    near = rs.block(x, small, first, count)
    far = rs.block(x, big, first + k * rs.L, count)
    assert same_bits(far, near)
    # ... and they are the right samples: the bar of the accuracy test, against the float64 sum over the same buffer
    want = resample._block(x.astype(np.float64) / 32768.0, small, first, count, rs.L, rs.M, resample.polyphase(rs.L, rs.M)[2])
    ref_err = np.abs(R.block_f32(x, small, first, count, *rates, start=False, end=False).astype(np.float64) - want).max()
    assert np.abs(to_np(far).astype(np.float64) - want).max() <= 4.0 * ref_err


@pytest.mark.parametrize("rates", R.RATIOS[:2], ids=IDS[:2])
def test_pcm_and_tokens_are_the_host_functions_of_the_devices_own_float_output(rates):
    rs = rs_of(rates)
    for x in (pcm(rates, length_for(rates, TILE + 91)), R.square(1200)):
        y = to_np(rs(x))
        want_pcm = resample.to_pcm16(y)
        got = to_np(rs(x, out="pcm16"))
        assert got.dtype == np.int16 and np.array_equal(got, want_pcm)
        for Q in (256, 1024):
            tok = to_np(rs(x, out="tokens", quantization_steps=Q))
            assert tok.dtype == np.int32 and np.array_equal(tok, data.mulaw_encode_pcm16(want_pcm, Q))
    y, tok = to_np(rs(R.square(1200))), to_np(rs(R.square(1200), out="tokens", quantization_steps=256))
    assert y.max() > 1.0 and y.min() < -1.0 and want_pcm.max() == 32767 and want_pcm.min() == -32768
    assert tok.min() == 0 and tok.max() == 254                                             # the table's ends (32767 / 32768 < 1)


def test_equal_rates_launch_nothing_and_return_the_inputs_bits():
    rs = Resampler(16000, 16000, device="cuda")
    x = pcm((48000, 16000), 500)
    f = (x.astype(np.float32) / np.float32(32768.0))
    assert same_bits(rs(f), f) and same_bits(rs(x), f) and same_bits(rs(x, out="pcm16"), x) and rs.launches == 0
    assert np.array_equal(to_np(rs(x, out="tokens")), data.mulaw_encode_pcm16(x, 256))


def test_a_replay_of_a_captured_launch_follows_a_refilled_input_buffer():
    rates = (48000, 16000)
    rs = rs_of(rates)
    n = length_for(rates, TILE + 44)
    a, b = pcm(rates, n), R.pcm16(n, 48000, seed=77)
    want_a, want_b = rs(a), rs(b)
    x = torch.as_tensor(a).cuda()
    out = torch.full((rs.count(n),), 7.0, device="cuda")
    clip = _resample.WnResampleClip(x=x.data_ptr(), n=n, origin=0, out=out.data_ptr(), first=0, count=rs.count(n), flags=3)

    def call():
        _resample.check(_resample.lib().wn_resample(C.byref(clip), 1, _resample.WN_RESAMPLE_IN_PCM16, _resample.WN_RESAMPLE_OUT_F32,
                                                    _lib.ptr(rs.taps), rs.L, rs.M, rs.T, None, _lib.stream_ptr()))

    call()                                                                                 # (the kernel's code is loaded before the capture)
    torch.cuda.synchronize()
    assert same_bits(out, want_a)
    out.fill_(7.0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())                                     # captured, not run
    for src, want in ((b, want_b), (a, want_a)):
        x.copy_(torch.as_tensor(src))
        g.replay()
        torch.cuda.synchronize()
        assert same_bits(out, want)


def test_an_output_past_an_unflagged_end_is_earg_and_nothing_runs():
    rs = rs_of((48000, 16000))
    x = torch.as_tensor(pcm((48000, 16000), 4000)).cuda()
    out = torch.full((100,), 7.0, device="cuda")
    lib = _resample.lib()

    def call(first, count, flags):
        clip = _resample.WnResampleClip(x=x.data_ptr(), n=4000, origin=0, out=out.data_ptr(), first=first, count=count, flags=flags)
        return lib.wn_resample(C.byref(clip), 1, 0, 0, _lib.ptr(rs.taps), rs.L, rs.M, rs.T, None, _lib.stream_ptr())

    assert call(0, 100, _resample.WN_RESAMPLE_END) == _resample.WNR_EARG and b"reads input -96" in lib.wn_resample_last_error()
    assert call(1300, 10, _resample.WN_RESAMPLE_START) == _resample.WNR_EARG and b"reads input 4023" in lib.wn_resample_last_error()
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())
    assert call(32, 100, 0) == _resample.WNR_OK                                            # inputs 0 .. 489: inside, no flag needed
    assert same_bits(out, rs(x)[32:132].contiguous())


# ---- the loader and the command line -------------------------------------------------------------------------------------------------
# (the model of the log-mel driver tests -- two layers of 32 channels, the widths whose training step reproduces itself to the bit
# -- at 16 kHz, with 8 mel channels; two files at 48 kHz, one per speaker)
CFG = {"quantization_steps": 256, "sampling_rate": 16000, "causal_conv_channels": [32], "residual_conv_channels": [32] * 2,
       "residual_num_blocks": 1, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
MEL = ["--local-mel", "--mels", "8", "--win", "64", "--local-hop", "16"]
LOOP = ["--seed", "1", "--lr", "0.003", "--batch-size", "2", "--train-width", "48", "--repeat", "3", "--max-epoch", "2"]


def _train(tmp, name, wav, extra):
    from wavenet_amd.train_audio import train as cli_train
    model = tmp / name
    model.mkdir()
    (model / "wavenet.json").write_text(json.dumps(CFG))
    cli_train.main(["-w", str(wav), "-m", str(model)] + LOOP + extra)
    with np.load(str(model / "wavenet.model.npz")) as z:
        return model, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def audio(tmp_path_factory):
    """Two 48 kHz files, the 16 kHz files the tool writes from them on the device, and the checkpoints of ``train --resample``
    on the first and ``train`` on the second."""
    from scipy.io import wavfile
    from wavenet_amd.train_audio import resample as cli_resample
    tmp = tmp_path_factory.mktemp("resample_cli")
    wav48, wav16 = tmp / "wav48", tmp / "wav16"
    wav48.mkdir()
    wavfile.write(str(wav48 / "p1_a.wav"), 48000, R.pcm16(9000, 48000, seed=1))
    wavfile.write(str(wav48 / "p2_b.wav"), 48000, np.stack([R.pcm16(6300, 48000, seed=2)] * 2, axis=1))       # stereo: the left channel
    cli_resample.main(["-w", str(wav48), "-o", str(wav16), "--rate", "16000", "--device"])
    model48, w48 = _train(tmp, "m48", wav48, MEL + ["--resample"])
    model16, w16 = _train(tmp, "m16", wav16, MEL)
    return dict(tmp=tmp, wav48=wav48, wav16=wav16, model48=model48, model16=model16, w48=w48, w16=w16)


def test_the_loader_reads_a_48_khz_file_as_the_file_the_tool_wrote_from_it(audio):
    from scipy.io import wavfile
    for name, n in (("p1_a.wav", 3000), ("p2_b.wav", 2100)):
        rate, written = wavfile.read(str(audio["wav16"] / name))
        assert rate == 16000 and written.dtype == np.int16 and written.shape == (n,)
        got, r = data.load_audio_file(str(audio["wav48"] / name), rate=16000, device="cuda")
        want, r16 = data.load_audio_file(str(audio["wav16"] / name))
        assert r == r16 == 16000 and got.dtype == want.dtype and np.array_equal(got, want)
    many = data.load_audio_files([str(audio["wav48"] / "p1_a.wav"), str(audio["wav16"] / "p2_b.wav"), str(audio["wav48"] / "p2_b.wav")],
                                 16000, 256, "cuda")
    assert np.array_equal(many[1], many[2]) and np.array_equal(many[0], data.load_audio_file(str(audio["wav16"] / "p1_a.wav"))[0])


def test_training_with_resample_ends_with_the_weights_of_training_on_the_converted_files(audio):
    wa, wb = audio["w48"], audio["w16"]
    assert sorted(wa) == sorted(wb) and "local_condition_projection/W" in wa
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    for name in ("wavenet.json", "local.json"):                                            # a property of the run: nothing is stored
        assert (audio["model48"] / name).read_bytes() == (audio["model16"] / name).read_bytes()


def test_the_corpus_run_with_speakers_and_mel_features_does_too(audio, tmp_path):
    extra = ["--corpus", "--speaker-prefix", "--condition-channels", "4"] + MEL
    _, wa = _train(tmp_path, "a", audio["wav48"], extra + ["--resample"])
    _, wb = _train(tmp_path, "b", audio["wav16"], extra)
    assert sorted(wa) == sorted(wb) and "local_condition_projection/W" in wa
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k


def test_evaluate_with_resample_prints_the_numbers_of_the_converted_files(audio):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    got = cli_evaluate.main(["-w", str(audio["wav48"]), "-m", str(audio["model48"]), "--local-mel", "--resample"])
    want = cli_evaluate.main(["-w", str(audio["wav16"]), "-m", str(audio["model48"]), "--local-mel"])
    assert got == want and got["total"]["samples"] > 0


def test_features_prompt_and_keep_read_a_48_khz_file_as_the_converted_one(audio, tmp_path):
    from wavenet_amd.train_audio import args as cli_args
    from wavenet_amd.train_audio import features as cli_features
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import model as cli_model
    mel = ["--hop", "16", "--mels", "8", "--win", "64", "--device"]
    cli_features.main(["-w", str(audio["wav48"]), "-o", str(tmp_path / "a")] + mel + ["--resample", "-m", str(audio["model48"])])
    cli_features.main(["-w", str(audio["wav16"]), "-o", str(tmp_path / "b")] + mel)
    for name in ("p1_a.npy", "p2_b.npy"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    f48, f16 = str(audio["wav48"] / "p1_a.wav"), str(audio["wav16"] / "p1_a.wav")
    params = cli_model.load_params(str(audio["model48"]))
    with_flag = cli_args.parse(["-m", str(audio["model48"]), "--fast", "--keep", f48, "--redraw", "0.01:0.02", "--resample"])
    without = cli_args.parse(["-m", str(audio["model48"]), "--fast", "--keep", f16, "--redraw", "0.01:0.02"])
    a, b = cli_generate.keep_job(with_flag, False), cli_generate.keep_job(without, False)
    assert np.array_equal(a[1][0], b[1][0]) and np.array_equal(a[2][0], b[2][0]) and a[1][0].size > 2900
    assert cli_generate.read_kw(without, params) == {}
    assert np.array_equal(cli_generate.read_prompt(f48, params, cli_generate.read_kw(with_flag, params)),
                          cli_generate.read_prompt(f16, params))


def test_copy_synthesis_from_a_48_khz_recording_is_that_of_the_converted_file(audio, tmp_path):
    from wavenet_amd.train_audio import generate as cli_generate

    def run(name, extra):
        out = tmp_path / name
        _, tokens = cli_generate.main(["-m", str(audio["model48"]), "-o", str(out), "--fast", "--seed", "3", "-s", "0.02"] + extra)
        return np.asarray(tokens), (out / "generated.wav").read_bytes()

    want = run("f16", ["--from-wav", str(audio["wav16"] / "p1_a.wav")])
    got = run("f48", ["--from-wav", str(audio["wav48"] / "p1_a.wav"), "--resample"])
    assert got[0].size > 0 and np.array_equal(got[0], want[0]) and got[1] == want[1]
    chunked = run("f48c", ["--from-wav", str(audio["wav48"] / "p1_a.wav"), "--resample", "--chunk-frames", "400"])
    assert np.array_equal(chunked[0], want[0])
