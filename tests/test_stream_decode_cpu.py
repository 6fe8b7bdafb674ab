"""Streaming synthesis without a GPU: the descriptor flag in the header and the binding (and an ABI that did not move), the
arithmetic of a frame ring held to a brute-force walk, the dealing of a large stream to launches, the refusals of ``push`` /
``pull`` / ``open_stream`` -- on books and models that never touch a device --, the growing .wav file, and the command line's
refusals before a model is built."""
import os
import re

import numpy as np
import pytest

import local_cond_ref as LR
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib, data
from wavenet_amd.faster_wavenet import StreamBook, deal_launches, stream_frames
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_defines_the_bit_as_1024_and_the_abi_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.findall(r"^#define\s+WN_DECODER_FRAME_RING\s+(\d+)u", hdr, flags=re.M) == ["1024"]
    assert _lib.WN_DECODER_FRAME_RING == 1024
    others = {k: v for k, v in vars(_lib).items() if re.match(r"WN_(EXEC|DECODER)_", k) and k not in
              ("WN_DECODER_FRAME_RING", "WN_DECODER_BATCH_MAX_ANY")}
    assert others and all(isinstance(v, int) and not (v & 1024) for v in others.values()), others
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 69
    assert _lib.ABI_VERSION == 5 == int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1))


def _walk(hop, lin, phase, fed, done, pull):
    """The same four answers by walking steps one at a time: step k reads frame (phase + k) // hop, and the next with lin."""
    def reads(k):
        j = (phase + k) // hop
        return {j, j + 1} if lin else {j}
    steps = 0
    while max(reads(done + steps)) < fed:
        steps += 1
    touched = set()
    for k in range(done, done + pull):
        touched |= reads(k)
    worst = 0
    for start in range(hop):                      # a run may start anywhere inside a frame
        t = set()
        for k in range(start, start + pull):
            t |= ({k // hop, k // hop + 1} if lin else {k // hop})
        worst = max(worst, len(t))
    return steps, (phase + done) // hop, len(touched), worst


@pytest.mark.parametrize("hop", [1, 3, 4])
@pytest.mark.parametrize("lin", [False, True], ids=["repeat", "linear"])
def test_the_ring_arithmetic_is_the_brute_force_walk(hop, lin):
    for phase in range(hop):
        for fed in range(0, 6):
            for done in range(0, 4 * hop + 2):
                for pull in (0, 1, 2, 3, hop, hop + 1, 2 * hop, 2 * hop + 1, 7):
                    got = stream_frames(hop, lin, phase, fed, done, pull)
                    steps, cur, touched, worst = _walk(hop, lin, phase, fed, done, pull)
                    # (steps already run past the frames fed leave nothing to run: never negative)
                    assert got.steps == max(0, steps) and got.current == cur, (phase, fed, done, pull, got)
                    assert got.reads == touched and got.min_ring == worst, (phase, fed, done, pull, got)
                    assert got.reads <= got.min_ring
    for bad in (dict(hop=0), dict(phase=hop), dict(phase=-1), dict(fed=-1), dict(done=-1), dict(pull=-1)):
        with pytest.raises(ValueError, match="stream_frames"):
            stream_frames(**dict(dict(hop=hop, linear=lin, phase=0), **bad))


def test_a_large_stream_is_dealt_to_launches():
    """Equal step counts for every utterance of a pull: launches of the limit in the caller's order, every index once."""
    for n, limit in ((1, 28), (28, 28), (29, 28), (60, 28), (1025, 1024)):
        got = deal_launches([7] * n, limit)
        assert [c for c, _ in got] == [7] * ((n + limit - 1) // limit)
        assert [i for _, idx in got for i in idx] == list(range(n)) and max(len(idx) for _, idx in got) <= limit


def test_pull_deals_its_utterances_with_deal_launches():
    """(What the dealing does to a stream of more utterances than a launch takes is a GPU test; here: it is the one function.)"""
    import inspect
    from wavenet_amd.faster_wavenet import DecodeStream
    src = inspect.getsource(DecodeStream.pull)
    assert "deal_launches([steps] * N, limit)" in src and "wn_decoder_batch_max()" in src and "WN_DECODER_BATCH_MAX_ANY" in src


def test_books_refuse_push_and_pull_with_their_messages():
    b = StreamBook([1, 3], hop=4, linear=True, ring=3, two_steps=False)
    assert b.available() == [1, 1]                                     # nothing fed: the prefill's sample alone
    with pytest.raises(Exception, match=r"push: 1 arrays for 2 utterances"):
        b.check_push([1])
    with pytest.raises(Exception, match=r"utterance 1: 4 more rows on top of the 0 fed would overwrite a row not yet consumed: the ring holds "
                                        r"3 rows and the decoder has consumed 0"):
        b.check_push([3, 4])
    b.check_push([3, 2])
    b.pushed([3, 2])
    # linear: 3 frames fed carry the steps of frames 0 and 1 -- 8 positions less the phase; 2 frames those of frame 0
    assert b.available() == [1 + 7, 1 + 1]
    with pytest.raises(Exception, match=r"pull: utterance 1: 3 samples asked for, the rows present allow 2 \(2 frames fed, 0 steps run, hop 4, "
                                        r"phase 3; linear interpolation reads the frame after a step's own\): push more first"):
        b.check_pull(3)
    with pytest.raises(Exception, match="n must be positive"):
        b.check_pull(0)
    assert b.check_pull(2) == 1                                         # the first pull: element 0 is the prefill's
    b.pulled(1)
    assert b.done == [1, 1] and b.available() == [6, 0]
    with pytest.raises(Exception, match=r"utterance 0: 2 more rows on top of the 3 fed"):
        b.check_push([2, 1])                                            # utterance 0 still reads frame 0
    b.check_push([0, 1])
    b.pushed([0, 1])
    assert b.available() == [6, 4] and b.check_pull(4) == 4
    # a pull that reads more frames at once than the ring holds: 9 steps from phase 3 read frames 0 .. 2 and, linear, 3
    big = StreamBook([3], hop=4, linear=True, ring=3)
    big.fed = [9]
    with pytest.raises(Exception, match=r"utterance 0: 10 samples read 4 frames at once, the ring holds 3"):
        big.check_pull(10)
    # the nine-workgroup decoder: no pull of exactly one step
    nine = StreamBook([0], hop=4, ring=8, two_steps=True)
    nine.pushed([8])
    with pytest.raises(Exception, match=r"ONE decoder step.*n >= 2 per launch.*pull 1, or 3 and more"):
        nine.check_pull(2)
    assert nine.check_pull(1) == 0 and nine.check_pull(3) == 2
    nine.pulled(2)
    with pytest.raises(Exception, match=r"ONE decoder step.*pull 2 and more"):
        nine.check_pull(1)
    assert nine.check_pull(2) == 2
    # no ring: nothing to push, nothing to wait for
    free = StreamBook([0, 0])
    assert free.available() == [None, None] and free.check_pull(5) == 4
    with pytest.raises(Exception, match="has no ring"):
        free.check_push([1, 1])


def test_open_stream_refuses_before_any_device_work():
    p = R.make_params(**LR.TINY)
    net = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=4, local_interp="linear")    # never moved to a device
    W = net.input_width
    h = np.zeros((LR.FEATS, W // 4 + 3), np.float32)
    with pytest.raises(Exception, match="locally conditioned"):
        net.open_stream()
    with pytest.raises(Exception, match="utterances must be positive"):
        net.open_stream(utterances=0, local=h)
    with pytest.raises(Exception, match=r"local= holds 2 feature arrays for 3 utterances"):
        net.open_stream(utterances=3, local=[h, h])
    with pytest.raises(Exception, match="feature columns"):
        net.open_stream(local=h[:, :2])                                 # the window is not covered
    # 9 samples at hop 4 read up to ceil(8 / 4) + 1 frames, linear one more
    assert stream_frames(4, True, 0, pull=9).min_ring == 4
    with pytest.raises(Exception, match=r"ring_frames = 3 is too small for max_pull = 9.*reads up to 4 frames at once \(linear "
                                        r"interpolation: one more\), the minimum"):
        net.open_stream(local=h, ring_frames=3, max_pull=9)
    with pytest.raises(Exception, match="max_pull must be positive"):
        net.open_stream(local=h, max_pull=0)
    plain = FasterWaveNet(Params(p), seed=0)
    with pytest.raises(Exception, match="no local conditioning"):
        plain.open_stream(ring_frames=8)
    with pytest.raises(Exception, match="no local conditioning"):
        plain.open_stream(local=h)


def test_the_growing_wav_is_the_file_save_audio_file_writes(tmp_path):
    tokens = np.random.RandomState(3).randint(0, 256, (1001,)).astype(np.int32)
    data.save_audio_file(str(tmp_path / "whole.wav"), tokens, 256, format="16bit_pcm", sampling_rate=16000)
    w = cli_generate._GrowingWav(str(tmp_path / "grown.wav"), 256, 16000)
    for a, b in ((0, 1), (1, 300), (300, 1001)):
        w.append(tokens[a:b])
    w.close()
    assert (tmp_path / "grown.wav").read_bytes() == (tmp_path / "whole.wav").read_bytes()


def test_the_command_line_refuses_before_a_model_is_built(tmp_path, monkeypatch):
    def no_model(*a, **kw):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli_generate._model, "build", no_model)
    m = str(tmp_path / "model")
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(["-m", m, "--local", "a.npy", "--chunk-frames", "4"])
    with pytest.raises(SystemExit, match="give --local FILE.npy"):
        cli_generate.main(["-m", m, "--fast", "--chunk-frames", "4"])
    with pytest.raises(SystemExit, match="give --chunk-frames C"):
        cli_generate.main(["-m", m, "--fast", "--local", "a.npy", "--ring-frames", "40"])
    with pytest.raises(SystemExit, match="C >= 1, got 0"):
        cli_generate.main(["-m", m, "--fast", "--local", "a.npy", "--chunk-frames", "0"])
    with pytest.raises(SystemExit, match="R >= 1, got -2"):
        cli_generate.main(["-m", m, "--fast", "--local", "a.npy", "--chunk-frames", "4", "--ring-frames", "-2"])
    for extra in (["--utterances", "2"], ["--prompt", "p.wav"], ["--keep", "k.wav"]):
        with pytest.raises(SystemExit, match="do not go with it"):
            cli_generate.main(["-m", m, "--fast", "--local", "a.npy", "--chunk-frames", "4"] + extra)
    assert not os.path.exists(m)
    assert cli_generate.stream_job(cli_args.parse(["--fast", "--local", "a.npy", "--chunk-frames", "4", "--ring-frames", "40"])) == (4, 40)
    assert cli_generate.stream_job(cli_args.parse(["--fast", "--local", "a.npy"])) == (None, None)


def test_a_command_line_without_the_new_flags_parses_as_before():
    for argv in ([], ["--fast", "--best-of", "4", "--report", "r.json"], ["--fast", "--local", "a.npy", "--speaker", "p225"]):
        a = cli_args.parse(argv)
        assert a.chunk_frames is None and a.ring_frames is None and "chunk_frames" not in vars(a) and "ring_frames" not in vars(a)
    text = " ".join(cli_args.build_parser().format_help().split())
    assert "--chunk-frames" in text and "--ring-frames" in text
