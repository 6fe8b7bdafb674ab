"""Pitch on the device (wn_pitch, pitch.Pitch) against the numpy definition, and the bit contract: a column's bits depend on its
own samples and the parameters only -- not on tile mates, batch mates, the call, `first` or `origin`, or tokens versus floats."""
import numpy as np
import pytest
import torch

import pitch_ref as P
from gpu_util import to_np
from wavenet_amd import data, features, pitch
from wavenet_amd.pitch import Pitch

pytestmark = pytest.mark.gpu
CASES = list(zip(P.SHAPES, P.LAGS))

_REF = {}


def ref(i):
    """Per shape, computed once and left unchanged: the signal, the definition's curve and selection, the device's outputs."""
    if i not in _REF:
        (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[i]
        x = P.chirp_signal(n, tau_min, tau_max).astype(np.float32)
        p = Pitch(rate, hop, win, fmin, fmax, P.THRESHOLD)
        assert (p.tau_min, p.tau_max) == (tau_min, tau_max)
        out, curve = p.analyse(x)
        c64 = pitch.yin_curve(x, rate, hop, win, fmin, fmax)
        t64, o64 = pitch.yin_select(c64, tau_min, P.THRESHOLD, rate)
        _REF[i] = dict(x=x, p=p, out=to_np(out), curve=to_np(curve), c64=c64, t64=t64, o64=o64)
    return _REF[i]


def same_bits(a, b):
    a, b = [v if isinstance(v, np.ndarray) else to_np(v) for v in (a, b)]
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=P.IDS)
def test_every_cell_of_the_curve_is_within_four_float32_restatement_errors_of_the_definition(i):
    """Bar per shape: 4 x the error of tests/pitch_ref.py (float32 sums in numpy) against pitch.yin_curve on the same input, at
    least 16 float32 spacings at 1.0.  Every cell counts."""
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[i]
    r = ref(i)
    bar, ref_err = P.bar(r["x"], hop, win, tau_max)
    assert r["curve"].shape == r["c64"].shape == (features.frame_count(n, hop), tau_max + 1)
    err = float(np.abs(r["curve"].astype(np.float64) - r["c64"]).max())
    print("pitch %d/%d/%d..%d/%d: device %.3g, float32 restatement %.3g, bar %.3g" % (win, hop, tau_min, tau_max, n, err, ref_err, bar))
    assert np.isfinite(r["curve"]).all() and (r["curve"][:, 0] == 1.0).all()
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("i", range(len(CASES)), ids=P.IDS)
def test_selection_on_the_kernels_own_curve_is_yin_select_in_float32(i):
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[i]
    r = ref(i)
    out, curve = r["out"], r["curve"]
    t32, o32 = pitch.yin_select(curve, tau_min, P.THRESHOLD, rate, np.float32)
    assert out.shape == (2, features.frame_count(n, hop)) and out.dtype == np.float32
    assert same_bits(out[1], curve[np.arange(t32.size), t32])                   # row 1 is curve[k, tau*]: the same tau*
    assert np.array_equal(out[0] > 0, o32[0] > 0)
    assert np.array_equal(out[0] > 0, out[1] < np.float32(P.THRESHOLD))
    fbar, t64, o64 = P.f0_bar(curve, tau_min, rate)
    assert np.array_equal(t64, t32)
    err = np.abs(out[0].astype(np.float64) - o64[0])
    print("F0 on the kernel's curve: largest error %.3g Hz, smallest slack %.3g Hz" % (err.max(), (fbar - err).min()))
    assert (err <= fbar).all(), (err, fbar)


@pytest.mark.parametrize("i", range(len(CASES)), ids=P.IDS)
def test_decisions_end_to_end_differ_from_the_definitions_on_at_most_one_frame_in_fifty(i):
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[i]
    r = ref(i)
    out, curve, t64, o64 = r["out"], r["curve"], r["t64"], r["o64"]
    tdev, _ = pitch.yin_select(curve, tau_min, P.THRESHOLD, rate, np.float32)    # the kernel's tau* (the test above)
    flips = (tdev != t64) | ((out[0] > 0) != (o64[0] > 0))
    print("%d of %d frames decide otherwise than the definition" % (flips.sum(), flips.size))
    assert 50 * int(flips.sum()) <= flips.size
    fbar, _, _ = P.f0_bar(curve, tau_min, rate)
    both = ~flips & (o64[0] > 0)
    k = np.flatnonzero(both)                                                 # voiced in both, the same tau*
    if k.size:
        err = np.abs(out[0, k].astype(np.float64) - o64[0, k])
        print("F0 against the definition: largest error %.3g Hz over %d voiced frames, bars %.3g .. %.3g Hz, largest error / bar %.3g"
              % (err.max(), k.size, fbar[k].min(), fbar[k].max(), (err / fbar[k]).max()))
        assert (err <= fbar[k]).all(), (err, fbar[k])


def test_a_batch_is_its_single_calls_in_one_launch_and_a_column_range_is_those_columns():
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[0]
    p = ref(0)["p"]
    clips = [P.chirp_signal(m, tau_min, tau_max, seed=m).astype(np.float32) for m in (700, 1001, 33)]
    before = p.launches
    outs = p.batch(clips)
    assert p.launches == before + 1
    singles = [p(c) for c in clips]
    for o, s in zip(outs, singles):
        assert same_bits(o, s)
    assert same_bits(singles[0], p.batch([clips[1], clips[0]])[1])
    full, total = singles[1], features.frame_count(1001, hop)
    assert pitch.pitch_tile_frames(tau_max) == 8
    for a, b in [(0, 3), (6, 19), (total - 3, total)]:                       # the start, across tile borders, the end
        assert same_bits(p.frames(clips[1], a, b - a), full[:, a:b].contiguous())


def test_the_production_shape_in_ranges_that_cut_its_tiles_of_six():
    r = ref(4)
    p, x, total = r["p"], r["x"], r["out"].shape[1]
    assert pitch.pitch_tile_frames(p.tau_max) == 6 and total == 32
    for a, b in [(0, 2), (2, 9), (total - 5, total)]:
        assert same_bits(p.frames(x, a, b - a), np.ascontiguousarray(r["out"][:, a:b]))


@pytest.mark.parametrize("i", [0, 1], ids=P.IDS[:2])
def test_tokens_and_their_decoded_floats_give_the_same_bits(i):
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[i]
    p = ref(i)["p"]
    tok = torch.as_tensor(data.mulaw_encode(P.chirp_signal(n, tau_min, tau_max), 256)).cuda()
    floats = data.mulaw_decode_device(tok, 256)
    out = p(floats)
    assert int((out[0] > 0).sum()) >= 4 and int((out[0] == 0).sum()) >= 4
    assert same_bits(p(tok, 256), out) and same_bits(p.curve(tok, 256), p.curve(floats))


def test_a_buffer_that_starts_inside_the_signal_gives_the_columns_it_can_serve():
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[0]
    r = ref(0)
    p, x = r["p"], r["x"]
    lo, hi = 100, 600                                                        # the buffer is x[100:600]
    first = -(-(lo + p.span // 2) // hop)                                    # the first column whose span starts at or behind lo
    last = (hi - p.span + p.span // 2) // hop                                # the last whose span ends before hi
    assert p.reach(first * hop - lo, 0, last - first + 1)[0] >= 0 and p.reach(first * hop - lo, 0, last - first + 1)[1] < hi - lo
    got = p.block(x[lo:hi], first * hop - lo, 0, last - first + 1)           # origin > 0, edges unflagged
    assert first * hop - lo > 0 and same_bits(got, np.ascontiguousarray(r["out"][:, first:last + 1]))
    got = p.block(x[lo:hi], -lo, first, last - first + 1)                    # the same columns by their own numbers: origin < 0
    assert same_bits(got, np.ascontiguousarray(r["out"][:, first:last + 1]))
    tail = p.block(x[lo:], -lo, first, r["out"].shape[1] - first, end=True)  # the signal's end is the buffer's
    assert same_bits(tail, np.ascontiguousarray(r["out"][:, first:]))


def test_refusals_come_before_device_work():
    p = ref(0)["p"]
    x = ref(0)["x"]
    before = p.launches
    with pytest.raises(ValueError, match="bytes of LDS"):
        Pitch(1600, 8000, 64, 40.0, 400.0)
    with pytest.raises(ValueError, match="win = 8"):
        Pitch(1600, 16, 8, 40.0, 400.0)
    with pytest.raises(ValueError, match="read samples -4 .. 115"):
        p.block(x[:500], 48, 0, 2)
    with pytest.raises(ValueError, match="the buffer holds 0 .. 499"):
        p.block(x[:500], 52, 0, 40, start=True)
    assert p.launches == before
    assert p.batch([]) == [] and p.launches == before
