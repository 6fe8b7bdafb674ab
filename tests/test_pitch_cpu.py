"""The host side of the pitch tracker: the numpy definition against truth, the float32 restatement's decisions against the
definition's on every frame of every test signal, selection in both precisions, and the ABI's names and refusals (no GPU
needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pitch_ref as P
from wavenet_amd import _pitch, features, pitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(zip(P.SHAPES, P.LAGS))


def test_pitch_lags_are_floor_and_ceil_and_refuse_a_range_too_small():
    for (rate, _, _, fmin, fmax, _), lags in CASES:
        assert pitch.pitch_lags(rate, fmin, fmax) == lags
    assert pitch.pitch_lags(16000) == (32, 267) and pitch.pitch_lags(22050, 60.0, 500.0) == (44, 368)
    with pytest.raises(ValueError, match="tau_min = .* = 1 < 2"):
        pitch.pitch_lags(1600, 400.0, 1000.0)
    with pytest.raises(ValueError, match="tau_max = .* = 3 below tau_min \\+ 2 = 4"):
        pitch.pitch_lags(1600, 600.0, 800.0)


@pytest.mark.parametrize("f", [102.0, 178.4, 415.0])
def test_a_harmonic_tone_is_voiced_on_every_interior_frame_and_its_f0_is_within_1e_3(f):
    """The prototype measured at most 1.2e-4 (at 415 Hz); 1e-3 is under 2 cents."""
    rate, n = 16000, 12000
    out = pitch.yin(P.harmonic_tone(f, rate, n), rate)
    assert out.shape == (2, features.frame_count(n, 256)) and out.dtype == np.float64
    S = 1024 + 267
    inside = [k for k in range(out.shape[1]) if k * 256 - S // 2 >= 0 and k * 256 - S // 2 + S <= n]
    assert len(inside) > 30
    rel = np.abs(out[0, inside] / f - 1.0)
    print("%.1f Hz: largest relative F0 error %.3g over %d interior frames" % (f, rel.max(), len(inside)))
    assert (out[0, inside] > 0).all() and (out[1, inside] < 0.15).all()
    assert rel.max() <= 1e-3


def test_noise_and_silence_are_never_voiced_and_a_constant_gives_one_everywhere():
    noise = np.random.RandomState(3).randn(12000) * 0.3
    out = pitch.yin(noise, 16000)
    print("white noise: smallest aperiodicity %.3f" % out[1].min())
    assert (out[0] == 0).all() and out[1].min() > 0.15
    for x in (np.zeros(3000), np.full(3000, 0.25)):
        c = pitch.yin_curve(x, 16000)
        S = 1024 + 267
        inside = [k for k in range(c.shape[0]) if k * 256 - S // 2 >= 0 and k * 256 - S // 2 + S <= x.size]
        rows = c if x[0] == 0 else c[inside]                            # a constant's edge frames see the step to zero
        assert (rows == 1.0).all()
        out = pitch.yin(x, 16000)
        assert (out[0] == 0).all() and (out[1, inside] == 1.0).all()


def test_the_curve_is_the_double_loop_of_the_definition_and_frames_are_zero_outside():
    (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) = CASES[1]
    x = P.chirp_signal(n, tau_min, tau_max)
    c = pitch.yin_curve(x, rate, hop, win, fmin, fmax)
    S = win + tau_max
    assert c.shape == (features.frame_count(n, hop), tau_max + 1)
    for k in (0, 7, c.shape[0] - 1):
        s = np.array([x[i] if 0 <= i < n else 0.0 for i in range(k * hop - S // 2, k * hop - S // 2 + S)])
        d = np.array([sum((s[j] - s[j + tau]) ** 2 for j in range(win)) for tau in range(tau_max + 1)])
        want, run = np.ones(tau_max + 1), 0.0
        for tau in range(1, tau_max + 1):
            run += d[tau]
            want[tau] = d[tau] * tau / run if run > 0 else 1.0
        assert np.abs(c[k] - want).max() < 1e-12
    out = pitch.yin(x, rate, hop, win, fmin, fmax)
    taus, sel = pitch.yin_select(c, tau_min, 0.15, rate)
    assert np.array_equal(out, sel) and np.array_equal(out[0] > 0, out[1] < 0.15)
    assert taus.min() >= tau_min and taus.max() <= tau_max - 1
    assert (out[0] > 0).sum() >= 4 and (out[0] == 0).sum() >= 4


def test_selection_walks_to_the_local_minimum_takes_the_first_argmin_and_refines_a_parabola():
    c = np.ones((3, 12))
    c[0, [4, 5, 6, 7]] = [0.14, 0.10, 0.05, 0.09]                        # first below at 4, walked to 6
    c[0, 9] = 0.01                                                       # a deeper dip later is not taken
    c[1, [3, 8]] = 0.5                                                   # none below: the first of two equal minima
    c[2, 2:11] = 0.2 + 0.01 * (np.arange(2, 11) - 6.3) ** 2              # a parabola with its minimum at 6.3: unvoiced, refined
    for dt in (np.float64, np.float32):
        taus, out = pitch.yin_select(c, 2, 0.15, 1200.0, dt)
        assert out.dtype == dt and taus.tolist() == [6, 3, 6]
        assert out[0, 1] == 0 and out[0, 2] == 0 and out[1].tolist() == [dt(0.05), dt(0.5), c.astype(dt)[2, 6]]
        shift = 0.5 * (0.10 - 0.09) / (0.10 - 0.10 + 0.09)
        assert abs(out[0, 0] - 1200.0 / (6 + shift)) < 1e-3
    c[2] -= 0.1                                                          # the same parabola below the threshold
    assert abs(pitch.yin_select(c, 2, 0.15, 1200.0)[1][0, 2] - 1200.0 / 6.3) < 1e-9
    flat = np.ones((1, 12))
    taus, out = pitch.yin_select(flat, 2, 0.15, 1200.0)                  # den = 0: no shift
    assert taus.tolist() == [2] and out[0, 0] == 0 and out[1, 0] == 1


@pytest.mark.parametrize("shape,lags", CASES, ids=P.IDS)
def test_the_float32_restatement_decides_as_the_definition_on_every_frame(shape, lags):
    """tau* and voicing of every frame: what makes the GPU tests' cap of 1 frame in 50 fair."""
    rate, win, hop, fmin, fmax, n = shape
    tau_min, tau_max = lags
    x = P.chirp_signal(n, tau_min, tau_max).astype(np.float32)
    c64, c32 = pitch.yin_curve(x, rate, hop, win, fmin, fmax), P.yin_curve_f32(x, hop, win, tau_max)
    t64, o64 = pitch.yin_select(c64, tau_min, P.THRESHOLD, rate)
    t32, o32 = pitch.yin_select(c32, tau_min, P.THRESHOLD, rate, np.float32)
    bar, err = P.bar(x, hop, win, tau_max)
    print("%s: float32 restatement within %.3g of the curve (bar %.3g), %d of %d frames voiced"
          % (shape, err, bar, (o64[0] > 0).sum(), t64.size))
    assert np.array_equal(t64, t32) and np.array_equal(o64[0] > 0, o32[0] > 0)
    t32_64, o32_64 = pitch.yin_select(c32, tau_min, P.THRESHOLD, rate, np.float64)       # the same curve in both precisions
    assert np.array_equal(t32_64, t32) and np.array_equal(o32_64[0] > 0, o32[0] > 0)
    assert np.array_equal(o32[1], c32[np.arange(t32.size), t32])
    fbar, _, _ = P.f0_bar(c32, tau_min, rate)
    assert fbar.shape == (t32.size,) and (fbar > 0).all()


# ---- the library: names, refusals ------------------------------------------------------------------------------------------------
def test_header_map_and_binding_name_the_same_three_functions():
    hdr = open(os.path.join(ROOT, "include", "wavenet_pitch.h")).read()
    declared = set(re.findall(r"\b(wn_pitch[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_pitch.EXPORTS) == {"wn_pitch_abi_version", "wn_pitch_last_error", "wn_pitch"}
    assert "wn_pitch*" in open(os.path.join(ROOT, "wavenet_amd", "csrc", "analysis", "pitch_exports.map")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _pitch.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in nm.splitlines() if ln.strip()} == declared
    assert _pitch.lib().wn_pitch_abi_version() == _pitch.ABI_VERSION == int(re.search(r"#define WN_PITCH_ABI_VERSION (\d+)", hdr).group(1))
    for name in ("WN_PITCH_MAX_CLIPS", "WN_PITCH_START", "WN_PITCH_END", "WNP_OK", "WNP_EARG", "WNP_EHIP"):
        assert int(re.search(r"#define %s\s+(-?\d+)" % name, hdr).group(1)) == getattr(_pitch, name), name
    assert _pitch.WN_PITCH_MAX_CLIPS == pitch.PITCH_MAX_CLIPS
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct WnPitchClip \{(.*?)\} WnPitchClip;", hdr, re.S).group(1), flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _pitch.WnPitchClip._fields_]
    assert C.sizeof(_pitch.WnPitchClip) == 6 * 8 + 4 * 4
    assert "getenv" not in open(os.path.join(ROOT, "wavenet_amd", "csrc", "analysis", "pitch.hip")).read()


def test_wn_pitch_refuses_every_bad_argument_by_name_without_a_gpu():
    lib = _pitch.lib()
    EARG = _pitch.WNP_EARG

    def clip(**kw):
        d = dict(x=64, n=700, origin=0, out=64, out_stride=44, curve=None, first=0, count=44, flags=3)
        d.update(kw)
        return C.byref(_pitch.WnPitchClip(**d))

    def call(cl, n_clips=1, table=None, Q=0, win=64, hop=16, tau_min=4, tau_max=40, threshold=0.15, rate=1600.0):
        return lib.wn_pitch(cl, n_clips, table, Q, win, hop, tau_min, tau_max, threshold, rate, None)

    assert call(None) == EARG and b"NULL" in lib.wn_pitch_last_error()
    for kw, word in [(dict(win=15), b"win = 15"), (dict(win=4097), b"win = 4097"), (dict(hop=0), b"hop = 0"),
                     (dict(tau_min=1), b"tau_min = 1"), (dict(tau_max=5), b"tau_max = 5"), (dict(tau_max=2048), b"tau_max = 2048"),
                     (dict(hop=8000), b"bytes of LDS"), (dict(n_clips=0), b"n_clips = 0"), (dict(n_clips=65), b"n_clips = 65"),
                     (dict(table=64, Q=0), b"Q = 0")]:
        assert call(clip(), **kw) == EARG, kw
        assert word in lib.wn_pitch_last_error(), (kw, lib.wn_pitch_last_error())
    # S = 104: frame 0 reads samples -52 .. 51, frame 43 reads 636 .. 739 of 700
    for kw, word in [(dict(out_stride=43), b"out_stride = 43"), (dict(first=-1), b"first = -1"), (dict(count=-2), b"count = -2"),
                     (dict(flags=4), b"flags = 4"), (dict(x=None), b"NULL buffer"), (dict(out=None), b"NULL buffer"),
                     (dict(flags=2), b"frame 0 reads sample -52, before the buffer"),
                     (dict(flags=1), b"frame 43 reads sample 739 of 700"),
                     (dict(flags=0, origin=52, count=40), b"frame 39 reads sample 727 of 700"),
                     (dict(flags=0, origin=51, count=4), b"frame 0 reads sample -1, before the buffer")]:
        assert call(clip(**kw)) == EARG, kw
        assert word in lib.wn_pitch_last_error(), (kw, lib.wn_pitch_last_error())
    from wavenet_amd import _lib
    with pytest.raises(_lib.WaveNetHipError, match="tau_max = 2048"):
        _pitch.check(call(clip(), tau_max=2048))
    assert call(clip(count=0, x=None, out=None, out_stride=0)) == _pitch.WNP_OK      # nothing to do: nothing is launched


def test_the_python_face_names_what_the_kernel_refuses_before_device_work():
    assert pitch._device_refusal(1024, 256, 32, 267) is None and pitch._device_refusal(4096, 512, 2, 2047) is None
    assert "win = 8" in pitch._device_refusal(8, 16, 4, 40)
    assert "hop = 0" in pitch._device_refusal(64, 0, 4, 40)
    assert "tau_max = 2048" in pitch._device_refusal(64, 16, 4, 2048)
    assert "bytes of LDS" in pitch._device_refusal(64, 8000, 4, 40)
    assert pitch.pitch_tile_frames(267) == 6 and pitch.pitch_tile_frames(40) == 8 and pitch.pitch_tile_frames(2047) == 1
    with pytest.raises(ValueError, match="win = 8192"):
        pitch.Pitch(16000, win=8192, device="cpu")
    with pytest.raises(ValueError, match="tau_max = 3200"):
        pitch.Pitch(16000, fmin=5.0, device="cpu")
    with pytest.raises(ValueError, match="tau_min = .* < 2"):
        pitch.Pitch(1600, fmax=1000.0, device="cpu")
    p = pitch.Pitch(1600, 16, 64, 40.0, 400.0, device="cpu")          # no device work yet: the refusals below come before any
    assert (p.tau_min, p.tau_max, p.span, p.launches) == (4, 40, 104, 0)
    with pytest.raises(ValueError, match="needs quantization_steps"):
        p(np.zeros(100, np.int32))
    with pytest.raises(ValueError, match="columns 0 .. 3 read samples -52 .. 99"):
        p.block(np.zeros(700, np.float32), 0, 0, 4)
    with pytest.raises(ValueError, match="columns 40 .. 44 of a clip that has 44"):
        p.frames(np.zeros(700, np.float32), 40, 5)
    assert p.launches == 0
