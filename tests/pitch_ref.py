"""A float32 numpy restatement of the device pitch tracker (wavenet_amd/csrc/analysis/pitch.hip): the same sums in the same
order, every operation in float32 -- what float32 arithmetic costs against ``pitch.yin_curve`` (float64), which is how the GPU
tests size their bar -- and the shapes and test signals those tests share."""
import numpy as np

from wavenet_amd import data, features, pitch

# (rate, win, hop, fmin, fmax, n) and the lags they give: the smallest shape; S odd, hop no divisor of win; three lags at hop 1;
# a clip shorter than one segment; one production shape (more than one workgroup, a ragged last tile, 67 groups of lags)
SHAPES = [(1600, 64, 16, 40.0, 400.0, 700), (1600, 96, 40, 26.4, 320.0, 1001), (1600, 16, 1, 400.0, 800.0, 40),
          (1600, 64, 16, 40.0, 400.0, 33), (16000, 1024, 256, 60.0, 500.0, 8000)]
LAGS = [(4, 40), (5, 61), (2, 4), (4, 40), (32, 267)]
IDS = ["64-16", "96-40", "16-1", "n33", "1024-256"]
THRESHOLD = 0.15
SPACING = 2.0 ** -23                   # the float32 spacing at 1.0


def chirp_signal(n: int, tau_min: int, tau_max: int, seed: int = 0) -> np.ndarray:
    """Voiced, noisy and silent columns: a harmonic chirp (three partials, 1 / h amplitudes) whose period starts at about
    tau_max / 2 samples and shortens by a tenth, plus weak noise over the first half, gated off for a stretch inside it; noise alone up to 80 %;
    the last fifth zero.  Through mu-law at Q = 256 and back, so that tokens exist (float64; the tests round to float32 once)."""
    rs = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64)
    half = n // 2
    f_lo = 1.0 / max(0.5 * tau_max, tau_min + 1.0)                  # cycles per sample; a slow chirp: a frame stays periodic
    f_hi = 1.1 * f_lo
    phase = 2 * np.pi * (f_lo * t + 0.5 * (f_hi - f_lo) * t * t / max(half, 1))
    tone = sum(np.sin(h * phase) / h for h in (1, 2, 3) if h * f_hi < 0.45) * 0.4
    gate = (t < half) & ~((t >= 0.2 * n) & (t < 0.27 * n))
    x = np.where(gate, tone, 0.0) + np.where(t < half, 0.004 * rs.randn(n), 0.0)
    x = x + np.where((t >= half) & (t < n - n // 5), 0.2 * rs.randn(n), 0.0)
    x[n - n // 5:] = 0.0
    return data.mulaw_decode(data.mulaw_encode(np.clip(x, -1.0, 1.0), 256), 256)


def harmonic_tone(f: float, rate: float, n: int) -> np.ndarray:
    t = np.arange(n) / float(rate)
    return 0.3 * sum(np.sin(2 * np.pi * h * f * t) / h for h in (1, 2, 3))


def yin_curve_f32(signal, hop: int, win: int, tau_max: int) -> np.ndarray:
    """(frames, tau_max + 1) float32: d summed over j ascending, r over tau ascending, c = d * tau / r, all in float32."""
    x = np.asarray(signal, dtype=np.float32).reshape(-1)
    fr = pitch.yin_frames(x, hop, win, tau_max)
    lag = np.arange(tau_max + 1)
    d = np.zeros((fr.shape[0], tau_max + 1), dtype=np.float32)
    for j in range(win):
        diff = fr[:, j:j + 1] - fr[:, j + lag]
        d += diff * diff
    r = np.zeros_like(d)
    run = np.zeros(fr.shape[0], dtype=np.float32)
    for tau in range(1, tau_max + 1):
        run = run + d[:, tau]
        r[:, tau] = run
    c = np.ones_like(d)
    ok = r > 0
    ok[:, 0] = False
    c[ok] = (d * lag.astype(np.float32)[None, :])[ok] / r[ok]
    assert c.dtype == np.float32
    return c


def bar(signal32, hop: int, win: int, tau_max: int):
    """(bar, error of the float32 restatement): 4 x that error against ``yin_curve``, never below 16 float32 spacings at 1."""
    want = pitch.yin_curve_lags(signal32, hop, win, tau_max)
    ref_err = float(np.abs(yin_curve_f32(signal32, hop, win, tau_max).astype(np.float64) - want).max())
    return max(4.0 * ref_err, 16 * SPACING), ref_err


def f0_bar(curve, tau_min: int, rate):
    """Per frame: 4 x |float32 yin_select - float64 yin_select| + 4 float32 spacings of F0, on the given curve; with the float64
    evaluation (tau*, out)."""
    t64, o64 = pitch.yin_select(np.asarray(curve, np.float64), tau_min, THRESHOLD, rate, np.float64)
    t32, o32 = pitch.yin_select(curve, tau_min, THRESHOLD, rate, np.float32)
    spacing = np.spacing(np.maximum(o64[0], 1.0).astype(np.float32)).astype(np.float64)
    return 4.0 * np.abs(o32[0].astype(np.float64) - o64[0]) + 4.0 * spacing, t64, o64
