"""A float32 numpy restatement of the device rate converter (wavenet_amd/csrc/front/resample.hip): the same float32-rounded tap
table, a multiply and an add per tap in t order -- what float32 arithmetic costs against ``resample.resample`` (float64), which
is how the GPU tests size their bar -- and the test signals those tests share.  Absolute indices are Python ints."""
import numpy as np

from wavenet_amd import resample

# the five ratios of the tests, and the lengths of the CPU comparisons against the direct double sum
RATIOS = [(48000, 16000), (44100, 16000), (8000, 16000), (22050, 16000), (16000, 44100)]
LENGTHS = [700, 1500, 300, 900, 400]


def chirp_noise(n: int, rate: float = 48000.0, amplitude: float = 0.5, seed: int = 0) -> np.ndarray:
    """A chirp from 100 Hz up to 0.45 x rate plus noise, peak below 0.75 (float64; the tests round it once)."""
    t = np.arange(n) / float(rate)
    dur = max(n, 1) / float(rate)
    x = amplitude * np.sin(2 * np.pi * (100.0 + 0.5 * (0.45 * rate - 100.0) * t / dur) * t)
    return x + 0.05 * np.clip(np.random.RandomState(seed).randn(n), -4, 4)


def pcm16(n: int, rate: float = 48000.0, seed: int = 0) -> np.ndarray:
    return resample.to_pcm16(chirp_noise(n, rate, seed=seed))


def square(n: int, period: int = 40) -> np.ndarray:
    """A full-scale square wave as int16 PCM: the band-limited copy overshoots +-1 at every edge."""
    return np.where((np.arange(n) // (period // 2)) % 2 == 0, 32767, -32768).astype(np.int16)


def block_f32(x, origin: int, first: int, count: int, rate_in, rate_out, start=True, end=True) -> np.ndarray:
    """Outputs first .. first + count - 1 in float32: acc = acc + taps[phi, t] * x[q + Kt - t], t = 0 .. T - 1, every product and
    every sum rounded to float32; samples outside the buffer are zero (``start`` / ``end`` must then say that the signal
    ends there)."""
    L, M, P, T, taps = resample.resample_tables(rate_in, rate_out)
    x = np.asarray(x).reshape(-1)
    x = (x.astype(np.float32) / np.float32(32768.0)) if x.dtype == np.int16 else x.astype(np.float32)
    Kt = (T - 1) // 2
    origin, first, count = int(origin), int(first), int(count)
    q0, r0 = divmod(first * M, L)                                   # Python ints
    v = r0 + np.arange(count, dtype=np.int64) * M
    dq, phi = v // L, v % L
    lo = q0 - Kt - origin
    hi = lo + int(dq[-1]) + T - 1 if count else lo
    assert (lo >= 0 or start) and (hi < x.size or end), "the taps reach past an end that is not the signal's"
    seg = np.zeros((int(dq[-1]) + T if count else 0,), dtype=np.float32)
    a, b = max(lo, 0), min(lo + seg.size, x.size)
    if b > a:
        seg[a - lo:b - lo] = x[a:b]
    acc = np.zeros((count,), dtype=np.float32)
    for t in range(T):
        acc = (acc + (taps[phi, t] * seg[dq + (T - 1 - t)]).astype(np.float32)).astype(np.float32)
    return acc


def resample_f32(x, rate_in, rate_out) -> np.ndarray:
    L, M = resample.ratio(rate_in, rate_out)
    return block_f32(x, 0, 0, resample.output_count(np.asarray(x).size, L, M), rate_in, rate_out)


def bar(x, rate_in, rate_out):
    """(bar, error of the float32 restatement): 4 x that error against the float64 definition on the same input."""
    want = resample.resample(x, rate_in, rate_out)
    ref_err = float(np.abs(resample_f32(x, rate_in, rate_out).astype(np.float64) - want).max())
    return 4.0 * ref_err, ref_err


def response_db(h, L, freqs):
    """Gain in dB of the prototype h (float64, 2 P + 1 taps, at the rate L * rate_in) at ``freqs``, given as fractions of THAT
    rate's sampling frequency; the gain of the converter is |H| / L."""
    P = (h.size - 1) // 2
    i = np.arange(-P, P + 1, dtype=np.float64)
    H = np.array([np.sum(h * np.cos(2 * np.pi * f * i)) for f in freqs]) / L        # h is even: the response is real
    return 20 * np.log10(np.maximum(np.abs(H), 1e-300))
