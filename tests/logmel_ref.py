"""A float32 numpy restatement of the device log-mel (wavenet_amd/csrc/logmel.hip): the same float32 basis and filterbank
arrays, plain ``@`` -- what float32 arithmetic costs against ``features.log_mel`` (float64 inside), which is how the GPU
tests size their bar -- and the test signal those tests share."""
import numpy as np

from wavenet_amd import data, features

# (win, hop, n_mels, N): the three measured shapes; hop does not divide win, 49 bins, a ragged tile of 26 frames; the smallest
# shape (40 frames: two tiles, maximal overlap); the shortest accepted clip, N = win / 2 + 1
SHAPES = [(64, 16, 8, 700), (256, 64, 20, 3000), (1024, 256, 80, 16000), (96, 40, 13, 1001), (16, 1, 1, 40), (64, 16, 8, 33)]
RATE = 16000
FLOOR_SPACING = 2.0 ** -20             # the float32 spacing at |log 1e-5| = 11.5


def chirp_signal(n: int) -> np.ndarray:
    """Loud, noisy and silent columns: a chirp over the first 60 %, noise from 30 % on, the last fifth zero, through mu-law
    at Q = 256 and back (float64; the tests round it to float32 once)."""
    t = np.arange(n) / 16000.0
    x = np.where(t < 0.6 * n / 16000.0, 0.5 * np.sin(2 * np.pi * (200 + 3000 * t) * t), 0.0)
    x = x + np.where(t > 0.3 * n / 16000.0, 0.05 * np.random.RandomState(0).randn(n), 0.0)
    x[n - n // 5:] = 0.0
    return data.mulaw_decode(data.mulaw_encode(x, 256), 256)


def log_mel_f32(signal, rate, n_mels: int, hop: int, win: int) -> np.ndarray:
    """(n_mels, frames) float32, every sum in float32."""
    x = np.asarray(signal, dtype=np.float32).reshape(-1)
    basis, fbT = features.logmel_tables(rate, win, n_mels)
    n = features.frame_count(x.size, hop)
    padded = np.pad(x, win // 2, mode="reflect")
    frames = padded[np.arange(n)[:, None] * hop + np.arange(win)[None, :]]          # (n, win) float32
    ri = frames @ basis                                                             # (n, 2 nb) float32
    nb = win // 2 + 1
    mag = np.sqrt(ri[:, :nb] * ri[:, :nb] + ri[:, nb:] * ri[:, nb:])
    mel = (mag @ fbT).T
    return np.log(np.maximum(mel, np.float32(1e-5))).astype(np.float32)


def bar(signal32, win, hop, n_mels):
    """(bar, error of the float32 restatement): 4 x that error against ``log_mel``, never below 16 float32 spacings at the
    floor."""
    want = features.log_mel(signal32, RATE, n_mels, hop, win)
    ref_err = float(np.abs(log_mel_f32(signal32, RATE, n_mels, hop, win).astype(np.float64) - want).max())
    return max(4.0 * ref_err, 16 * FLOOR_SPACING), ref_err
