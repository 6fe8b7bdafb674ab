"""Acoustic features for local conditioning (numpy only): a log-mel spectrogram with one column per ``hop`` samples.

``log_mel(signal, rate)`` -> (n_mels, ceil(N / hop)) float32.  Column k describes the ``win`` samples centred on sample
k * hop, so it is the column that ``local_alignment`` hands to samples k * hop .. (k + 1) * hop - 1:

    frames    the signal reflect-padded by win // 2 on both sides, frame k = padded[k hop : k hop + win]
    spectrum  |rfft(frame * w)|, w the periodic Hann window  0.5 - 0.5 cos(2 pi n / win)
    mel       a triangular filterbank of n_mels filters whose corners are equally spaced on the mel scale
              m = 2595 log10(1 + f / 700) between 0 Hz and rate / 2, evaluated at the rfft bin frequencies
    value     log(max(mel, 1e-5))

Users may bring any other (F, frames) ``.npy`` features instead; nothing here is special to the network."""
from __future__ import annotations

import numpy as np


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_filterbank(rate: float, win: int, n_mels: int) -> np.ndarray:
    """(n_mels, win // 2 + 1) float64: filter i rises from corner i to corner i + 1 and falls to corner i + 2."""
    corners = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(rate / 2.0), n_mels + 2))
    freqs = np.arange(win // 2 + 1, dtype=np.float64) * (float(rate) / win)
    fb = np.zeros((n_mels, freqs.size), dtype=np.float64)
    for i in range(n_mels):
        lo, mid, hi = corners[i], corners[i + 1], corners[i + 2]
        up = (freqs - lo) / (mid - lo)
        down = (hi - freqs) / (hi - mid)
        fb[i] = np.maximum(0.0, np.minimum(up, down))
    return fb


def frame_count(n_samples: int, hop: int) -> int:
    return (int(n_samples) + int(hop) - 1) // int(hop)


def log_mel(signal, rate, n_mels: int = 80, hop: int = 256, win: int = 1024) -> np.ndarray:
    x = np.asarray(signal, dtype=np.float64).reshape(-1)
    if x.size < 2:
        raise ValueError("log_mel: the signal needs at least 2 samples, got %d" % x.size)
    if n_mels < 1 or hop < 1 or win < 2 or win % 2:
        raise ValueError("log_mel: n_mels >= 1, hop >= 1 and an even win >= 2 (got %d, %d, %d)" % (n_mels, hop, win))
    n = frame_count(x.size, hop)
    padded = np.pad(x, win // 2, mode="reflect")
    idx = np.arange(n)[:, None] * hop + np.arange(win)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    spec = np.abs(np.fft.rfft(padded[idx] * w[None, :], axis=1))             # (n, win // 2 + 1)
    mel = mel_filterbank(rate, win, n_mels) @ spec.T                          # (n_mels, n)
    return np.log(np.maximum(mel, 1e-5)).astype(np.float32)
