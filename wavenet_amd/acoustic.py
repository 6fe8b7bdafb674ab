"""Log-mel and pitch on one column grid: the features of a network that is conditioned on both.

``mel_pitch(signal, rate)`` -> (n_mels + 3, ceil(N / hop)) is the definition (numpy): ``features.log_mel`` on top of
``pitch.pitch_channels(pitch.yin(...))``.  Column k of both is centred on sample k * hop: the mel window is the ``win`` samples
around it (reflected at the signal's ends), the pitch span the S = win + tau_max samples from k * hop - S // 2 on (zeros beyond
the ends).

``MelPitch`` holds a ``features.LogMel`` and a ``pitch.Pitch`` with those settings and is

    cat([LogMel(x), Pitch.channels(Pitch(x))])

bit for bit, in every form of the call: one clip, a batch, a column range, a stream, tokens or floats.  So every bit-level
contract of the two analysers carries over, and so do their refusals, under their own names.  No kernel is added: the two
launches are the analysers' own, and the map from a pitch column to its three channels is a few elementwise operations."""
from __future__ import annotations

import numpy as np

from . import features, pitch
from .features import mel_stream_frames
from .pitch import PITCH_CHANNELS, pitch_stream_frames


def mel_pitch(signal, rate, n_mels: int = 80, hop: int = 256, win: int = 1024, fmin: float = 60.0, fmax: float = 500.0,
              threshold: float = 0.15) -> np.ndarray:
    """(n_mels + 3, ceil(N / hop)) float64: the log-mel rows, then voiced, log-F0 and aperiodicity."""
    return np.vstack([features.log_mel(signal, rate, n_mels, hop, win),
                      pitch.pitch_channels(pitch.yin(signal, rate, hop, win, fmin, fmax, threshold), fmin, fmax)])


def mel_pitch_stream_frames(total_fed: int, hop: int, win: int, span: int, final: bool = False) -> int:
    """Columns a ``MelPitch`` stream has emitted once ``total_fed`` samples have arrived: those that both analysers have
    completed.  The pitch look-ahead, span - span // 2 samples, is the larger one (span = win + tau_max), so it decides."""
    return min(mel_stream_frames(total_fed, hop, win, final), pitch_stream_frames(total_fed, hop, span, final))


class MelPitch(object):
    """``mel_pitch`` on the device: ``MelPitch(rate)(x)`` -> (n_mels + 3, ceil(N / hop)) float32 device tensor.  ``x`` is a float32
    signal, or int32 mu-law tokens together with ``quantization_steps``, as for ``LogMel`` and ``Pitch`` (``.mel``, ``.pitch``)."""

    def __init__(self, rate, n_mels: int = 80, hop: int = 256, win: int = 1024, fmin: float = 60.0, fmax: float = 500.0,
                 threshold: float = 0.15, device=None):
        device = "cuda" if device is None else device
        self.mel = features.LogMel(rate, n_mels=n_mels, hop=hop, win=win, device=device)
        self.pitch = pitch.Pitch(rate, hop=hop, win=win, fmin=fmin, fmax=fmax, threshold=threshold, device=device)
        self.rate, self.hop, self.win, self.n_mels = rate, self.mel.hop, self.mel.win, self.mel.n_mels
        self.n_channels = self.n_mels + PITCH_CHANNELS
        self.device = self.mel.device

    def _join(self, mels, pits):
        """One (n_mels + 3, n_i) tensor per clip: the channel map runs once, over the columns of all clips."""
        import torch
        if not mels:
            return []
        chans = self.pitch.channels(pits[0] if len(pits) == 1 else torch.cat(pits, dim=1))
        out, at = [], 0
        for m, p in zip(mels, pits):
            n = int(p.shape[1])
            out.append(torch.cat([m, chans[:, at:at + n]], dim=0))
            at += n
        return out

    def batch(self, clips, quantization_steps=None):
        """A list of clips of any lengths -> a list of (n_mels + 3, ceil(N_i / hop)) tensors: one ``LogMel`` launch and one
        ``Pitch`` launch per 64 clips, the channel map once over all columns, and one ``cat`` per clip."""
        xs = [self.mel._signal(x, quantization_steps) for x in clips]
        for x in xs:
            self.mel._check_length(x.numel())
        return self._join(self.mel.batch(xs, quantization_steps), self.pitch.batch(xs, quantization_steps))

    def __call__(self, x, quantization_steps=None):
        return self.batch([x], quantization_steps)[0]

    def frames(self, x, first: int, count: int, quantization_steps=None):
        """Columns [first, first + count) of ``self(x)``."""
        x = self.mel._signal(x, quantization_steps)
        return self._join([self.mel.frames(x, first, count, quantization_steps)],
                          [self.pitch.frames(x, first, count, quantization_steps)])[0]

    def stream(self, quantization_steps=None):
        return MelPitchStream(self, quantization_steps)


class MelPitchStream(object):
    """``MelPitch.stream()``: ``feed(samples)`` returns the (n_mels + 3, k) columns that both analysers have completed (k may be
    0), ``flush()`` the remaining ones.  The mel stream is ahead of the pitch stream by (span - span // 2) - (win / 2 + 1)
    samples; its surplus columns wait here.  Whatever the chunking, the columns concatenated are ``MelPitch(...)(signal)`` bit
    for bit; ``mel_pitch_stream_frames`` says how many there are after each call."""

    def __init__(self, both: MelPitch, quantization_steps=None):
        self.both, self.q = both, quantization_steps
        self.mel, self.pitch = both.mel.stream(quantization_steps), both.pitch.stream(quantization_steps)
        self.emitted = 0
        self._mels, self._pits = [], []          # columns made and not handed out yet
        self.closed = False

    def _empty(self):
        import torch
        return torch.empty((self.both.n_channels, 0), dtype=torch.float32, device=self.both.device)

    def _emit(self, m, p):
        import torch
        if m.shape[1]:
            self._mels.append(m)
        if p.shape[1]:
            self._pits.append(p)
        have_m, have_p = sum(int(c.shape[1]) for c in self._mels), sum(int(c.shape[1]) for c in self._pits)
        k = min(have_m, have_p)
        if not k:
            return self._empty()
        mels = self._mels[0] if len(self._mels) == 1 else torch.cat(self._mels, dim=1)
        pits = self._pits[0] if len(self._pits) == 1 else torch.cat(self._pits, dim=1)
        self._mels = [mels[:, k:]] if have_m > k else []
        self._pits = [pits[:, k:]] if have_p > k else []
        self.emitted += k
        return torch.cat([mels[:, :k], self.both.pitch.channels(pits[:, :k])], dim=0)

    def feed(self, samples):
        if self.closed:
            raise ValueError("MelPitch.stream: feed after flush")
        x = self.both.mel._signal(samples, self.q)
        return self._emit(self.mel.feed(x), self.pitch.feed(x))

    def flush(self):
        if self.closed:
            raise ValueError("MelPitch.stream: flush twice")
        self.closed = True
        return self._emit(self.mel.flush(), self.pitch.flush())
