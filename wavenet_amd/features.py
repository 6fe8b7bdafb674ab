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


# ---- the same features on the device (libwavenet_logmel.so: wn_logmel) -------------------------------------------------------------
# Everything above is numpy and stays the definition; what follows computes it with one kernel launch per batch of clips and
# needs torch and the built library.  Supported there: an even win in [16, 4096], hop >= 1, n_mels in [1, 256], clips of more
# than win / 2 samples; `log_mel` keeps serving everything else.

LOGMEL_MAX_CLIPS = 64          # clips per launch (WN_LOGMEL_MAX_CLIPS)
LOGMEL_LDS_BYTES = 160 * 1024  # a workgroup holds the 31 hop + win samples of its 32 frames, and a 32 x 129 image of magnitudes


def dft_basis(win: int) -> np.ndarray:
    """(win, 2 * (win // 2 + 1)) float64: row n is  w[n] cos(2 pi n b / win), b = 0 .. win / 2,  then  -w[n] sin(2 pi n b / win),
    w the periodic Hann window -- ``frame @ basis`` is (Re, Im) of ``rfft(frame * w)``.  The angle is reduced as (n b) % win
    before it is scaled, so that large n b lose nothing."""
    n = np.arange(win, dtype=np.int64)[:, None]
    b = np.arange(win // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((n * b) % win).astype(np.float64) / win
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win, dtype=np.float64) / win)
    return np.concatenate([w[:, None] * np.cos(ang), -w[:, None] * np.sin(ang)], axis=1)


_TABLES = {}


def logmel_tables(rate, win: int, n_mels: int):
    """(basis, fbT) float32, cached per (rate, win, n_mels): :func:`dft_basis` and the transposed :func:`mel_filterbank`
    (one row per bin), each made in float64 and rounded once."""
    key = (float(rate), int(win), int(n_mels))
    if key not in _TABLES:
        _TABLES[key] = (np.ascontiguousarray(dft_basis(win).astype(np.float32)),
                        np.ascontiguousarray(mel_filterbank(rate, win, n_mels).T.astype(np.float32)))
    return _TABLES[key]


def mel_stream_frames(total_fed: int, hop: int, win: int, final: bool = False) -> int:
    """Columns a streaming analyser has emitted once ``total_fed`` samples have arrived.  Column k needs the samples up to
    k hop + win / 2 (column 0 reads that far when it reflects on the left; later columns are held to the same rule, one sample
    more than their window), so it is out as soon as total_fed > k hop + win / 2: a look-ahead of win / 2 samples.  ``final``
    (after ``flush``): every column of the signal, ``frame_count(total_fed, hop)``."""
    total_fed, hop, half = int(total_fed), int(hop), int(win) // 2
    if final:
        return frame_count(total_fed, hop)
    return 0 if total_fed <= half else (total_fed - half - 1) // hop + 1


def _check_logmel_shape(n_mels, hop, win) -> None:
    """What the device kernel takes, each refusal naming its value.  None: not known yet (a command line whose other values
    come from a checkpoint) -- what depends on it is not judged."""
    if win is not None and (win % 2 or win < 16 or win > 4096):
        raise ValueError("LogMel: win = %d; the device kernel takes an even win in 16 .. 4096 (features.log_mel serves the "
                         "rest)" % win)
    if hop is not None and hop < 1:
        raise ValueError("LogMel: hop = %d < 1" % hop)
    if n_mels is not None and (n_mels < 1 or n_mels > 256):
        raise ValueError("LogMel: n_mels = %d; the device kernel takes 1 .. 256 (features.log_mel serves the rest)" % n_mels)
    if hop is None or win is None:
        return
    seg = 31 * hop + win
    need = 4 * (seg + (seg // hop + 1 if hop % 2 == 0 else 0) + 32 * 129)
    if need > LOGMEL_LDS_BYTES:
        raise ValueError("LogMel: 32 frames at hop = %d, win = %d span %d samples, %d bytes of LDS; the limit is %d"
                         % (hop, win, seg, need, LOGMEL_LDS_BYTES))


class ClipAnalyser(object):
    """What the per-clip analysers share (``LogMel`` here, ``pitch.Pitch``): how a clip is taken in and which columns are asked
    for.  A subclass has ``hop`` and ``_launch(jobs, quantization_steps)`` -> one tensor per job, where a job is
    (samples, origin, first, count, left, right) and left / right say that this end of the buffer is the signal's.  Its name
    opens the messages."""

    def __init__(self, device):
        import torch
        self.device = torch.device(device)
        self._decode = {}
        self.launches = 0

    def _signal(self, x, quantization_steps):
        import torch
        name = type(self).__name__
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
        t = t.reshape(-1)
        if quantization_steps is None:
            if t.dtype != torch.float32:
                if not t.dtype.is_floating_point:
                    raise ValueError("%s: integer input (%s) is tokens and needs quantization_steps" % (name, t.dtype))
                t = t.to(torch.float32)
        else:
            if t.dtype.is_floating_point:
                raise ValueError("%s: quantization_steps = %d given with a %s signal; tokens are integers"
                                 % (name, quantization_steps, t.dtype))
            t = t.to(torch.int32)
        return t.to(self.device).contiguous()

    def _table(self, quantization_steps):
        import torch
        from . import data
        if quantization_steps is None:
            return None
        q = int(quantization_steps)
        if q not in self._decode:
            self._decode[q] = torch.as_tensor(data.mulaw_decode(np.arange(q), q).astype(np.float32)).to(self.device)
        return self._decode[q]

    def _check_length(self, n: int) -> None:
        """Refuse a clip of n samples that the analyser cannot take; any length by default."""

    def batch(self, clips, quantization_steps=None):
        """A list of clips of any lengths -> a list of (rows, ceil(N_i / hop)) tensors, at most 64 clips per launch."""
        xs = [self._signal(x, quantization_steps) for x in clips]
        for x in xs:
            self._check_length(x.numel())
        if not xs:
            return []
        return self._launch([(x, 0, 0, frame_count(x.numel(), self.hop), True, True) for x in xs], quantization_steps)

    def __call__(self, x, quantization_steps=None):
        return self.batch([x], quantization_steps)[0]

    def frames(self, x, first: int, count: int, quantization_steps=None):
        """Columns [first, first + count) of ``self(x)``."""
        x = self._signal(x, quantization_steps)
        self._check_length(x.numel())
        total = frame_count(x.numel(), self.hop)
        if first < 0 or count < 1 or first + count > total:
            raise ValueError("%s.frames: columns %d .. %d of a clip that has %d"
                             % (type(self).__name__, first, first + count - 1, total))
        return self._launch([(x, 0, first, count, True, True)], quantization_steps)[0]


class LogMel(ClipAnalyser):
    """``log_mel`` on the device: ``LogMel(rate)(x)`` -> (n_mels, ceil(N / hop)) float32 device tensor.

    ``x`` is a float32 signal, or int32 mu-law tokens together with ``quantization_steps`` (decoded inside the kernel with
    ``data.mulaw_decode``'s table); a numpy array or a tensor on any device is moved.  A column's bits depend on its own
    ``win`` samples only -- not on the call, the batch or the chunking that produced it, nor on tokens versus floats."""

    def __init__(self, rate, n_mels: int = 80, hop: int = 256, win: int = 1024, device=None):
        import torch
        n_mels, hop, win = int(n_mels), int(hop), int(win)
        _check_logmel_shape(n_mels, hop, win)
        self.rate, self.n_mels, self.hop, self.win = rate, n_mels, hop, win
        ClipAnalyser.__init__(self, "cuda" if device is None else device)
        basis, fbT = logmel_tables(rate, win, n_mels)
        self.basis = torch.as_tensor(basis).to(self.device)
        self.fbT = torch.as_tensor(fbT).to(self.device)

    def _check_length(self, n: int) -> None:
        if n <= self.win // 2:
            raise ValueError("LogMel: a clip of %d samples; the reflection at its ends needs more than win / 2 = %d"
                             % (n, self.win // 2))

    # -- the launch -----------------------------------------------------------------------------------------------------------
    def _launch(self, jobs, quantization_steps):
        """jobs: (samples, origin, first, count, reflect_left, reflect_right) -> one (n_mels, count) tensor each, in launches of
        at most LOGMEL_MAX_CLIPS clips."""
        import torch
        from . import _lib, _logmel
        table = self._table(quantization_steps)
        outs = [torch.empty((self.n_mels, int(j[3])), dtype=torch.float32, device=self.device) for j in jobs]
        with torch.cuda.device(self.device):
            for at in range(0, len(jobs), LOGMEL_MAX_CLIPS):
                part = jobs[at:at + LOGMEL_MAX_CLIPS]
                clips = (_logmel.WnLogmelClip * len(part))()
                for c, (x, origin, first, count, left, right) in enumerate(part):
                    clips[c].x, clips[c].n, clips[c].origin = x.data_ptr(), x.numel(), int(origin)
                    clips[c].out, clips[c].out_stride = outs[at + c].data_ptr(), int(count)
                    clips[c].first, clips[c].count = int(first), int(count)
                    clips[c].flags = (_logmel.WN_LOGMEL_REFLECT_LEFT if left else 0) | (_logmel.WN_LOGMEL_REFLECT_RIGHT if right else 0)
                _logmel.check(_logmel.lib().wn_logmel(clips, len(part), _lib.ptr(table), int(quantization_steps or 0),
                                                      _lib.ptr(self.basis), _lib.ptr(self.fbT), self.win, self.hop, self.n_mels,
                                                      _lib.stream_ptr()))
                self.launches += 1
        return outs

    def stream(self, quantization_steps=None):
        return MelStream(self, quantization_steps)


class MelStream(object):
    """``LogMel.stream()``: ``feed(samples)`` returns the (n_mels, k) columns whose windows the samples fed so far cover (k may be
    0), ``flush()`` the remaining ones, reflected at the signal's end.  Whatever the chunking, the columns concatenated are
    ``LogMel(...)(signal)`` bit for bit; ``mel_stream_frames`` says how many there are after each call.  Only the samples that a
    later column still reads are kept: from next_column * hop - win / 2 on."""

    def __init__(self, mel: LogMel, quantization_steps=None):
        self.mel, self.q = mel, quantization_steps
        self.total = 0           # samples fed
        self.emitted = 0         # columns returned
        self.start = 0           # signal index of tail[0]
        self.tail = None
        self.closed = False

    def _empty(self):
        import torch
        return torch.empty((self.mel.n_mels, 0), dtype=torch.float32, device=self.mel.device)

    def _emit(self, upto: int, final: bool):
        count = upto - self.emitted
        if count <= 0:
            return self._empty()
        m = self.mel
        if self.tail.numel() <= m.win // 2:      # only a signal shorter than the kernel accepts gets here
            raise ValueError("LogMel.stream: %d samples in all; the reflection needs more than win / 2 = %d"
                             % (self.total, m.win // 2))
        # frame 0 of the launch is column `emitted`; its centre sits at tail index emitted * hop - start
        out = m._launch([(self.tail, self.emitted * m.hop - self.start, 0, count, self.start == 0, final)], self.q)[0]
        self.emitted = upto
        keep_from = max(self.start, self.emitted * m.hop - m.win // 2)
        if keep_from > self.start:
            self.tail = self.tail[keep_from - self.start:].clone()
            self.start = keep_from
        return out

    def feed(self, samples):
        import torch
        if self.closed:
            raise ValueError("LogMel.stream: feed after flush")
        x = self.mel._signal(samples, self.q)
        self.tail = x if self.tail is None else torch.cat([self.tail, x])
        self.total += x.numel()
        return self._emit(mel_stream_frames(self.total, self.mel.hop, self.mel.win), False)

    def flush(self):
        if self.closed:
            raise ValueError("LogMel.stream: flush twice")
        self.closed = True
        if self.tail is None:
            return self._empty()
        return self._emit(mel_stream_frames(self.total, self.mel.hop, self.mel.win, True), True)
