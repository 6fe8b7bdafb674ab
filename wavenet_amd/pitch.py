"""Pitch tracking (numpy, float64): YIN (de Cheveigne & Kawahara 2002), stated so that every output depends on its own samples.

``yin(signal, rate)`` -> (2, ceil(N / hop)) float64: row 0 is F0 in Hz (0: unvoiced), row 1 the aperiodicity c[tau*]; row 0 > 0
exactly when row 1 < threshold.  Column k sits on ``features.log_mel``'s column k:

    lags      tau_min = floor(rate / fmax) .. tau_max = ceil(rate / fmin)  (``pitch_lags``; tau_min >= 2, tau_max >= tau_min + 2)
    frames    with S = win + tau_max, frame k is the S samples from k * hop - S // 2 on; outside the signal they are ZERO (a
              reflection would fake periodicity)
    d[tau]    sum_{j = 0}^{win - 1} (s[j] - s[j + tau])^2,  tau = 0 .. tau_max, j ascending
    c[tau]    c[0] = 1; with r_tau = d[1] + ... + d[tau] in index order, d[tau] * tau / r_tau -- 1 where r_tau is not > 0, so a
              silent or constant frame has c = 1 everywhere and is unvoiced
    tau*      over tau_min .. tau_max - 1: the first tau with c[tau] < threshold, walked on while c[tau + 1] < c[tau] (voiced);
              if there is none, the first argmin (unvoiced)
    f0        a, b, g = c[tau* - 1], c[tau*], c[tau* + 1]; den = a - 2 b + g; shift = 0.5 (a - g) / den if den > 0 else 0, clamped
              to [-1, 1]; f0 = rate / (tau* + shift)

``Pitch`` computes the same on the device (libwavenet_pitch.so: wn_pitch), one launch per batch of clips.

``pitch_channels(rows, fmin, fmax)`` -> (3, n): what a network is conditioned on -- voiced (1 / 0), log-F0 on a scale where fmin is 0
and fmax is 1 (0 where unvoiced; never clamped: the refinement may leave [fmin, fmax] by a fraction of a lag, and the value follows
it) and the aperiodicity min(c[tau*], 1).  ``Pitch.channels`` is the same map in float32 on the device, ``scale_f0`` moves the
pitch of such channels, ``Pitch.stream`` makes the rows as the audio arrives (``pitch_stream_frames`` says how many)."""
from __future__ import annotations

import math

import numpy as np

from .features import ClipAnalyser, frame_count


def pitch_lags(rate, fmin: float = 60.0, fmax: float = 500.0):
    """(tau_min, tau_max) = (floor(rate / fmax), ceil(rate / fmin))."""
    if not (rate > 0 and fmin > 0 and fmax > fmin):
        raise ValueError("pitch_lags: rate = %r, fmin = %r, fmax = %r; it takes rate > 0 and 0 < fmin < fmax" % (rate, fmin, fmax))
    tau_min, tau_max = int(math.floor(rate / fmax)), int(math.ceil(rate / fmin))
    if tau_min < 2:
        raise ValueError("pitch_lags: tau_min = floor(%r / %r) = %d < 2" % (rate, fmax, tau_min))
    if tau_max < tau_min + 2:
        raise ValueError("pitch_lags: tau_max = ceil(%r / %r) = %d below tau_min + 2 = %d" % (rate, fmin, tau_max, tau_min + 2))
    return tau_min, tau_max


def yin_frames(x: np.ndarray, hop: int, win: int, tau_max: int) -> np.ndarray:
    """(frames, win + tau_max): frame k is x[k hop - S // 2 : + S], zero outside the signal."""
    S = win + tau_max
    n = frame_count(x.size, hop)
    padded = np.concatenate([np.zeros(S // 2, x.dtype), x, np.zeros(S + hop, x.dtype)])
    return padded[np.arange(n)[:, None] * hop + np.arange(S)[None, :]]


def yin_curve_lags(signal, hop: int, win: int, tau_max: int) -> np.ndarray:
    """(frames, tau_max + 1) float64: the normalised difference c of every frame."""
    x = np.asarray(signal, dtype=np.float64).reshape(-1)
    if hop < 1 or win < 1 or tau_max < 1:
        raise ValueError("yin: hop >= 1, win >= 1 and tau_max >= 1 (got %d, %d, %d)" % (hop, win, tau_max))
    fr = yin_frames(x, hop, win, tau_max)
    d = np.zeros((fr.shape[0], tau_max + 1), dtype=np.float64)
    head = fr[:, :win]
    for tau in range(1, tau_max + 1):
        diff = head - fr[:, tau:tau + win]
        d[:, tau] = np.einsum("fj,fj->f", diff, diff)
    r = np.cumsum(d, axis=1)                                         # d[0] = 0: r_tau = d[1] + ... + d[tau]
    c = np.ones_like(d)
    ok = r > 0
    ok[:, 0] = False
    tau = np.arange(tau_max + 1, dtype=np.float64)[None, :]
    c[ok] = (d * tau)[ok] / r[ok]
    return c


def yin_curve(signal, rate, hop: int = 256, win: int = 1024, fmin: float = 60.0, fmax: float = 500.0) -> np.ndarray:
    return yin_curve_lags(signal, hop, win, pitch_lags(rate, fmin, fmax)[1])


def yin_select(curve, tau_min: int, threshold: float, rate, dtype=np.float64):
    """Selection and refinement on a (frames, tau_max + 1) curve, every comparison and operation in ``dtype``.
    Returns (tau*, out): (frames,) int64 and (2, frames) ``dtype`` -- F0 (0: unvoiced) and c[tau*]."""
    dt = np.dtype(dtype).type
    c = np.asarray(curve).astype(dt)
    n, tau_max = c.shape[0], c.shape[1] - 1
    if tau_min < 1 or tau_max < tau_min + 2:
        raise ValueError("yin_select: lags %d .. %d" % (tau_min, tau_max))
    thr, rate = dt(threshold), dt(rate)
    taus = np.zeros(n, dtype=np.int64)
    out = np.zeros((2, n), dtype=dt)
    half, one, two = dt(0.5), dt(1.0), dt(2.0)
    for k in range(n):
        row = c[k]
        cand = row[tau_min:tau_max]                                 # tau_min .. tau_max - 1
        below = np.flatnonzero(cand < thr)
        if below.size:
            t = tau_min + int(below[0])
            while t + 1 <= tau_max - 1 and row[t + 1] < row[t]:
                t += 1
        else:
            t = tau_min + int(np.argmin(cand))
        a, b, g = row[t - 1], row[t], row[t + 1]
        den = (a - two * b) + g
        shift = (half * (a - g)) / den if den > 0 else dt(0.0)
        shift = min(max(shift, -one), one)
        taus[k] = t
        out[1, k] = b
        out[0, k] = rate / (dt(t) + shift) if b < thr else dt(0.0)
    return taus, out


def yin(signal, rate, hop: int = 256, win: int = 1024, fmin: float = 60.0, fmax: float = 500.0, threshold: float = 0.15):
    tau_min, tau_max = pitch_lags(rate, fmin, fmax)
    return yin_select(yin_curve_lags(signal, hop, win, tau_max), tau_min, threshold, rate, np.float64)[1]


# ---- pitch as conditioning channels -------------------------------------------------------------------------------------------------
PITCH_CHANNELS = 3             # voiced, log-F0, aperiodicity


def _check_band(who, fmin, fmax):
    if not fmin > 0:
        raise ValueError("%s: fmin = %r; it takes fmin > 0" % (who, fmin))
    if not fmax > fmin:
        raise ValueError("%s: fmax = %r; it takes fmax > fmin = %r" % (who, fmax, fmin))


def pitch_channels(rows, fmin: float = 60.0, fmax: float = 500.0) -> np.ndarray:
    """(2, n) pitch rows (F0 with 0 for unvoiced; c[tau*]) -> (3, n) float64 conditioning channels:

        row 0   1 where f0 > 0, else 0
        row 1   (log2(f0) - log2(fmin)) / log2(fmax / fmin) where voiced, else 0 -- fmin is 0, fmax is 1, nothing is clamped
        row 2   min(c[tau*], 1)"""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] != 2:
        raise ValueError("pitch_channels: rows of shape %s; it takes (2, n)" % (rows.shape,))
    _check_band("pitch_channels", fmin, fmax)
    voiced = rows[0] > 0
    out = np.zeros((PITCH_CHANNELS, rows.shape[1]), dtype=np.float64)
    out[0, voiced] = 1.0
    out[1, voiced] = (np.log2(rows[0, voiced]) - math.log2(fmin)) / math.log2(fmax / fmin)
    out[2] = np.minimum(rows[1], 1.0)
    return out


def channel_constants(fmin, fmax):
    """(lo, k) of the float32 map: lo = float32(log2(fmin)), k = float32(1 / log2(fmax / fmin)); lf = (log2(f0) - lo) * k."""
    _check_band("pitch_channels", fmin, fmax)
    return np.float32(math.log2(fmin)), np.float32(1.0 / math.log2(fmax / fmin))


def scale_f0(channels, scale, fmin: float = 60.0, fmax: float = 500.0):
    """Pitch channels (3, n) -- a numpy array or a tensor -- with the pitch of the voiced columns multiplied by ``scale``:
    log2(scale) / log2(fmax / fmin), rounded to the array's type, is added to row 1 where row 0 is 1.  Everything else keeps its
    bits, and ``scale`` = 1 hands the input back."""
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("scale_f0: scale = %r; it takes a finite scale > 0" % (scale,))
    _check_band("scale_f0", fmin, fmax)
    if len(channels.shape) != 2 or channels.shape[0] != PITCH_CHANNELS:
        raise ValueError("scale_f0: channels of shape %s; it takes (3, n)" % (tuple(channels.shape),))
    if scale == 1.0:
        return channels
    delta = math.log2(scale) / math.log2(fmax / fmin)
    if isinstance(channels, np.ndarray):
        out = channels.copy()
        out[1] = np.where(channels[0] == 1, channels[1] + channels.dtype.type(delta), channels[1])
        return out
    import torch
    out = channels.clone()
    out[1] = torch.where(channels[0] == 1, channels[1] + delta, channels[1])
    return out


def pitch_stream_frames(total_fed: int, hop: int, span: int, final: bool = False) -> int:
    """Columns a streaming pitch analyser has emitted once ``total_fed`` samples have arrived.  Column k reads the ``span``
    samples from k hop - span // 2 on, the last of them sample k hop - span // 2 + span - 1, so it is out as soon as
    total_fed >= k hop + span - span // 2: a look-ahead of span - span // 2 samples.  ``final`` (after ``flush``): every column of
    the signal, ``frame_count(total_fed, hop)``."""
    total_fed, hop, ahead = int(total_fed), int(hop), int(span) - int(span) // 2
    if final:
        return frame_count(total_fed, hop)
    return 0 if total_fed < ahead else (total_fed - ahead) // hop + 1


# ---- the same on the device (libwavenet_pitch.so: wn_pitch) -----------------------------------------------------------------------
# Everything above is numpy and stays the definition; what follows computes it with one kernel launch per batch of clips and
# needs torch and the built library.  Supported there: win in [16, 4096], hop >= 1, tau_min >= 2, tau_max in
# [tau_min + 2, 2047] and a workgroup's frames within the LDS; `yin` keeps serving everything else.

PITCH_MAX_CLIPS = 64           # clips per launch (WN_PITCH_MAX_CLIPS)
PITCH_LDS_BYTES = 160 * 1024
PITCH_LAGS_PER_LANE = 7        # pitch.hip: kLags
PITCH_MAX_TILE = 8             # pitch.hip: kMaxTile


def pitch_tile_frames(tau_max: int) -> int:
    """Frames a workgroup takes: as many as fill its 256 lanes with groups of 7 lags, 1 .. 8 (pitch.hip: tile_frames)."""
    groups = (tau_max + PITCH_LAGS_PER_LANE) // PITCH_LAGS_PER_LANE
    return max(1, min(PITCH_MAX_TILE, 256 // groups))


def pitch_lds_bytes(win: int, hop: int, tau_max: int) -> int:
    """The tile's samples (and 8 zeros behind them), then d and the running sums of its frames."""
    ft = pitch_tile_frames(tau_max)
    return 4 * ((ft - 1) * hop + win + tau_max + 8 + 2 * ft * (tau_max + 1))


def _device_refusal(win, hop, tau_min, tau_max):
    """What wn_pitch refuses, naming the value; None when it takes the shape."""
    if win < 16 or win > 4096:
        return "Pitch: win = %d; the device kernel takes 16 .. 4096 (pitch.yin serves the rest)" % win
    if hop < 1:
        return "Pitch: hop = %d < 1" % hop
    if tau_min < 2:
        return "Pitch: tau_min = %d < 2" % tau_min
    if tau_max < tau_min + 2 or tau_max > 2047:
        return "Pitch: tau_max = %d; the device kernel takes tau_min + 2 = %d .. 2047 (pitch.yin serves the rest)" % (tau_max, tau_min + 2)
    need = pitch_lds_bytes(win, hop, tau_max)
    if need > PITCH_LDS_BYTES:
        return ("Pitch: %d frames at hop = %d, win = %d, tau_max = %d need %d bytes of LDS; the limit is %d"
                % (pitch_tile_frames(tau_max), hop, win, tau_max, need, PITCH_LDS_BYTES))
    return None


class Pitch(ClipAnalyser):
    """``yin`` on the device: ``Pitch(rate)(x)`` -> (2, ceil(N / hop)) float32 device tensor (F0 with 0 for unvoiced;
    aperiodicity).

    ``x`` is a float32 signal, or int32 mu-law tokens together with ``quantization_steps`` (decoded inside the kernel with
    ``data.mulaw_decode``'s table).  A column's bits depend on its own win + tau_max samples and the parameters only -- not on
    the call, the batch, the column range asked for, nor on tokens versus floats."""

    def __init__(self, rate, hop: int = 256, win: int = 1024, fmin: float = 60.0, fmax: float = 500.0, threshold: float = 0.15,
                 device="cuda"):
        hop, win = int(hop), int(win)
        self.tau_min, self.tau_max = pitch_lags(rate, fmin, fmax)
        why = _device_refusal(win, hop, self.tau_min, self.tau_max)
        if why:
            raise ValueError(why)
        self.rate, self.hop, self.win, self.fmin, self.fmax, self.threshold = rate, hop, win, fmin, fmax, float(threshold)
        self.span = win + self.tau_max                                # S: the samples a column reads
        ClipAnalyser.__init__(self, device)

    def reach(self, origin: int, first: int, count: int):
        """Buffer indices (lo, hi) of the first and last sample that columns first .. first + count - 1 read."""
        lo = origin + first * self.hop - self.span // 2
        return lo, lo + (count - 1) * self.hop + self.span - 1

    # -- the launch -----------------------------------------------------------------------------------------------------------
    def _launch(self, jobs, quantization_steps, curve: bool = False):
        """jobs: (samples, origin, first, count, start, end) -> one (2, count) tensor each (and, with ``curve``, one
        (count, tau_max + 1) tensor each), in launches of at most PITCH_MAX_CLIPS clips.  Everything is checked before the first
        launch."""
        import torch
        from . import _lib, _pitch
        for x, origin, first, count, start, end in jobs:
            if first < 0 or count < 0:
                raise ValueError("Pitch: first = %d or count = %d is negative" % (first, count))
            if count:
                lo, hi = self.reach(origin, first, count)
                if (lo < 0 and not start) or (hi >= x.numel() and not end):
                    raise ValueError("Pitch: columns %d .. %d read samples %d .. %d, the buffer holds 0 .. %d and that edge is not "
                                     "the signal's" % (first, first + count - 1, lo, hi, x.numel() - 1))
        table = self._table(quantization_steps)
        outs = [torch.empty((2, int(j[3])), dtype=torch.float32, device=self.device) for j in jobs]
        curves = [torch.empty((int(j[3]), self.tau_max + 1), dtype=torch.float32, device=self.device) for j in jobs] if curve else None
        with torch.cuda.device(self.device):
            for at in range(0, len(jobs), PITCH_MAX_CLIPS):
                part = jobs[at:at + PITCH_MAX_CLIPS]
                clips = (_pitch.WnPitchClip * len(part))()
                for c, (x, origin, first, count, start, end) in enumerate(part):
                    clips[c].x, clips[c].n, clips[c].origin = x.data_ptr(), x.numel(), int(origin)
                    clips[c].out, clips[c].out_stride = outs[at + c].data_ptr(), int(count)
                    clips[c].curve = curves[at + c].data_ptr() if curve else None
                    clips[c].first, clips[c].count = int(first), int(count)
                    clips[c].flags = (_pitch.WN_PITCH_START if start else 0) | (_pitch.WN_PITCH_END if end else 0)
                _pitch.check(_pitch.lib().wn_pitch(clips, len(part), _lib.ptr(table), int(quantization_steps or 0), self.win, self.hop,
                                                   self.tau_min, self.tau_max, self.threshold, float(self.rate), _lib.stream_ptr()))
                self.launches += 1
        return (outs, curves) if curve else outs

    def block(self, x, origin: int, first: int, count: int, start: bool = False, end: bool = False, quantization_steps=None):
        """``count`` columns from a buffer that is part of a longer signal: column ``first + j`` is centred on buffer sample
        origin + (first + j) * hop.  ``start`` / ``end``: that edge of the buffer is the signal's (zeros beyond it); a column that
        reaches past another edge is refused."""
        return self._launch([(self._signal(x, quantization_steps), origin, first, count, start, end)], quantization_steps)[0]

    def curve(self, x, quantization_steps=None):
        """(frames, tau_max + 1): the normalised difference of every column (for tests and plots)."""
        x = self._signal(x, quantization_steps)
        return self._launch([(x, 0, 0, frame_count(x.numel(), self.hop), True, True)], quantization_steps, curve=True)[1][0]

    def analyse(self, x, quantization_steps=None):
        """(pitch (2, frames), curve (frames, tau_max + 1)) of one launch."""
        x = self._signal(x, quantization_steps)
        outs, curves = self._launch([(x, 0, 0, frame_count(x.numel(), self.hop), True, True)], quantization_steps, curve=True)
        return outs[0], curves[0]

    def channels(self, rows):
        """``pitch_channels`` of (2, n) device rows, in float32 with elementwise torch operations: lo = float32(log2(fmin)),
        k = float32(1 / log2(fmax / fmin)), lf = (log2(f0) - lo) * k.  A column's bits depend on its own column of ``rows``."""
        import torch
        if rows.dim() != 2 or rows.shape[0] != 2:
            raise ValueError("Pitch.channels: rows of shape %s; it takes (2, n)" % (tuple(rows.shape),))
        lo, k = (float(v) for v in channel_constants(self.fmin, self.fmax))
        rows = rows.to(torch.float32)
        f0, voiced = rows[0], rows[0] > 0
        lf = (torch.log2(torch.where(voiced, f0, torch.ones_like(f0))) - lo) * k
        return torch.stack([voiced.to(torch.float32), torch.where(voiced, lf, torch.zeros_like(lf)), torch.clamp(rows[1], max=1.0)])

    def stream(self, quantization_steps=None):
        return PitchStream(self, quantization_steps)


class PitchStream(object):
    """``Pitch.stream()``: ``feed(samples)`` returns the (2, k) columns whose spans the samples fed so far cover (k may be 0),
    ``flush()`` the remaining ones, with zeros beyond the signal's end.  Whatever the chunking, the columns concatenated are
    ``Pitch(...)(signal)`` bit for bit; ``pitch_stream_frames`` says how many there are after each call.  Only the samples that a
    later column still reads are kept: from next_column * hop - span // 2 on."""

    def __init__(self, pitch: Pitch, quantization_steps=None):
        self.pitch, self.q = pitch, quantization_steps
        self.total = 0           # samples fed
        self.emitted = 0         # columns returned
        self.start = 0           # signal index of tail[0]
        self.tail = None
        self.closed = False

    def _empty(self):
        import torch
        return torch.empty((2, 0), dtype=torch.float32, device=self.pitch.device)

    def _emit(self, upto: int, final: bool):
        count = upto - self.emitted
        if count <= 0:
            return self._empty()
        p = self.pitch
        # frame 0 of the launch is column `emitted`; its centre sits at tail index emitted * hop - start
        out = p._launch([(self.tail, self.emitted * p.hop - self.start, 0, count, self.start == 0, final)], self.q)[0]
        self.emitted = upto
        keep_from = min(max(self.start, self.emitted * p.hop - p.span // 2), self.total)
        if keep_from > self.start:
            self.tail = self.tail[keep_from - self.start:].clone()
            self.start = keep_from
        return out

    def feed(self, samples):
        import torch
        if self.closed:
            raise ValueError("Pitch.stream: feed after flush")
        x = self.pitch._signal(samples, self.q)
        self.tail = x if self.tail is None else torch.cat([self.tail, x])
        self.total += x.numel()
        return self._emit(pitch_stream_frames(self.total, self.pitch.hop, self.pitch.span), False)

    def flush(self):
        if self.closed:
            raise ValueError("Pitch.stream: flush twice")
        self.closed = True
        if self.tail is None:
            return self._empty()
        return self._emit(pitch_stream_frames(self.total, self.pitch.hop, self.pitch.span, True), True)
