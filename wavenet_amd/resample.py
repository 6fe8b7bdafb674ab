"""Sample-rate conversion: a windowed-sinc polyphase converter for a rational ratio.  The numpy part (float64) is the
definition and the host fallback; ``Resampler`` runs the same sum on the device (libwavenet_resample.so: wn_resample).

    g = gcd(rate_in, rate_out), L = rate_out // g, M = rate_in // g, K = max(L, M), P = zeros * K
    h[i] = L c sinc(c i) kaiser(2 P + 1, beta)[i + P],  c = rolloff / K,  i = -P .. P      the low-pass at the rate L * rate_in
    y[n] = sum over m with |n M - m L| <= P of  h[n M - m L] x[m],  n = 0 .. ceil(N L / M) - 1,  x zero outside the signal

In polyphase form, with q, phi = divmod(n M, L), Kt = ceil(P / L) and T = 2 Kt + 1:

    taps[phi, t] = h[phi + (t - Kt) L]   (0 where the index leaves [-P, P]),     y[n] = sum_{t = 0}^{T - 1} taps[phi, t] x[q + Kt - t]

Equal rates are the identity: no filter, the input's bits.  A stream (``resample_stream_counts``): output n is complete once input
sample floor((n M + P) / L) has been fed, a look-ahead of P / L input samples; only the inputs from ceil((next_n M - P) / L) on are
kept."""
from __future__ import annotations

from math import gcd

import numpy as np

ZEROS, ROLLOFF, BETA = 32, 0.9, 8.6
RESAMPLE_MAX_CLIPS = 64            # clips per launch (WN_RESAMPLE_MAX_CLIPS)
RESAMPLE_TILE = 256                # outputs per workgroup (WN_RESAMPLE_TILE)
RESAMPLE_LDS_BYTES = 160 * 1024    # a workgroup holds the input span of its tile
OUT_KINDS = ("float", "pcm16", "tokens")


def ratio(rate_in, rate_out):
    """(L, M) of a conversion: rate_out / rate_in in lowest terms."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in < 1 or rate_out < 1:
        raise ValueError("resample: rates must be positive integers, got %r -> %r" % (rate_in, rate_out))
    g = gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def prototype(L: int, M: int, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA) -> np.ndarray:
    """h[-P .. P] as a float64 array of 2 P + 1 entries (entry i + P is h[i])."""
    K = max(int(L), int(M))
    P = int(zeros) * K
    c = float(rolloff) / K
    i = np.arange(-P, P + 1, dtype=np.float64)
    return L * c * np.sinc(c * i) * np.kaiser(2 * P + 1, beta)


def polyphase(L: int, M: int, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA):
    """(P, T, taps) with taps the (L, T) float64 rows of the polyphase form."""
    L, M = int(L), int(M)
    h = prototype(L, M, zeros, rolloff, beta)
    P = (h.size - 1) // 2
    Kt = -(-P // L)
    T = 2 * Kt + 1
    idx = np.arange(L)[:, None] + (np.arange(T)[None, :] - Kt) * L
    taps = np.where(np.abs(idx) <= P, h[np.clip(idx + P, 0, 2 * P)], 0.0)
    return P, T, np.ascontiguousarray(taps)


def resample_tables(rate_in, rate_out, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA):
    """(L, M, P, T, taps): ``taps`` (L, T) float32, made in float64 and rounded once -- what the device kernel is handed."""
    L, M = ratio(rate_in, rate_out)
    P, T, taps = polyphase(L, M, zeros, rolloff, beta)
    return L, M, P, T, np.ascontiguousarray(taps.astype(np.float32))


def output_count(n_samples: int, L: int, M: int) -> int:
    return -(-int(n_samples) * int(L) // int(M))


def resample_stream_counts(total_fed: int, L: int, M: int, P: int, final: bool = False) -> int:
    """Outputs a stream has emitted once ``total_fed`` input samples have arrived: output n reads inputs up to
    floor((n M + P) / L), so it is complete when L total_fed - 1 >= n M + P.  ``final`` (after ``flush``): every output of the
    signal, ceil(total_fed L / M)."""
    total_fed, L, M, P = int(total_fed), int(L), int(M), int(P)
    if final:
        return output_count(total_fed, L, M)
    return max(0, (L * total_fed - 1 - P) // M + 1)


def stream_keep_from(next_n: int, L: int, M: int, P: int) -> int:
    """The first input sample that output ``next_n`` (and so any later one) reads: ceil((next_n M - P) / L), at least 0."""
    return max(0, -(-(int(next_n) * int(M) - int(P)) // int(L)))


def _block(x, origin: int, first: int, count: int, L: int, M: int, taps) -> np.ndarray:
    """Outputs first .. first + count - 1 of the polyphase sum over a buffer whose sample 0 is input ``origin``; what lies
    outside the buffer is zero.  Sums in the dtype of ``taps``, terms added in t order (float64 here; tests restate it in float32)."""
    T = taps.shape[1]
    Kt = (T - 1) // 2
    acc = np.zeros((int(count),), dtype=taps.dtype)
    if count <= 0:
        return acc
    q0, r0 = divmod(int(first) * int(M), int(L))                     # Python ints: no 64-bit limit on n M
    v = r0 + np.arange(int(count), dtype=np.int64) * int(M)
    dq, phi = v // int(L), v % int(L)
    lo = q0 - Kt - int(origin)                                       # buffer index of the first sample output `first` reads
    span = int(dq[-1]) + T
    seg = np.zeros((span,), dtype=taps.dtype)
    a, b = max(lo, 0), min(lo + span, int(x.size))
    if b > a:
        seg[a - lo:b - lo] = x[a:b]
    for t in range(T):
        acc = acc + taps[phi, t] * seg[dq + (T - 1 - t)]
    return acc


def _as_float64(signal) -> np.ndarray:
    x = np.asarray(signal).reshape(-1)
    if x.dtype == np.int16:
        return x.astype(np.float64) / 32768.0
    if x.dtype.kind != "f":
        raise ValueError("resample: the signal is int16 PCM or floating point, got %s" % x.dtype)
    return x.astype(np.float64)


def resample(signal, rate_in, rate_out, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA) -> np.ndarray:
    """The definition: ceil(N L / M) float64 samples (int16 input is v / 32768)."""
    x = _as_float64(signal)
    L, M = ratio(rate_in, rate_out)
    if L == M:
        return x
    _, _, taps = polyphase(L, M, zeros, rolloff, beta)
    return _block(x, 0, 0, output_count(x.size, L, M), L, M, taps)


def resample_direct(signal, rate_in, rate_out, zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA) -> np.ndarray:
    """The double sum of the definition as it is written, for checking the polyphase form (slow: short signals only)."""
    x = _as_float64(signal)
    L, M = ratio(rate_in, rate_out)
    h = prototype(L, M, zeros, rolloff, beta)
    P = (h.size - 1) // 2
    y = np.zeros((output_count(x.size, L, M),), dtype=np.float64)
    for n in range(y.size):
        for m in range(max(0, -(-(n * M - P) // L)), min(x.size - 1, (n * M + P) // L) + 1):
            y[n] += h[n * M - m * L + P] * x[m]
    return y


def to_pcm16(y) -> np.ndarray:
    """clip(rint(y * 32768), -32768, 32767) as int16 (half to even): what a 16-bit file written by a resampling tool holds."""
    return np.clip(np.rint(np.asarray(y) * 32768.0), -32768, 32767).astype(np.int16)


def resample_tokens(signal, rate_in, rate_out, quantization_steps: int = 256, **kw) -> np.ndarray:
    from . import data
    return data.mulaw_encode_pcm16(to_pcm16(resample(signal, rate_in, rate_out, **kw)), quantization_steps)


def _finish_host(y, out, quantization_steps):
    from . import data
    if out == "float":
        return y
    pcm = to_pcm16(y)
    return pcm if out == "pcm16" else data.mulaw_encode_pcm16(pcm, quantization_steps)


# ---- the same sum on the device (libwavenet_resample.so: wn_resample) --------------------------------------------------------------
# Everything above is numpy and stays the definition; what follows runs it with one launch per 64 clips and needs torch and the
# built library.  Supported there: L and M in 1 .. 1024, T <= 2047 and a tile whose input span fits the LDS; the definition
# serves every other ratio, and a Resampler made without a device.

def _device_refusal(L: int, M: int, T: int):
    """None when wn_resample takes the ratio, else the reason, naming the value."""
    if not (1 <= L <= 1024 and 1 <= M <= 1024):
        return "L = %d, M = %d outside 1 .. 1024" % (L, M)
    if T > 2047:
        return "T = %d taps per output above 2047" % T
    span = (L - 1 + (RESAMPLE_TILE - 1) * M) // L + T
    if span * 4 > RESAMPLE_LDS_BYTES:
        return "a tile's span of %d samples needs %d bytes of LDS, the limit is %d" % (span, span * 4, RESAMPLE_LDS_BYTES)
    return None


class Resampler(object):
    """``Resampler(48000, 16000, device="cuda")(x)`` -> ceil(N L / M) float32 samples as a device tensor; ``out="pcm16"`` int16,
    ``out="tokens"`` int32 mu-law tokens of ``quantization_steps``.  ``x`` is int16 PCM or float32, numpy or a tensor on any
    device.  An output's bits depend on its own T input samples and the taps only -- not on the call, the batch, the chunking
    of a stream, a block's origin, or int16 versus the same values as float32.  ``device=None``, or a ratio the kernel
    refuses (``self.refusal`` says why): the numpy definition serves, in float64 (numpy arrays without a device)."""

    def __init__(self, rate_in, rate_out, device="cuda", zeros: int = ZEROS, rolloff: float = ROLLOFF, beta: float = BETA):
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.design = dict(zeros=int(zeros), rolloff=float(rolloff), beta=float(beta))
        self.L, self.M, self.P, self.T, taps = resample_tables(rate_in, rate_out, **self.design)
        self.identity = self.L == self.M
        self.refusal = None if self.identity else _device_refusal(self.L, self.M, self.T)
        self.device = None
        self.launches = 0
        self._lut = {}
        if device is not None:
            import torch
            self.device = torch.device(device)
        self.on_device = self.device is not None and self.device.type == "cuda" and not self.identity and self.refusal is None
        if self.on_device:
            import torch
            self.taps = torch.as_tensor(taps).to(self.device)
        else:
            self._taps64 = None if self.identity else polyphase(self.L, self.M, **self.design)[2]

    # -- inputs and outputs -----------------------------------------------------------------------------------------------------
    def count(self, n_samples: int) -> int:
        return int(n_samples) if self.identity else output_count(n_samples, self.L, self.M)

    def _check_out(self, out):
        if out not in OUT_KINDS:
            raise ValueError("Resampler: out = %r; one of %s" % (out, ", ".join(OUT_KINDS)))

    def _signal(self, x):
        """A contiguous int16 or float32 vector, on the device when there is one (numpy otherwise)."""
        if self.device is None:
            a = np.asarray(x.cpu() if hasattr(x, "cpu") else x).reshape(-1)
            if a.dtype != np.int16:
                if a.dtype.kind != "f":
                    raise ValueError("Resampler: the signal is int16 PCM or floating point, got %s" % a.dtype)
                a = a.astype(np.float32)
            return a
        import torch
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
        t = t.reshape(-1)
        if t.dtype != torch.int16:
            if not t.dtype.is_floating_point:
                raise ValueError("Resampler: the signal is int16 PCM or floating point, got %s" % t.dtype)
            t = t.to(torch.float32)
        return t.to(self.device).contiguous()

    def _table(self, quantization_steps):
        import torch
        from . import data
        q = int(quantization_steps)
        if q not in self._lut:
            data.mulaw_encode_pcm16(np.zeros(1, np.int16), q)                 # builds the table
            self._lut[q] = torch.as_tensor(data._LUT16[q].astype(np.int32)).to(self.device)
        return self._lut[q]

    def _to_device(self, a):
        import torch
        if a.dtype == np.float64:
            a = a.astype(np.float32)
        return torch.as_tensor(np.ascontiguousarray(a)).to(self.device)

    def _host(self, jobs, out, quantization_steps):
        """The numpy definition over the same jobs (no device, or a ratio the kernel refuses)."""
        res = []
        for x, origin, first, count, start, end in jobs:
            a = _as_float64(x.cpu().numpy() if hasattr(x, "cpu") else x)
            if self.identity:
                y = a[int(first) - int(origin):int(first) - int(origin) + int(count)]
            else:
                y = _block(a, origin, first, count, self.L, self.M, self._taps64)
            y = _finish_host(y, out, quantization_steps)
            res.append(y if self.device is None else self._to_device(y))
        return res

    def _identity_device(self, jobs, out, quantization_steps):
        import torch
        res = []
        for x, origin, first, count, start, end in jobs:
            y = x[int(first) - int(origin):int(first) - int(origin) + int(count)]
            if out == "float":
                y = y.to(torch.float32) / 32768.0 if y.dtype == torch.int16 else y.clone()
            else:
                if y.dtype != torch.int16:
                    y = torch.clamp(torch.round(y * 32768.0), -32768.0, 32767.0).to(torch.int16)
                if out == "tokens":
                    y = self._table(quantization_steps)[y.to(torch.int64) + 32768]
            res.append(y)
        return res

    # -- the launch -------------------------------------------------------------------------------------------------------------
    def _launch(self, jobs, out="float", quantization_steps=256):
        """jobs: (samples, origin, first, count, start, end) -> one tensor of ``count`` outputs each, in launches of at most
        RESAMPLE_MAX_CLIPS clips."""
        self._check_out(out)
        if self.device is None or not (self.on_device or self.identity):          # no GPU, or a ratio the kernel refuses
            return self._host(jobs, out, quantization_steps)
        if self.identity:
            return self._identity_device(jobs, out, quantization_steps)
        import torch
        from . import _lib, _resample
        dtype = {"float": torch.float32, "pcm16": torch.int16, "tokens": torch.int32}[out]
        lut = self._table(quantization_steps) if out == "tokens" else None
        outs = [torch.empty((int(j[3]),), dtype=dtype, device=self.device) for j in jobs]
        live = [i for i, j in enumerate(jobs) if int(j[3]) > 0]
        with torch.cuda.device(self.device):
            for kind in (torch.int16, torch.float32):                          # a launch reads one kind of input
                idx = [i for i in live if jobs[i][0].dtype == kind]
                for at in range(0, len(idx), RESAMPLE_MAX_CLIPS):
                    part = idx[at:at + RESAMPLE_MAX_CLIPS]
                    clips = (_resample.WnResampleClip * len(part))()
                    for c, i in enumerate(part):
                        x, origin, first, count, start, end = jobs[i]
                        clips[c].x, clips[c].n, clips[c].origin = x.data_ptr(), x.numel(), int(origin)
                        clips[c].out, clips[c].first, clips[c].count = outs[i].data_ptr(), int(first), int(count)
                        clips[c].flags = (_resample.WN_RESAMPLE_START if start else 0) | (_resample.WN_RESAMPLE_END if end else 0)
                    _resample.check(_resample.lib().wn_resample(
                        clips, len(part), _resample.WN_RESAMPLE_IN_PCM16 if kind == torch.int16 else _resample.WN_RESAMPLE_IN_F32,
                        _resample.OUT_KIND[out], _lib.ptr(self.taps), self.L, self.M, self.T, _lib.ptr(lut), _lib.stream_ptr()))
                    self.launches += 1
        return outs

    def batch(self, clips, out="float", quantization_steps=256):
        """A list of clips of any lengths -> a list of ceil(N_i L / M) outputs each, RESAMPLE_MAX_CLIPS clips per launch."""
        xs = [self._signal(x) for x in clips]
        n = lambda x: int(x.numel() if hasattr(x, "numel") else x.size)
        return self._launch([(x, 0, 0, self.count(n(x)), True, True) for x in xs], out, quantization_steps)

    def __call__(self, x, out="float", quantization_steps=256):
        return self.batch([x], out, quantization_steps)[0]

    def block(self, buffer, origin: int, first: int, count: int, start: bool = False, end: bool = False, out="float",
              quantization_steps=256):
        """Outputs first .. first + count - 1 of a signal whose sample ``origin`` is ``buffer[0]``; ``start`` / ``end``: the
        buffer's first / last sample is the signal's, zeros lie beyond.  Equals that slice of the whole call."""
        x = self._signal(buffer)
        n = int(x.numel() if hasattr(x, "numel") else x.size)
        origin, first, count = int(origin), int(first), int(count)
        if origin < 0 or first < 0 or count < 0 or (start and origin != 0):
            raise ValueError("Resampler.block: origin = %d, first = %d, count = %d%s" % (origin, first, count,
                                                                                       " with start" if start else ""))
        if count and not self.on_device:
            lo, hi = (first, first + count - 1) if self.identity else self.reach(first, count)
            if (lo < origin and not start) or (hi >= origin + n and not end) or (self.identity and (lo < origin or hi >= origin + n)):
                raise ValueError("Resampler.block: outputs %d .. %d read inputs %d .. %d, the buffer holds %d .. %d"
                                 % (first, first + count - 1, lo, hi, origin, origin + n - 1))
        return self._launch([(x, origin, first, count, start, end)], out, quantization_steps)[0]

    def reach(self, first: int, count: int):
        """(lowest, highest) input sample that outputs first .. first + count - 1 read: q - Kt of the first, q + Kt of the last."""
        Kt = (self.T - 1) // 2
        return (int(first) * self.M) // self.L - Kt, ((int(first) + int(count) - 1) * self.M) // self.L + Kt

    def stream(self, out="float", quantization_steps=256):
        return ResampleStream(self, out, quantization_steps)


class ResampleStream(object):
    """``Resampler.stream()``: ``feed(samples)`` returns the outputs that the samples fed so far complete (possibly none),
    ``flush()`` the rest, zeros behind the signal's end.  Whatever the chunking, the outputs concatenated are the one-shot
    call's, bit for bit; ``resample_stream_counts`` says how many there are after each call.  Only the inputs that a later
    output still reads are kept: from ceil((next_n M - P) / L) on.  (A polyphase row may begin or end with a zero tap, h's
    index falling outside [-P, P]: where such a tap's sample is not held, a zero stands in for it -- any finite value gives
    the same bits.)"""

    def __init__(self, rs: Resampler, out="float", quantization_steps=256):
        rs._check_out(out)
        self.rs, self.out, self.q = rs, out, quantization_steps
        self.total = 0           # inputs fed
        self.emitted = 0         # outputs returned
        self.start = 0           # input index of tail[0]
        self.tail = None
        self.closed = False

    def _cat(self, parts):
        if self.rs.device is None:
            return np.concatenate(parts)
        import torch
        return torch.cat(parts)

    def _zeros(self, k):
        if self.rs.device is None:
            return np.zeros((k,), dtype=self.tail.dtype)
        import torch
        return torch.zeros((k,), dtype=self.tail.dtype, device=self.rs.device)

    def _emit(self, upto: int, final: bool):
        rs = self.rs
        count = upto - self.emitted
        if count <= 0 or self.tail is None:
            return rs._launch([(self.tail if self.tail is not None else rs._signal(np.zeros(0, np.float32)), 0, 0, 0, True, True)],
                              self.out, self.q)[0]
        buf, origin = self.tail, self.start
        if not rs.identity:
            lo, hi = rs.reach(self.emitted, count)
            before = max(0, origin - lo) if origin > 0 else 0              # samples that only a zero tap reads
            behind = 0 if final else max(0, hi - (origin + len(buf) - 1))
            if before or behind:
                buf = self._cat(([self._zeros(before)] if before else []) + [buf] + ([self._zeros(behind)] if behind else []))
                origin -= before
        res = rs._launch([(buf, origin, self.emitted, count, origin == 0, final)], self.out, self.q)[0]
        self.emitted = upto
        keep_from = max(self.start, self.emitted if rs.identity else stream_keep_from(self.emitted, rs.L, rs.M, rs.P))
        if keep_from > self.start:
            cut = self.tail[keep_from - self.start:]
            self.tail = cut.copy() if rs.device is None else cut.clone()
            self.start = keep_from
        return res

    def _counts(self, final):
        rs = self.rs
        return self.total if rs.identity else resample_stream_counts(self.total, rs.L, rs.M, rs.P, final)

    def feed(self, samples):
        if self.closed:
            raise ValueError("Resampler.stream: feed after flush")
        x = self.rs._signal(samples)
        if self.tail is not None and x.dtype != self.tail.dtype:
            raise ValueError("Resampler.stream: %s samples fed to a stream of %s" % (x.dtype, self.tail.dtype))
        self.tail = x if self.tail is None else self._cat([self.tail, x])
        self.total += len(x)
        return self._emit(self._counts(False), False)

    def flush(self):
        if self.closed:
            raise ValueError("Resampler.stream: flush twice")
        self.closed = True
        return self._emit(self._counts(True), True)


_CACHE = {}


def resampler(rate_in, rate_out, device=None) -> Resampler:
    """The ``Resampler`` of a rate pair on a device, made once and kept."""
    key = (int(rate_in), int(rate_out), None if device is None else str(device))
    if key not in _CACHE:
        _CACHE[key] = Resampler(rate_in, rate_out, device=device)
    return _CACHE[key]
