"""What the pitch-conditioning tests share: the small shape, four signals, a float32 numpy restatement of the channel map, and
numpy stand-ins for the two analysers' launches (the definitions, evaluated on a job's buffer)."""
import numpy as np

import pitch_ref as P
from wavenet_amd import data, features, pitch

RATE, WIN, HOP, FMIN, FMAX, MELS = 1600, 64, 16, 40.0, 400.0, 8
TAU_MIN, TAU_MAX, SPAN = 4, 40, 104
THRESHOLD = P.THRESHOLD
SPACING = P.SPACING                       # the float32 spacing at 1.0


def _mulaw(x):
    return data.mulaw_decode(data.mulaw_encode(np.clip(x, -1.0, 1.0), 256), 256)


def signals():
    """name -> float64 signal (through mu-law at Q = 256, so that tokens exist): a harmonic tone of 100 Hz, noise, silence, and a
    tone of 80 Hz that starts in the middle of the signal."""
    late = P.harmonic_tone(80.0, RATE, 2000)
    late[:1000] = 0.0
    return {"tone": _mulaw(P.harmonic_tone(100.0, RATE, 700)), "noise": _mulaw(0.2 * np.random.RandomState(1).randn(1001)),
            "silence": _mulaw(np.zeros(800)), "late": _mulaw(late)}


def chunkings(n):
    """name -> chunk lengths that sum to n: 1 sample, 7, one hop, 3 hops + 5, everything; empty feeds between."""
    out = {}
    for name, step in (("1", 1), ("7", 7), ("hop", HOP), ("3hops+5", 3 * HOP + 5), ("all", n)):
        parts = []
        for at in range(0, n, step):
            parts.append(min(step, n - at))
            if len(parts) % 3 == 1:
                parts.append(0)
        out[name] = [0] + parts
    return out


def channels_f32(rows, fmin, fmax):
    """``Pitch.channels`` in numpy, every operation in float32."""
    rows = np.asarray(rows, dtype=np.float32)
    lo, k = pitch.channel_constants(fmin, fmax)
    voiced = rows[0] > 0
    out = np.zeros((3, rows.shape[1]), dtype=np.float32)
    out[0, voiced] = 1.0
    out[1, voiced] = (np.log2(rows[0, voiced]) - lo) * k
    out[2] = np.minimum(rows[1], np.float32(1.0))
    assert out.dtype == np.float32
    return out


def _aligned(x, origin, hop):
    """(signal', m0): the buffer behind just enough zeros that its sample ``origin`` sits on a multiple m0 * hop."""
    shift = (-origin) % hop
    while origin + shift < 0:
        shift += hop
    return np.concatenate([np.zeros(shift), x]), (origin + shift) // hop


def numpy_pitch_launch(p, log=None):
    """A stand-in for ``Pitch._launch``: ``pitch.yin`` on each job's buffer (floats only).  The checks of the real launch are kept."""
    import torch

    def launch(jobs, quantization_steps, curve=False):
        assert quantization_steps is None and not curve
        outs = []
        for x, origin, first, count, start, end in jobs:
            x = np.asarray(x.cpu().numpy(), dtype=np.float64)
            if count:
                lo, hi = p.reach(origin, first, count)
                if (lo < 0 and not start) or (hi >= x.size and not end):
                    raise ValueError("Pitch: columns read samples %d .. %d of 0 .. %d" % (lo, hi, x.size - 1))
            sig, m0 = _aligned(x, origin, p.hop)
            m0 += first
            sig = np.concatenate([sig, np.zeros(max(0, (m0 + count) * p.hop - sig.size))])
            out = pitch.yin(sig, p.rate, p.hop, p.win, p.fmin, p.fmax, p.threshold)[:, m0:m0 + count]
            assert out.shape == (2, count)
            outs.append(torch.as_tensor(out.astype(np.float32)))
            if log is not None:
                log.append((int(x.size), int(origin), int(count), bool(start), bool(end)))
        p.launches += 1
        return outs
    return launch


def numpy_mel_launch(m):
    """A stand-in for ``LogMel._launch``: ``features.log_mel`` on each job's buffer (floats only).  A column that reflects must
    sit at a flagged edge of the buffer; zeros put in front for alignment are never read."""
    import torch

    def launch(jobs, quantization_steps):
        assert quantization_steps is None
        outs = []
        for x, origin, first, count, left, right in jobs:
            x = np.asarray(x.cpu().numpy(), dtype=np.float64)
            lo = origin + first * m.hop - m.win // 2
            hi = lo + (count - 1) * m.hop + m.win - 1
            assert (lo >= 0 or (left and origin % m.hop == 0)) and (hi < x.size or right)
            sig, m0 = _aligned(x, origin, m.hop)
            m0 += first
            out = features.log_mel(sig, m.rate, m.n_mels, m.hop, m.win)[:, m0:m0 + count]
            assert out.shape == (m.n_mels, count)
            outs.append(torch.as_tensor(out.astype(np.float32)))
        m.launches += 1
        return outs
    return launch
