"""Folded decoding on the host: the rule that cuts one long utterance into overlapping segments, aligns each segment's window,
uniforms and feature columns, and joins the decoded segments again.  Numpy only, no device: this module is the statement of the
rule, as ``sampling.py`` is for the draw; ``FasterWaveNet.generate_folded`` runs it on the device and equals it bit for bit.

A single utterance is a strict sample-to-sample chain, so one utterance decodes at the speed of one chain.  A locally
conditioned model does not need the chain to be unbroken: the features pin down what every stretch sounds like.  The segments
of a plan decode side by side as utterances of ONE ``generate_batch`` call and are cross-faded where they meet (WaveRNN
vocoders ship this as "batched mode").

Positions p = 0 .. n - 1 are the emitted samples of the utterance; p = 0 is the first sample behind its window of W_in samples.
With body B >= 1, overlap 0 <= O <= B and warm-up W >= 0, all in samples:

* S = max(1, ceil((n - O) / B)) segments; body u is [a_u, b_u) with a_u = u B, b_u = a_(u+1), b_(S-1) = n.  Every body but the
  last is B long; the last is longer than O and at most B + O.
* Segment u decodes [s_u, e_u): s_0 = 0, s_u = max(0, a_u - W); e_u = b_u + O, e_(S-1) = n.  [s_u, a_u) is warm-up, decoded and
  thrown away.  [b_u, b_u + O) is the seam: the tail of u and the head of u + 1.  No position outside a warm-up is covered by
  more than two segments.
* Window: a segment with s_u = 0 takes the utterance's own window; any other one a window of silence tokens -- its real
  context is unknown at launch time, which is what the warm-up is for.
* Uniforms are keyed by position: the utterance has ONE row U[0 .. n) and segment u draws with U[s_u : e_u].  So segment 0 IS
  the sequential chain, a plan of one segment is ``generate()``, and both sides of a seam see the same draw at the same
  position (common random numbers).
* Features: the utterance's columns cover it from the first sample of its window, at phase phi (``local_alignment``).  Segment
  u's window starts at window-inclusive index s_u: it gets the columns from (s_u + phi) // H on at phase (s_u + phi) % H, as
  many as ``coarse_frames_needed`` says for its W_in + (e_u - s_u) - 1 positions (``segment_columns``).
* Output: ``table[token]`` is the int16 value ``data.save_audio_file`` writes for a token (``data.pcm_table``).  Outside seams
  the owner's value is copied.  At seam index i, with t and h the two sides' values as float32 and
  w_i = float32((i + 0.5) / O) (the quotient made in float64): d = h - t; m = w_i * d; y = t + m -- three separately rounded
  float32 operations -- then round half to even and clip to int16.  Equal tokens on both sides give that token's value.
"""
from __future__ import annotations

import collections

import numpy as np

from .wavenet import coarse_frames_needed

# one segment: its body [a, b) and what it decodes, [s, e)
Segment = collections.namedtuple("Segment", "a b s e")
# ``fold_plan``'s answer: its arguments and the S segments
FoldPlan = collections.namedtuple("FoldPlan", "n body overlap warmup segments")


def _int(name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("fold: %s must be an integer, got %r" % (name, v))
    return int(v)


def check_fold(body, overlap, warmup):
    """The argument rules of a fold: body >= 1, 0 <= overlap <= body, warmup >= 0, integers all; ValueError naming the value."""
    B, O, W = _int("body", body), _int("overlap", overlap), _int("warmup", warmup)
    if B < 1:
        raise ValueError("fold: body must be at least 1 sample, got %d" % B)
    if O < 0 or O > B:
        raise ValueError("fold: overlap must lie in [0, body = %d], got %d" % (B, O))
    if W < 0:
        raise ValueError("fold: warmup must be >= 0 samples, got %d" % W)
    return B, O, W


def fold_plan(n, body, overlap, warmup) -> FoldPlan:
    """The plan of an utterance of ``n`` >= 1 emitted samples (the module's rule)."""
    n = _int("n", n)
    if n < 1:
        raise ValueError("fold: n must be at least 1 sample, got %d" % n)
    B, O, W = check_fold(body, overlap, warmup)
    S = max(1, -(-(n - O) // B))
    segs = []
    for u in range(S):
        a = u * B
        b = n if u == S - 1 else a + B
        segs.append(Segment(a, b, 0 if u == 0 else max(0, a - W), n if u == S - 1 else b + O))
    return FoldPlan(n, B, O, W, tuple(segs))


def auto_body(n, capacity, overlap, warmup) -> int:
    """``body="auto"``: max(4 (W + O), ceil(n / capacity)).  The second term fills ``capacity`` slots of a launch and no more;
    the first keeps B / (B + W + O) >= 4 / 5 -- at least 80 % of the decoded steps are samples of the result.  Derived, not tuned."""
    n, cap, O, W = _int("n", n), _int("capacity", capacity), _int("overlap", overlap), _int("warmup", warmup)
    if cap < 1:
        raise ValueError("fold: capacity must be at least 1, got %d" % cap)
    return max(1, 4 * (W + O), -(-n // cap))


def useful_share(plan) -> float:
    """The share of a plan's decoded steps that are samples of the result: n / sum (e_u - s_u)."""
    return plan.n / float(sum(g.e - g.s for g in plan.segments))


def segment_columns(s, e, window, phase, hop, interp="repeat", upsample=1):
    """(first column, column count, phase) of a segment that decodes [s, e) behind a window of ``window`` samples, for an
    utterance whose columns cover it from the first sample of its window at phase ``phase`` and hop ``hop``: the segment's
    window starts ``s`` samples later, so ``local_alignment(s + phase, hop)`` gives its first column and phase, and its
    ``window + (e - s) - 1`` positions read ``coarse_frames_needed`` columns from there (``interp``, ``upsample``: the model's
    ``local_interp`` / ``local_upsample``)."""
    s, e, hop = int(s), int(e), int(hop)
    if not 0 <= s < e or hop < 1 or not 0 <= int(phase) < hop:
        raise ValueError("segment_columns: needs 0 <= s < e, hop >= 1 and 0 <= phase < hop, got s %d, e %d, hop %d, phase %d"
                         % (s, e, hop, int(phase)))
    first, ph = divmod(s + int(phase), hop)
    return first, coarse_frames_needed(int(window) + (e - s) - 1, hop, int(upsample), ph, interp), ph


def check_columns(plan, window, phase, hop, interp, upsample, columns, what="fold"):
    """Every segment's ``segment_columns`` against the ``columns`` the utterance was given; raises naming the first segment whose
    count runs past them, and both counts.  Returns the list of (first, count, phase)."""
    out = []
    for u, g in enumerate(plan.segments):
        first, count, ph = segment_columns(g.s, g.e, window, phase, hop, interp, upsample)
        if first + count > int(columns):
            raise ValueError("%s: segment %d (samples %d .. %d) reads feature columns %d .. %d, the utterance has %d: %d are needed"
                             % (what, u, g.s, g.e, first, first + count - 1, int(columns), first + count))
        out.append((first, count, ph))
    return out


def owner(plan) -> np.ndarray:
    """(n,) int32: the segment whose body holds each position."""
    out = np.empty((plan.n,), dtype=np.int32)
    for u, g in enumerate(plan.segments):
        out[g.a:g.b] = u
    return out


def seam_weights(overlap) -> np.ndarray:
    """(O,) float32: w_i = float32((i + 0.5) / O), the quotient made in float64 -- the weight of the head side at seam index i."""
    O = int(overlap)
    return ((np.arange(O, dtype=np.float64) + 0.5) / max(O, 1)).astype(np.float32)


def fade_weights(plan) -> np.ndarray:
    """(S, n) float64: the weight each segment's sample has in each position of the result -- 1 for the owner outside seams,
    (1 - w_i, w_i) for the tail and the head of a seam, 0 elsewhere (warm-ups included)."""
    S, own = len(plan.segments), owner(plan)
    out = np.zeros((S, plan.n), dtype=np.float64)
    out[own, np.arange(plan.n)] = 1.0
    w = seam_weights(plan.overlap).astype(np.float64)
    for u in range(S - 1):
        b = plan.segments[u].b
        out[u, b:b + plan.overlap] = 1.0 - w
        out[u + 1, b:b + plan.overlap] = w
    return out


def _check_rows(rows, plan):
    rows = [np.asarray(r).reshape(-1) for r in rows]
    if len(rows) != len(plan.segments):
        raise ValueError("fold: %d rows for a plan of %d segments" % (len(rows), len(plan.segments)))
    for u, (r, g) in enumerate(zip(rows, plan.segments)):
        if r.size != g.e - g.s:
            raise ValueError("fold: row %d holds %d samples, segment %d decodes %d" % (u, r.size, u, g.e - g.s))
    return rows


def gather_owner(rows, plan) -> np.ndarray:
    """(n,): every position's value in its owner's row (tokens, or the probabilities of ``return_chosen``)."""
    rows = _check_rows(rows, plan)
    return np.concatenate([r[g.a - g.s:g.b - g.s] for r, g in zip(rows, plan.segments)])


def unfold(rows, plan, table) -> np.ndarray:
    """The utterance's (n,) int16 signal from the segments' token rows (``rows[u]``: the e_u - s_u tokens of segment u) and
    ``table`` (``data.pcm_table``): the module's output rule."""
    rows = _check_rows(rows, plan)
    table = np.asarray(table)
    out = table[gather_owner(rows, plan)].astype(np.int16)
    O = plan.overlap
    w = seam_weights(O)
    for u in range(len(plan.segments) - 1 if O else 0):
        g, h_seg = plan.segments[u], plan.segments[u + 1]
        t = table[rows[u][g.b - g.s:g.b - g.s + O]].astype(np.float32)
        h = table[rows[u + 1][g.b - h_seg.s:g.b - h_seg.s + O]].astype(np.float32)
        d = h - t
        m = w * d
        y = t + m
        out[g.b:g.b + O] = np.clip(np.rint(y), -32768.0, 32767.0).astype(np.int16)
    return out


def identical_seams(rows, plan) -> int:
    """The seams whose two sides hold equal tokens throughout (a seam of O = 0 samples holds nothing and counts)."""
    rows = _check_rows(rows, plan)
    O, count = plan.overlap, 0
    for u in range(len(plan.segments) - 1):
        g, h_seg = plan.segments[u], plan.segments[u + 1]
        count += int(np.array_equal(rows[u][g.b - g.s:g.b - g.s + O], rows[u + 1][g.b - h_seg.s:g.b - h_seg.s + O]))
    return count
