"""Sampling controls on the host: temperature, top-k and top-p (nucleus) in front of the categorical draw.

The reference draws every sample from the raw softmax (train_audio/generate.py:39: ``np.random.choice(..., p=softmax)``).
The decode kernels and ``wn_sample_categorical_filtered`` (include/wavenet_hip.h) can truncate the distribution first; this
module is the same rule in numpy, for callers that sample on the host (the step-by-step loop of train_audio/generate.py)
and as the statement of the contract.  Given a row ``p`` of float32 probabilities:

1. order: token j precedes token i iff ``p[j] > p[i]``, or ``p[j] == p[i]`` and ``j < i``; ``rank(i)`` is the number of
   tokens preceding i;
2. top-k: ``pk[i] = p[i]`` if ``rank(i) < top_k`` else 0 (``top_k == 0`` or ``top_k >= Q``: off);
3. top-p, relative to the mass top-k kept: ``total`` = float64 sum of ``pk`` in index order, ``before(i)`` = float64 sum, in
   index order, of ``pk[j]`` over the j preceding i; keep i iff ``before(i) < top_p * total``; the rank-0 token is always
   kept (``top_p >= 1``: off);
4. draw: excluded entries become 0.0f, kept entries keep their float32 value (no renormalisation in float32), and numpy's
   legacy ``choice`` runs on that row: float64 running sum, divide by the last entry, first index with ``cdf > u``.

5. given samples (``forced=`` of ``FasterWaveNet.generate`` / ``generate_batch``, ``WN_DECODER_FORCED_TOKENS`` in the library): a
   step whose entry of ``forced`` is a token of ``[0, Q)`` emits that token -- steps 1-4 do not run, the step's uniform is not
   looked at, and the probability reported for it is the untruncated ``p[token]``; a step whose entry is -1 runs steps 1-4 as
   ever.  ``draw_or_keep`` is the rule for one step, ``check_forced`` what a caller may pass.

Everything is integer and float64 arithmetic in a fixed order (``np.cumsum`` adds sequentially), so the token equals the
device's bit for bit when the probabilities do.  Temperature acts on the logits (``logits * (1.0f / temperature)`` in
float32, then the softmax): ``inv_temperature`` gives that factor.
"""
from __future__ import annotations

import math

import numpy as np


def check_controls(temperature=1.0, top_k=0, top_p=1.0) -> None:
    """The argument rules of ``wn_decoder_set_sampling``: raise ValueError for what the library refuses."""
    t = float(temperature)
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError("temperature must be finite and > 0, got %r" % (temperature,))
    if int(top_k) != top_k or int(top_k) < 0:
        raise ValueError("top_k must be an integer >= 0 (0 = off), got %r" % (top_k,))
    tp = float(top_p)
    if not (0.0 < tp <= 1.0):                   # False for NaN
        raise ValueError("top_p must lie in (0, 1], got %r" % (top_p,))


def controls_off(temperature=1.0, top_k=0, top_p=1.0, Q=None) -> bool:
    return float(temperature) == 1.0 and (int(top_k) == 0 or (Q is not None and int(top_k) >= Q)) and float(top_p) >= 1.0


def inv_temperature(temperature) -> np.float32:
    """``1.0f / temperature`` in float32: the factor the logits are multiplied by."""
    return np.float32(1.0) / np.float32(temperature)


def filter_probs(p, top_k=0, top_p=1.0) -> np.ndarray:
    """Steps 1-3 on one row: the float32 row with the excluded entries set to 0."""
    check_controls(1.0, top_k, top_p)
    p = np.asarray(p, dtype=np.float32)
    if p.ndim != 1:
        raise ValueError("filter_probs takes one row of probabilities")
    Q = p.shape[0]
    top_k, top_p = int(top_k), float(top_p)
    out = p.copy()
    if (top_k == 0 or top_k >= Q) and top_p >= 1.0:
        return out
    # a stable sort of -p lists the tokens in the order of step 1 (equal values stay in index order)
    order = np.argsort(-p.astype(np.float64), kind="stable")
    rank = np.empty(Q, dtype=np.int64)
    rank[order] = np.arange(Q)
    if 0 < top_k < Q:
        out[rank >= top_k] = np.float32(0.0)
    if top_p < 1.0:
        pk = out.astype(np.float64)
        total = np.cumsum(pk)[-1]
        thr = top_p * total
        # before(i): the preceding tokens' values added in INDEX order -- a sum per token, as the device forms it (a prefix
        # sum over the sorted row would add them in rank order and may round differently)
        keep = np.zeros(Q, dtype=bool)
        for i in range(Q):
            pre = (rank < rank[i])
            sel = np.where(pre, pk, 0.0)
            before = np.cumsum(sel)[-1]
            keep[i] = before < thr or rank[i] == 0
        out[~keep] = np.float32(0.0)
    return out


def choice_from_uniform(p, u) -> int:
    """numpy's legacy ``RandomState.choice(arange(Q), p=p)`` given its one ``random_sample()`` draw ``u``
    (generate.py:39)."""
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))
    cdf /= cdf[-1]
    return int(np.searchsorted(cdf, u, side="right"))


def sample(p, u, top_k=0, top_p=1.0) -> int:
    """Steps 1-4: the token drawn from the row ``p`` with the uniform ``u``."""
    return choice_from_uniform(filter_probs(p, top_k, top_p), u)


def check_forced(forced, n_samples, Q) -> np.ndarray:
    """``forced=`` of one utterance -> a 1-D int32 array of ``n_samples`` entries, each -1 (draw) or a token of ``[0, Q)``
    (emit as given).  Raises ValueError for anything else -- a wrong length, a non-integer dtype, a value outside
    ``{-1} | [0, Q)`` -- and names the first offending index.  Pure numpy: it runs before any device work."""
    a = np.asarray(forced.detach().cpu() if hasattr(forced, "detach") else forced)
    if a.dtype == bool or a.dtype.kind not in "iu":
        raise ValueError("forced must hold integers (-1: draw, a token of [0, %d): emit as given), got dtype %s" % (Q, a.dtype))
    if a.ndim != 1 or a.shape[0] != int(n_samples):
        raise ValueError("forced must be a 1-D array of n_samples = %d entries, got shape %s" % (int(n_samples), a.shape))
    wide = a.astype(np.int64)
    bad = np.flatnonzero((wide < -1) | (wide >= int(Q)))
    if bad.size:
        raise ValueError("forced[%d] = %d is neither -1 (draw) nor a token of [0, %d)" % (bad[0], wide[bad[0]], Q))
    return np.ascontiguousarray(wide.astype(np.int32))


def draw_or_keep(prob, u, forced_i, temperature=1.0, top_k=0, top_p=1.0) -> int:
    """Step 5 for one step: the given token when ``forced_i`` is one, else the draw of steps 1-4 from the row ``prob`` with
    the uniform ``u``.  ``prob`` is the post-temperature row (``temperature`` acts on the logits, before this function: it is
    taken for the argument check only)."""
    check_controls(temperature, top_k, top_p)
    if int(forced_i) != -1:
        if not 0 <= int(forced_i) < len(prob):
            raise ValueError("forced entry %d is neither -1 nor a token of [0, %d)" % (int(forced_i), len(prob)))
        return int(forced_i)
    return sample(prob, u, top_k, top_p)


def apply_temperature(logits, temperature) -> np.ndarray:
    """float32 softmax of ``logits * (1.0f / temperature)`` over the last axis (host arithmetic: close to, not bit-equal
    with, the device's ``expf``)."""
    x = np.asarray(logits, dtype=np.float32)
    if float(temperature) != 1.0:
        x = x * inv_temperature(temperature)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


def per_utterance(value, n, name="control"):
    """A scalar or a length-``n`` sequence -> a list of ``n`` values."""
    if np.ndim(value) == 0:
        return [value] * n
    vals = list(value)
    if len(vals) != n:
        raise ValueError("%s: expected a scalar or %d values, got %d" % (name, n, len(vals)))
    return vals


def chosen_nll(chosen) -> float:
    """Nats per sample of one utterance from the probabilities of the tokens it emitted (``generate(..., return_chosen=True)``:
    a 1-D array or tensor): the float64 mean of ``-log(float64(p))`` -- the number ``evaluate`` prints for held-out audio,
    here for generated audio.  ``inf`` when a token of probability 0.0 was drawn (the fallback at the end of the cumulative
    distribution); 0.0 for no samples."""
    p = np.asarray(chosen.detach().cpu() if hasattr(chosen, "detach") else chosen, dtype=np.float64).reshape(-1)
    if p.size == 0:
        return 0.0
    with np.errstate(divide="ignore"):
        return float(np.mean(-np.log(p)))


def pick_best(nlls) -> int:
    """The index of the smallest of ``nlls`` (the candidate the model found most likely), the lowest index on ties.  NaN never
    wins: it is passed over, and index 0 comes back only when every value is NaN."""
    vals = [float(v) for v in nlls]
    if not vals:
        raise ValueError("pick_best: no candidate")
    best = 0
    for i, v in enumerate(vals):
        if not math.isnan(v) and (math.isnan(vals[best]) or v < vals[best]):
            best = i
    return best
