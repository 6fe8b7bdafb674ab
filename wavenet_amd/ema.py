"""The schedule of the exponential moving average of the weights (``WaveNet.enable_ema``; new capability: the reference
generates from the raw iterates).

After every optimiser step the average ``e`` moves towards the weights ``w``: ``e += (1 - decay_t) (w - e)``
(``wn_rule_step`` with ``WN_RULE_EMA``).  With ``warmup`` the decay grows with the number of steps made, the rule of
TensorFlow's ``ExponentialMovingAverage(decay, num_updates)``: the first step uses 0.1, so the initial weights the
average starts from are forgotten quickly instead of weighing on it for ~1 / (1 - decay) steps."""
from __future__ import annotations

import numpy as np


def ema_decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """The decay of the averaging step made after ``t`` earlier ones: ``min(decay, (1 + t) / (10 + t))`` with ``warmup``,
    else ``decay``."""
    if t < 0:
        raise ValueError("t must be >= 0, got %r" % (t,))
    decay = float(decay)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_rate_at(t: int, decay: float, warmup: bool = True) -> np.float32:
    """What the kernel is handed for that step: ``1 - decay_t``, computed in float64 and rounded to fp32 once."""
    return np.float32(1.0 - ema_decay_at(t, decay, warmup))


def check_decay(decay: float) -> float:
    decay = float(decay)
    if not (0.0 <= decay <= 1.0):                                   # false for NaN
        raise ValueError("the EMA decay must lie in [0, 1], got %r" % (decay,))
    return decay
