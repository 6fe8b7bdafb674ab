"""CPU reference of the learned upsampling layer ahead of the local projection (``local_upsample`` = U), a float64 numpy
restatement of the layer and of its alignment rule, built next to tests/local_cond_ref.py / local_interp_ref.py /
local_phase_ref.py without changing them.

The layer: coarse columns h_k (F values each, hop H) -> fine columns y_m (hop H' = H / U), for q in [0, U)

    y[:, k U + q] = W[qF:(q+1)F, :F] h_k + W[qF:(q+1)F, F:] h_k+1

so n coarse columns make (n - 1) U fine ones, fine column m anchored at position m H'.  Alignment: a window whose position 0
lies ``phase`` positions into coarse column 0 starts at fine column c0 = phase // H' with phase' = phase % H' and reads
``fine_needed`` fine columns from there; that takes ceil((c0 + nf) / U) + 1 coarse columns (``coarse_needed``)."""
import numpy as np

import local_cond_ref as LR

TINY, B, T, FEATS, HOP = LR.TINY, LR.B, LR.T, LR.FEATS, LR.HOP
PHASES = (0, 5, 11)


def initial_weight(U, F, dtype=np.float32):
    """The starting weight, entry by entry from the rule: W[qF + c, c] = 1 - q / U, W[qF + c, F + c] = q / U, 0 elsewhere; the
    quotient is the float32 one (float32(q) / float32(U)) for ``dtype`` float32 and the float64 one for float64."""
    w = np.zeros((U * F, 2 * F), dtype)
    for q in range(U):
        a = dtype(q) / dtype(U)
        for c in range(F):
            w[q * F + c, c] = dtype(1) - a
            w[q * F + c, F + c] = a
    return w


def random_weight(U, F, seed=5):
    return (np.random.RandomState(seed).standard_normal((U * F, 2 * F)) / np.sqrt(2 * F)).astype(np.float32)


def upsample(W, h):
    """(B, F, n) -> (B, F, (n - 1) U) in float64, column by column from the rule."""
    W, h = np.asarray(W, np.float64).reshape(-1, 2 * h.shape[1]), np.asarray(h, np.float64)
    Bn, F, n = h.shape
    U = W.shape[0] // F
    y = np.zeros((Bn, F, (n - 1) * U))
    for k in range(n - 1):
        for q in range(U):
            y[:, :, k * U + q] = h[:, :, k] @ W[q * F:(q + 1) * F, :F].T + h[:, :, k + 1] @ W[q * F:(q + 1) * F, F:].T
    return y


def upsample_grads(W, h, dy):
    """(dW (U F, 2 F), dh (B, F, n)) in float64 from the fine features' gradient dy (B, F, (n - 1) U): the pair-matrix product
    and the add-back of its two halves onto columns k and k + 1."""
    h, dy = np.asarray(h, np.float64), np.asarray(dy, np.float64)
    W = np.asarray(W, np.float64).reshape(-1, 2 * h.shape[1])
    Bn, F, n = h.shape
    U = W.shape[0] // F
    pairs = np.concatenate([h[:, :, :-1], h[:, :, 1:]], axis=1).transpose(0, 2, 1).reshape(Bn * (n - 1), 2 * F)
    d2 = dy.transpose(0, 2, 1).reshape(Bn * (n - 1), U * F)            # row (b, k): fine columns k U .. k U + U - 1, F each
    dW = d2.T @ pairs
    dp = (d2 @ W).reshape(Bn, n - 1, 2 * F)
    dh = np.zeros((Bn, n, F))
    dh[:, :-1] += dp[:, :, :F]
    dh[:, 1:] += dp[:, :, F:]
    return dW, dh.transpose(0, 2, 1)


def fine_needed(Tn, fine_hop, phase, interp):
    return (Tn + phase + fine_hop - 1) // fine_hop + (1 if interp == "linear" else 0)


def alignment(H, U, phase):
    """(H', c0, phase') of an int phase in [0, H)."""
    fine = H // U
    return fine, phase // fine, phase % fine


def coarse_needed(Tn, H, U, phase, interp):
    """Coarse columns a window reads; ``phase`` None: a phase per clip (c0 = U - 1, phase' = H' - 1)."""
    fine = H // U
    c0, ph = (U - 1, fine - 1) if phase is None else (phase // fine, phase % fine)
    return -(-(c0 + fine_needed(Tn, fine, ph, interp)) // U) + 1


def lerp(cols, hop, phase, Tn, float32_alpha=False):
    """(B, F, Tn) float64: linear interpolation between the columns ``cols`` (B, F, n) at ``hop`` positions per column, position
    t at p = t + phase reading cols[p // hop] moved towards the next by (p % hop) / hop (the exact quotient, or the float32
    one the kernels form)."""
    cols = np.asarray(cols, np.float64)
    p = np.arange(Tn) + phase
    j, r = p // hop, p % hop
    al = (r.astype(np.float32) / np.float32(hop)).astype(np.float64) if float32_alpha else r / float(hop)
    return cols[:, :, j] + al * (cols[:, :, j + 1] - cols[:, :, j])


def layer_then_lerp(W, h, H, U, phase, Tn):
    """What a ``local_interp="linear"`` model with the layer feeds position t, before the projection: the layer, the cut at
    c0, and interpolation at hop H' and phase'."""
    fine, c0, ph = alignment(H, U, phase)
    y = upsample(W, h)
    nf = fine_needed(Tn, fine, ph, "linear")
    assert c0 + nf <= y.shape[2]
    return lerp(y[:, :, c0:c0 + nf], fine, ph, Tn)
