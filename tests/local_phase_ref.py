"""CPU reference of local conditioning with A PHASE PER CLIP, built on tests/local_cond_ref.py (repeat mode) and
tests/local_interp_ref.py (linear mode) without changing either: the reference of the scalar-phase rule is run clip by clip,
clip b with its own phase, and the results are concatenated.  Position t of clip b reads, with p = t + phases[b], frame
p // hop (and, in linear mode, moves towards frame p // hop + 1 by float32(p % hop) / float32(hop)).

A block holds the rows of the worst phase, hop - 1 -- ``rows_needed`` -- whatever the phases are; a clip's reference run is
handed the clip's whole block and touches the rows its own phase reads, so the gradient of every other row is exactly 0.
Weight gradients are summed over clips; row (and feature) gradients are per clip."""
import numpy as np

import local_cond_ref as LR
import local_interp_ref as LI

TINY, B, T, FEATS, HOP = LR.TINY, LR.B, LR.T, LR.FEATS, LR.HOP
PHASES = (0, 5, 11)                         # one clip on a column border, one inside a column, one on a column's last position


def _mod(interp):
    return LI if interp else LR


def rows_needed(Tn, hop, interp):
    """Rows of a clip's block: ceil((T + hop - 1) / hop), one more in linear mode."""
    return (Tn + 2 * hop - 2) // hop + (1 if interp else 0)


def rows_read(Tn, hop, phase, interp):
    """Rows a clip of this phase reads (a prefix of its block)."""
    return (Tn + phase + hop - 1) // hop + (1 if interp else 0)


def stack_forward(p, w, x, rows, hop, phases, interp):
    """local_cond_ref.stack_forward's result for a batch whose clip b has phase phases[b]: per layer (out, z, tanh, sigmoid)
    as (B, C, 1, T) numpy, the skip sum, the largest |pre-activation|."""
    per = [_mod(interp).stack_forward(p, w, x[b:b + 1], rows[b:b + 1], hop, int(ph)) for b, ph in enumerate(phases)]
    L = len(per[0][0])
    layers = [tuple(np.concatenate([c[0][l][k] for c in per], axis=0) for k in range(4)) for l in range(L)]
    return layers, np.concatenate([c[1] for c in per], axis=0), max(c[2] for c in per)


def stack_row_grads(p, w, x, rows, hop, phases, interp, dout, dskip, t_off):
    """The (B, n, sum 2 cd) gradient block of the residual stack alone, clip b under phases[b]."""
    return np.concatenate([_mod(interp).stack_row_grads(p, w, x[b:b + 1], rows[b:b + 1], hop, int(ph), dout[b:b + 1],
                                                        dskip[b:b + 1], t_off) for b, ph in enumerate(phases)], axis=0)


def train_step_grads(p, w, V, h, hop, phases, interp, idx_in, target, E=None, Vg=None, ids=None):
    """loss, logits (B, Q, 1, Tw) and {name: gradient} of the whole model, the loss the mean over all rows of all clips: every
    clip contributes 1 / B of its own mean (the clips hold equally many rows)."""
    n = len(phases)
    loss, logits, grads = 0.0, [], {}
    for b, ph in enumerate(phases):
        kw = {} if E is None else dict(E=E, Vg=Vg, ids=np.asarray(ids)[b:b + 1])
        l, lg, g = _mod(interp).train_step_grads(p, w, V, h[b:b + 1], hop, int(ph), idx_in[b:b + 1], target[b:b + 1], **kw)
        loss += l / n
        logits.append(lg)
        for k, v in g.items():
            if k == "h":
                grads.setdefault(k, []).append(v / n)
            else:
                grads[k] = grads.get(k, 0) + v.astype(np.float64) / n
    grads["h"] = np.concatenate(grads["h"], axis=0)
    return loss, np.concatenate(logits, axis=0), {k: np.asarray(v, np.float32) for k, v in grads.items()}
