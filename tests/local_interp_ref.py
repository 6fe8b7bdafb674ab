"""CPU reference of local conditioning with LINEAR INTERPOLATION between feature frames, a float64 restatement of the one
rule everything implements, built on tests/local_cond_ref.py without changing it.

Column (row) k of a clip's block is anchored at the first position of its frame, k * hop.  Position t of a clip reads, with
p = t + phase, j = p // hop and alpha = float32(p % hop) / float32(hop) -- the weight is the float32 quotient the kernels
form, carried into the reference's dtype unchanged --

    y(t) = r[j] + alpha * (r[j + 1] - r[j])

for t >= Z and nothing below (Z: the zero prefix of ``conv_pad_and_prefix``, as in local_cond_ref.py).  A window of T
positions therefore reads ``frames_needed(T, hop, phase) + 1`` rows: the last position reads row j + 1 whatever its alpha.
Everything is a torch expression of the rows, so autograd gives row f the sum of (1 - alpha_t) d[t] over the t >= Z of frame f
plus the sum of alpha_t d[t] over the t >= Z of frame f - 1."""
import numpy as np
import torch

from oracle import wavenet_ref as R

import cond_ref
import local_cond_ref as LR

TINY, B, T, FEATS, HOP, PHASE = LR.TINY, LR.B, LR.T, LR.FEATS, LR.HOP, LR.PHASE


def frames_needed(T, hop, phase=0):
    """Rows a window of T positions reads in linear mode: one more than the frames it spans."""
    return LR.frames_needed(T, hop, phase) + 1


def init_local(p, feats=FEATS, frames=None, seed=77, scale=1.0, clips=B):
    return LR.init_local(p, feats, frames_needed(T, HOP, PHASE) if frames is None else frames, seed, scale, clips)


def weights(Tn, hop, phase):
    """(j (Tn,) int64, alpha (Tn,) float32): the frame of every position and the float32 weight of the next row."""
    pos = np.arange(Tn, dtype=np.int64) + int(phase)
    j = pos // int(hop)
    alpha = (pos % int(hop)).astype(np.float32) / np.float32(hop)
    return j, alpha


class LinearRefWaveNet(LR.LocalRefWaveNet):
    def gate_bias(self, pre, d, Tn):
        of, og, cd = self.slots[pre]
        fw = self.p["residual_conv_filter_width"]
        Z = R.conv_pad_and_prefix(Tn, d, fw)[1]
        j, alpha = weights(Tn, self.hop, self.phase)
        al = torch.as_tensor(alpha.astype(np.float64)).to(self.rows.dtype).reshape(1, Tn, 1)
        a = self.rows.index_select(1, torch.as_tensor(j))
        b = self.rows.index_select(1, torch.as_tensor(j + 1))
        per_t = a + al * (b - a)                                                    # (B, T, R)
        live = torch.as_tensor((np.arange(Tn) >= Z)).to(self.rows.dtype).reshape(1, 1, 1, Tn)
        bf = per_t[:, :, of:of + cd].permute(0, 2, 1).unsqueeze(2) * live
        bg = per_t[:, :, og:og + cd].permute(0, 2, 1).unsqueeze(2) * live
        return bf, bg


def _with(fn, *a, **k):
    """Run a function of local_cond_ref with its network class replaced by the interpolating one."""
    keep = LR.LocalRefWaveNet
    LR.LocalRefWaveNet = LinearRefWaveNet
    try:
        return fn(*a, **k)
    finally:
        LR.LocalRefWaveNet = keep


def stack_forward(p, w, x, rows, hop, phase, dtype=torch.float64):
    return _with(LR.stack_forward, p, w, x, rows, hop, phase, dtype=dtype)


def train_step_grads(p, w, V, h, hop, phase, idx_in, target, dtype=torch.float32, E=None, Vg=None, ids=None):
    return _with(LR.train_step_grads, p, w, V, h, hop, phase, idx_in, target, dtype=dtype, E=E, Vg=Vg, ids=ids)


def stack_row_grads(p, w, x, rows, hop, phase, dout, dskip, t_off, dtype=torch.float64):
    return _with(LR.stack_row_grads, p, w, x, rows, hop, phase, dout, dskip, t_off, dtype=dtype)


state_dict = LR.state_dict
rows_of = LR.rows_of
