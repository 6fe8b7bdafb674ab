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
colsum_in_kernel_order = LR.colsum_in_kernel_order


def _fma32(w, d, p):
    """(float32 fma(w, d, p), entries that are not certain) for float32 arrays, through float64.  w * d is exact in float64 (two
    24-bit significands); the float64 sum is rounded to 53 bits and then to 24, which can differ from the single rounding of a
    fused multiply-add only when the float64 sum sits exactly on a float32 tie (its low 29 significand bits are 1 << 28) and
    was itself rounded.  TwoSum gives the float64 addition's error exactly: on such a tie the sum is nudged one float64 step
    towards the true value before the second rounding, which then falls on the right side.  Below the float32 normal range
    the tie lies elsewhere: those entries are reported, not trusted."""
    prod, p64 = np.atleast_1d(np.float64(w) * np.float64(d)), np.atleast_1d(np.float64(p))
    s = prod + p64
    bb = s - prod
    err = (prod - (s - bb)) + (p64 - bb)
    tie = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
    fix = tie & (err != 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32), (np.abs(s) < 2.0 ** -126) & (s != 0)


def colsum_lerp_in_kernel_order(a, f, hop, phase, tmin=0, t_chunk=32):
    """(float32 (M,) sum, number of suspect roundings): what k_colsum_per_frame_lerp adds to row ``f`` of a clip's gradient block
    from ``a`` (T, M), the clip's (da | dg) rows, in the documented order.  Two halves of 8 reduction lanes: the first takes
    the rows t >= tmin of frame f with weight 1 - alpha_t (one float32 subtraction), the second those of frame f - 1 with weight
    alpha_t, alpha_t = fl32(fl32(t - lo) / fl32(hop)) for a frame whose first position is lo.  Each segment is cut into chunks of
    ``t_chunk`` rows from its first row; a chunk's rows go to four row lanes, each row as ONE fused multiply-add p = fma(w, d,
    p), combined as (p0 + p1) + (p2 + p3); chunk y on lane y % 8 of its half in ascending order; the 16 partials added in index
    order.  The count is of the float64-emulated multiply-adds ``_fma32`` could not vouch for: 0 means the sum is the kernel's,
    bit for bit."""
    a = np.asarray(a, np.float32)
    T, M = a.shape
    lanes = np.zeros((16, M), np.float32)
    suspect = 0
    lo_own = f * hop - phase
    for half, lo in ((0, lo_own), (1, lo_own - hop)):
        ta, tb = max(lo, tmin), min(lo + hop, T)
        for y in range(max(0, (tb - ta + t_chunk - 1) // t_chunk)):
            t0 = ta + y * t_chunk
            p = np.zeros((4, M), np.float32)
            for t in range(t0, min(tb, t0 + t_chunk)):
                al = np.float32(t - lo) / np.float32(hop)
                w = al if half else np.float32(1) - al
                p[(t - t0) % 4], bad = _fma32(w, a[t], p[(t - t0) % 4])
                suspect += int(bad.sum())
            lanes[8 * half + y % 8] = lanes[8 * half + y % 8] + ((p[0] + p[1]) + (p[2] + p[3]))
    tot = np.zeros((M,), np.float32)
    for k in range(16):
        tot = tot + lanes[k]
    return tot, suspect
