"""CPU reference of local conditioning (van den Oord et al. 2016, eq. 4, with y = the features repeated over time), built on
the oracle without changing it.

A ``RefWaveNet`` whose residual layer adds a (cd, T) bias to each gate's convolution output: column t of it is row
(t + phase) // hop of the clip's block of per-frame rows -- ``V h[:, (t + phase) // hop]`` for features h (F, n) and the
projection V (sum_l 2 cd_l, F; rows layer-major, a layer's filter rows before its gate rows, as in tests/cond_ref.py) -- for
t >= Z and nothing below: Z is the zero prefix of ``conv_pad_and_prefix``, the rule cond_ref.py documents (for t < Z a d > 1
layer's convolution output, bias included, is exactly 0).  Everything is a torch expression of V and h, so autograd reaches
both.  With global conditioning also on, the clip's row V_g E[id] is added to every frame row of its clip."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import wavenet_ref as R

import cond_ref

TINY = cond_ref.TINY
B, T = cond_ref.B, cond_ref.T
FEATS = 5                                   # feature channels F
HOP, PHASE = 12, 5                          # 7 frames: borders inside tiles, a partial first and last frame


def frames_needed(T, hop, phase=0):
    return (T + phase + hop - 1) // hop


def init_local(p, feats=FEATS, frames=None, seed=77, scale=1.0, clips=B):
    """(V (rows, F), h (clips, F, frames)) float32."""
    rows = cond_ref.cond_rows(p)[1]
    frames = frames_needed(T, HOP, PHASE) if frames is None else frames
    rs = np.random.RandomState(seed)
    V = (rs.standard_normal((rows, feats)) * scale / np.sqrt(feats)).astype(np.float32)
    h = rs.standard_normal((clips, feats, frames)).astype(np.float32)
    return V, h


def state_dict(w, V, E=None, Vg=None):
    """Oracle weights + the conditioning tensors under the model's checkpoint keys."""
    sd = dict(w) if E is None else cond_ref.state_dict(w, E, Vg)
    sd["local_condition_projection/W"] = np.asarray(V, np.float32).reshape(V.shape[0], V.shape[1], 1, 1)
    return sd


class LocalRefWaveNet(R.RefWaveNet):
    """``rows``: (B, n, sum 2 cd) torch block of per-(clip, frame) gate biases; the batch the net is run on has B clips."""

    def set_rows(self, rows, hop, phase):
        self.rows, self.hop, self.phase = rows, int(hop), int(phase)
        self.slots = {pre: s for (_, _, _, pre), s in zip(self.layers(), cond_ref.cond_rows(self.p)[0])}
        return self

    def gate_bias(self, pre, d, Tn):
        """(B, cd, 1, T) filter and gate biases of layer ``pre``: the frame row of every column, 0 below the zero prefix."""
        of, og, cd = self.slots[pre]
        fw = self.p["residual_conv_filter_width"]
        Z = R.conv_pad_and_prefix(Tn, d, fw)[1]
        frame = torch.as_tensor((np.arange(Tn) + self.phase) // self.hop)
        live = torch.as_tensor((np.arange(Tn) >= Z)).to(self.rows.dtype).reshape(1, 1, 1, Tn)
        per_t = self.rows.index_select(1, frame)                                   # (B, T, R)
        bf = per_t[:, :, of:of + cd].permute(0, 2, 1).unsqueeze(2) * live
        bg = per_t[:, :, og:og + cd].permute(0, 2, 1).unsqueeze(2) * live
        return bf, bg

    def gates(self, x, pre, d):
        """Pre-activations (a, c) of the two gates."""
        fw = self.p["residual_conv_filter_width"]
        Wf, _ = self._W(pre + "wf")
        Wg, _ = self._W(pre + "wg")
        bf, bg = self.gate_bias(pre, d, x.shape[3])
        return R.dilated_conv_literal(x, Wf, None, d, fw) + bf, R.dilated_conv_literal(x, Wg, None, d, fw) + bg

    def residual_layer(self, x, pre, d):
        a, c = self.gates(x, pre, d)
        z = torch.tanh(a) * R._sigmoid_t(c)
        Wp, bp = self._W(pre + "projection_block")
        Ws, bs = self._W(pre + "projection_softmax")
        return F.conv2d(z, Wp, bp) + x, F.conv2d(z, Ws, bs), z


def rows_of(V, h, glob=None):
    """(B, n, R) block: V h[b, :, f] (+ the clip's global row (B, R))."""
    rows = torch.einsum("rc,bcf->bfr", V, h)
    return rows if glob is None else rows + glob.unsqueeze(1)


def stack_forward(p, w, x, rows, hop, phase, dtype=torch.float64):
    """The residual stack alone on a dense input x (B, Cr, 1, T) with the (B, n, sum 2 cd) block ``rows``: per layer
    (out, z, tanh, sigmoid) as (B, C, 1, T) numpy, the skip sum, and the largest |pre-activation| of any gate -- the float64
    target of the library-level tests (the shape of cond_ref.stack_forward's result)."""
    net = LocalRefWaveNet(p, w, dtype=dtype).set_rows(torch.tensor(np.asarray(rows), dtype=dtype), hop, phase)
    layers, total, amax = [], 0, 0.0
    with torch.no_grad():
        out = torch.tensor(x, dtype=dtype)
        for _, _, d, pre in net.layers():
            a, c = net.gates(out, pre, d)
            amax = max(amax, float(a.abs().max()), float(c.abs().max()))
            f, g = torch.tanh(a), R._sigmoid_t(c)
            out, skip, z = net.residual_layer(out, pre, d)
            layers.append((out.numpy(), z.numpy(), f.numpy(), g.numpy()))
            total = total + skip
    return layers, total.numpy(), amax


def train_step_grads(p, w, V, h, hop, phase, idx_in, target, dtype=torch.float32, E=None, Vg=None, ids=None):
    """loss, logits (B, Q, 1, Tw) and {name: gradient} for every weight of ``w`` plus ``"V"`` and ``"h"`` (and ``"E"`` /
    ``"Vg"`` with global conditioning also on).  The loss is the mean over all rows of all clips."""
    wt = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    Vt = torch.tensor(np.asarray(V), dtype=dtype, requires_grad=True)
    ht = torch.tensor(np.asarray(h), dtype=dtype, requires_grad=True)
    glob = None
    if E is not None:
        Et = torch.tensor(np.asarray(E), dtype=dtype, requires_grad=True)
        Vgt = torch.tensor(np.asarray(Vg), dtype=dtype, requires_grad=True)
        glob = Et[torch.as_tensor(np.asarray(ids, dtype=np.int64))] @ Vgt.t()
    net = LocalRefWaveNet(p, {}, dtype=dtype)
    net.w = dict(wt)
    net.set_rows(rows_of(Vt, ht, glob), hop, phase)
    loss, logits = net.train_loss(R.onehot_t(idx_in, p["quantization_steps"], dtype), target)
    loss.backward()
    g = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape), np.dtype(str(dtype).split(".")[1])))
         for k, v in wt.items()}
    g["V"], g["h"] = Vt.grad.numpy().copy(), ht.grad.numpy().copy()
    if E is not None:
        g["E"], g["Vg"] = Et.grad.numpy().copy(), Vgt.grad.numpy().copy()
    return float(loss.detach()), logits.detach().numpy(), g


def stack_row_grads(p, w, x, rows, hop, phase, dout, dskip, t_off, dtype=torch.float64):
    """d/d rows of sum(out * dout) + sum(skip[t_off:] * dskip) for the residual stack alone: the (B, n, sum 2 cd) gradient block
    that wn_stack_bwd accumulates into its dbf / dbg rows.  x, dout (B, Cr, 1, T), dskip (B, Cs, 1, T - t_off)."""
    rt = torch.tensor(np.asarray(rows), dtype=dtype, requires_grad=True)
    net = LocalRefWaveNet(p, w, dtype=dtype).set_rows(rt, hop, phase)
    out, skip = net.forward_residual_block(torch.tensor(x, dtype=dtype))
    obj = (out * torch.tensor(dout, dtype=dtype)).sum() + (skip[:, :, :, t_off:] * torch.tensor(dskip, dtype=dtype)).sum()
    obj.backward()
    return rt.grad.numpy().copy()


def colsum_in_kernel_order(a, ta, tb, t_chunk=256):
    """float32 sum of rows ta .. tb - 1 of ``a`` (T, M) in the documented order of k_colsum_per_clip / k_colsum_per_frame: chunks
    of ``t_chunk`` rows from ta, four row lanes per chunk combined as (p0 + p1) + (p2 + p3), chunk y on reduction lane y % 16
    in ascending order, the 16 lane sums in index order."""
    a = np.asarray(a, np.float32)
    M = a.shape[1]
    lanes = np.zeros((16, M), np.float32)
    nchunk = (tb - ta + t_chunk - 1) // t_chunk
    for y in range(nchunk):
        t0 = ta + y * t_chunk
        t1 = min(tb, t0 + t_chunk)
        p = np.zeros((4, M), np.float32)
        for t in range(t0, t1):
            p[(t - t0) % 4] = p[(t - t0) % 4] + a[t]
        lanes[y % 16] = lanes[y % 16] + ((p[0] + p[1]) + (p[2] + p[3]))
    tot = np.zeros((M,), np.float32)
    for k in range(16):
        tot = tot + lanes[k]
    return tot
