"""CPU reference of global conditioning (van den Oord et al. 2016, eq. 3), built on the oracle without changing it.

To one clip, conditioning on class ``id`` IS an ordinary biased network: ``wf/b = Vf_l E[id]`` and ``wg/b = Vg_l E[id]`` in
every residual layer.  So the reference runs one ``RefWaveNet`` per clip with ``residual_conv_dilation_no_bias = False``
whose bias entries are torch expressions of the embedding ``E`` (classes, channels) and the projection ``V``
(sum_l 2 cd_l, channels; rows layer-major, a layer's filter rows before its gate rows), and autograd reaches ``E`` and ``V``
through them.  The oracle's zero-prefix rule applies to those biases as to any (for t < Z a d > 1 layer's convolution output,
bias included, is exactly 0).  The loss is the mean over all rows of all clips."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import wavenet_ref as R

# the tiny model and batch of the conditioning tests: three 32-column tiles per clip, the last one partial, so that one
# four-wave workgroup holds tiles of two clips; a repeated id and an unused class; the compatibility zero prefix is on
TINY = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 3, residual_num_blocks=2,
            softmax_conv_channels=[64, 256])
CLASSES, CHANNELS = 3, 8
B, T = 3, 70
IDS = [2, 0, 2]


def cond_rows(p):
    """[(filter offset, gate offset, cd)] per residual layer into the rows of V, and the number of rows."""
    out, off = [], 0
    for _ in range(p["residual_num_blocks"]):
        for cd in p["residual_conv_channels"]:
            out.append((off, off + cd, cd))
            off += 2 * cd
    return out, off


def init_condition(p, classes=CLASSES, channels=CHANNELS, seed=99, scale=1.0):
    rows = cond_rows(p)[1]
    rs = np.random.RandomState(seed)
    E = rs.standard_normal((classes, channels)).astype(np.float32)
    V = (rs.standard_normal((rows, channels)) * scale / np.sqrt(channels)).astype(np.float32)
    return E, V


def state_dict(w, E, V):
    """Oracle weights + the two conditioning tensors under the model's checkpoint keys."""
    sd = dict(w)
    sd["global_condition_embed/W"] = np.asarray(E, np.float32).reshape(E.shape[0], E.shape[1], 1, 1)
    sd["global_condition_projection/W"] = np.asarray(V, np.float32).reshape(V.shape[0], V.shape[1], 1, 1)
    return sd


def _clip_net(pb, wt, bias, dtype):
    net = R.RefWaveNet(pb, {}, dtype=dtype)
    net.w = dict(wt)
    for (of, og, cd), (_, _, _, pre) in zip(cond_rows(pb)[0], net.layers()):
        net.w[pre + "wf/b"] = bias[of:of + cd]
        net.w[pre + "wg/b"] = bias[og:og + cd]
    return net


def train_step_grads(p, w, E, V, ids, idx_in, target, dtype=torch.float32):
    """loss, logits (B, Q, 1, Tw) and {name: gradient} for every weight of ``w`` plus ``"E"`` and ``"V"``."""
    pb = dict(p, residual_conv_dilation_no_bias=False)
    wt = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in w.items()}
    Et = torch.tensor(np.asarray(E), dtype=dtype, requires_grad=True)
    Vt = torch.tensor(np.asarray(V), dtype=dtype, requires_grad=True)
    logits = []
    for b in range(idx_in.shape[0]):
        net = _clip_net(pb, wt, Vt @ Et[int(ids[b])], dtype)
        _, lg = net.train_loss(R.onehot_t(idx_in[b:b + 1], p["quantization_steps"], dtype), target[b:b + 1])
        logits.append(lg)
    logits = torch.cat(logits, dim=0)
    Bn, Q, _, Tw = logits.shape
    rows = logits.permute(0, 3, 2, 1).reshape(Bn * Tw, Q)                      # the oracle's cross_entropy, over all clips
    loss = F.cross_entropy(rows, torch.as_tensor(np.asarray(target).reshape(-1).astype(np.int64)))
    loss.backward()
    g = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape), np.dtype(str(dtype).split(".")[1])))
         for k, v in wt.items()}
    g["E"], g["V"] = Et.grad.numpy().copy(), Vt.grad.numpy().copy()
    return float(loss.detach()), logits.detach().numpy(), g


def loss_only(p, w, E, V, ids, idx_in, target, dtype=torch.float64):
    with torch.no_grad():
        pb = dict(p, residual_conv_dilation_no_bias=False)
        wt = {k: torch.tensor(v, dtype=dtype) for k, v in w.items()}
        Et, Vt = torch.tensor(np.asarray(E), dtype=dtype), torch.tensor(np.asarray(V), dtype=dtype)
        logits = []
        for b in range(idx_in.shape[0]):
            net = _clip_net(pb, wt, Vt @ Et[int(ids[b])], dtype)
            logits.append(net.train_loss(R.onehot_t(idx_in[b:b + 1], p["quantization_steps"], dtype), target[b:b + 1])[1])
        logits = torch.cat(logits, dim=0)
        Bn, Q, _, Tw = logits.shape
        rows = logits.permute(0, 3, 2, 1).reshape(Bn * Tw, Q)
        return float(F.cross_entropy(rows, torch.as_tensor(np.asarray(target).reshape(-1).astype(np.int64))))


def stack_forward(p, w, x, bias_rows, dtype=torch.float64):
    """The residual stack alone on a dense input x (B, Cr, 1, T) with per-clip bias rows (B, sum 2 cd): per layer
    (out, z, tanh, sigmoid) as (B, C, 1, T) numpy, the skip sum, and the largest |pre-activation| of any gate -- the float64
    target of the library-level tests."""
    pb = dict(p, residual_conv_dilation_no_bias=False)
    wt = {k: torch.tensor(v, dtype=dtype) for k, v in w.items()}
    fw = p["residual_conv_filter_width"]
    per_clip, amax = [], 0.0
    with torch.no_grad():
        for b in range(x.shape[0]):
            net = _clip_net(pb, wt, torch.tensor(np.asarray(bias_rows[b]), dtype=dtype), dtype)
            out = torch.tensor(x[b:b + 1], dtype=dtype)
            layers, total = [], 0
            for _, _, d, pre in net.layers():
                Wf, bf = net._W(pre + "wf")
                Wg, bg = net._W(pre + "wg")
                a, c = R.dilated_conv_literal(out, Wf, bf, d, fw), R.dilated_conv_literal(out, Wg, bg, d, fw)
                amax = max(amax, float(a.abs().max()), float(c.abs().max()))
                f, g = torch.tanh(a), R._sigmoid_t(c)
                out, skip, z = net.residual_layer(out, pre, d)
                layers.append((out.numpy(), z.numpy(), f.numpy(), g.numpy()))
                total = total + skip
            per_clip.append((layers, total.numpy()))
    L = len(per_clip[0][0])
    layers = [tuple(np.concatenate([pc[0][l][k] for pc in per_clip], axis=0) for k in range(4)) for l in range(L)]
    return layers, np.concatenate([pc[1] for pc in per_clip], axis=0), amax
