"""Teacher-forced scoring: how well a model fits audio, in nats (or bits) per sample.

New capability (the reference trains and generates; it never evaluates).  ``score(net, tokens)`` returns the negative
log-likelihood of every sample of a token sequence given all samples before it:

    nll[i] = -log softmax(net(s[i : i + C]))[:, last column][tokens[i]],     s = C silence tokens ++ tokens

with C = :func:`context_width`, the number of input columns the last output column of a window depends on.  Output column
C - 1 of a window is the first one that depends neither on where the window starts nor on the reference's zero-prefix rule
(the columns before it see the window's own left edge), so a long signal is cut into overlapping pieces of C - 1 context
columns plus up to ``chunk_width`` scored columns, ``batch_size`` pieces per launch: the result does not depend on either
knob beyond arithmetic (the fp16x2 kernels scale per tile, and the tiles move with the cut).

The per-row values come from ``WaveNet.token_nll``: where the library covers it, the last head convolution and the rows
are one launch (``wn_head_xent`` under WN_EXEC_HEAD_ROW_NLL) and neither logits nor a gradient reach memory.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np


def silence_token(quantization_steps: int) -> int:
    """The token train_audio pads with before a file's first sample (train_audio/train.py:53; generation starts from the same token)."""
    return 127 if quantization_steps > 127 else quantization_steps // 2


def context_width(params) -> int:
    """C = 1 + sum over all causal and residual layers of (filter width - 1) * dilation: the input columns the network's
    last output column depends on.  With the default filter widths (2) this is ``WaveNet.input_width``."""
    fwc, fwr = params.causal_conv_filter_width, params.residual_conv_filter_width
    c = 1 + (fwc - 1) * len(params.causal_conv_channels)
    for _ in range(params.residual_num_blocks):
        for li in range(len(params.residual_conv_channels)):
            c += (fwr - 1) * fwr ** li
    return c


def plan_chunks(n: int, chunk_width: int, batch_size: int) -> List[List[Tuple[int, int]]]:
    """The launches that score samples [0, n): a list of launches, each a list of at most ``batch_size`` pieces
    (start, width) of ONE width (they form the rows of a batch).  Read in order, the pieces cover [0, n) exactly once:
    full launches of ``batch_size`` pieces of ``chunk_width``, then the remaining full pieces as a smaller batch, then
    the ragged tail alone."""
    if n < 0 or chunk_width < 1 or batch_size < 1:
        raise ValueError("plan_chunks: n >= 0, chunk_width >= 1 and batch_size >= 1 (got %d, %d, %d)" % (n, chunk_width, batch_size))
    full, tail = divmod(n, chunk_width)
    pieces = [(k * chunk_width, chunk_width) for k in range(full)]
    plan = [pieces[k:k + batch_size] for k in range(0, full, batch_size)]
    if tail:
        plan.append([(full * chunk_width, tail)])
    return plan


def summarize(nll) -> Dict[str, float]:
    """{"samples", "nats_per_sample", "bits_per_sample"} of per-sample negative log-likelihoods in nats (a numpy array or a
    tensor), summed in float64.  No samples: both rates are 0."""
    a = np.asarray(nll.detach().cpu().numpy() if hasattr(nll, "detach") else nll, dtype=np.float64).reshape(-1)
    nats = float(a.sum() / a.size) if a.size else 0.0
    return {"samples": int(a.size), "nats_per_sample": nats, "bits_per_sample": nats / math.log(2.0)}


def score(net, tokens, chunk_width: int = 16384, batch_size: int = 8, condition=None, local=None):
    """(n,) float32 on the device: see the module text.  ``tokens``: a 1-D integer numpy array or tensor.  ``condition``: the
    class id of the sequence (every piece of it), for a globally conditioned model.

    ``local``: the sequence's (F, >= ceil(n / H)) features for a locally conditioned model (hop H): sample i of the sequence,
    as a network input, reads column i // H (``local_alignment`` with s0 = the piece's first sample); the silence in front of
    the first sample reads column 0.  The pieces of one launch share one phase, so ``chunk_width`` must be a multiple of H
    (raises otherwise); the result still does not depend on ``chunk_width`` or ``batch_size`` beyond arithmetic.  With
    ``local_interp="linear"`` every sample also reads the column after its own, so ``local`` needs ceil(n / H) + 1 columns
    and neighbouring pieces overlap by one column.  With a learned upsampling layer (``local_upsample`` = U > 1) ``local``
    needs ``coarse_frames_needed(n, H, U, 0, interp)`` columns -- the layer reads pairs of neighbouring columns."""
    import torch
    t = net.to_variable(np.asarray(tokens) if not isinstance(tokens, torch.Tensor) else tokens)
    if t.dim() != 1 or t.is_floating_point():
        raise Exception("score: tokens must be a 1-D integer sequence, got %s %s" % (t.dtype, tuple(t.shape)))
    if not t.is_cuda:
        raise Exception("score: the network is not on a HIP device (call to_gpu() first)")
    n = int(t.shape[0])
    if condition is not None and np.ndim(condition) != 0:
        raise Exception("score: condition must be ONE class id (the sequence is one clip)")
    net._condition_ids(None if condition is None else [int(condition)], 1)      # raises on a mismatch before any work
    C = context_width(net.params)
    ext = None
    if getattr(net, "local_channels", 0):
        H = net.local_hop
        if local is None:
            net._local_features(None, 1, 1)                                      # raises: a locally conditioned model needs features
        if int(chunk_width) % H:
            raise Exception("score: a locally conditioned model needs chunk_width %% local_hop == 0 (the pieces of one launch "
                            "share a phase), got chunk_width = %d, hop = %d" % (int(chunk_width), H))
        f = local if isinstance(local, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(local, dtype=np.float32)))
        if f.dim() != 2:
            raise Exception("score: local must be (F, frames) features of the one sequence, got %s" % (tuple(f.shape),))
        f = net._local_features(f[None], 1, max(n, 1), 0)[0][0]                  # raises on channels, dtype or too few columns
        pad_cols = (C + H - 1) // H                                              # the silence in front reads column 0
        ext = torch.cat([f[:, :1].expand(f.shape[0], pad_cols), f], dim=1)
        shift = pad_cols * H - C                                                 # input j of `s` below sits at extended position j + shift
    elif local is not None:
        net._local_features(local, 1, 1)                                         # raises: features for a model that takes none
    out = torch.empty((n,), device=t.device, dtype=torch.float32)
    t = t.to(torch.int32)
    s = torch.cat([torch.full((C,), silence_token(net.params.quantization_steps), device=t.device, dtype=torch.int32), t])
    for launch in plan_chunks(n, int(chunk_width), int(batch_size)):
        w = launch[0][1]
        # piece (start, w): inputs s[start : start + C - 1 + w]; output column C - 1 + k predicts s[start + C + k] = tokens[start + k]
        x = torch.stack([s[a:a + C - 1 + w] for a, _ in launch])
        tgt = torch.stack([t[a:a + w] for a, _ in launch])
        cond = None if condition is None else [int(condition)] * len(launch)
        kw = {}
        if ext is not None:
            ph = (launch[0][0] + shift) % H
            need = (C - 1 + w + ph + H - 1) // H + (1 if getattr(net, "local_interp", "repeat") == "linear" else 0)
            if getattr(net, "local_upsample", 1) > 1:                            # a learned upsampling layer reads pairs of columns
                from .wavenet import coarse_frames_needed
                need = coarse_frames_needed(C - 1 + w, H, net.local_upsample, ph, net.local_interp)
            kw = dict(local=torch.stack([ext[:, (a + shift) // H:(a + shift) // H + need] for a, _ in launch]).contiguous(),
                      local_phase=ph)
        out[launch[0][0]:launch[-1][0] + w] = net.token_nll(x, tgt, condition=cond, **kw).reshape(-1)
    return out
