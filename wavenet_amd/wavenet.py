"""`WaveNet` / `Params` with the reference's Python face, backed by libwavenet_hip.so.

Drop-in for wavenet.py of musyoku/wavenet: same class, method and hyper-parameter names (including
``update_laerning_rate``), same logical tensor shapes ``(B, C, 1, T)`` and the same numerical
conventions (zero prefix of the reshape-trick convolution, activation before every head conv,
cross-entropy row order).  Nothing here computes on the CPU: every forward / backward FLOP is a HIP
kernel reached through the C ABI in include/wavenet_hip.h, and calling a forward method without a
GPU raises.  PyTorch supplies device memory, streams and the autograd tape only.

Memory layout: activations live time-major / channel-minor, ``x[b][t][c]``; the tensors handed back
to the caller are ``(B, C, 1, T)`` *views* of that storage (``torch.channels_last`` strides), so the
reference's indexing (``out[0, :, 0, -1]``) works unchanged and no transpose is ever materialised on
the hot path.  T-contiguous inputs (numpy one-hot images) are converted once at the boundary.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, ptr_array, int_array, stream_ptr, ACT


# ----------------------------------------------------------------------------------------------
# hyper-parameters (wavenet.py:100-173): same fields, same defaults, same checks
# ----------------------------------------------------------------------------------------------
class Params(object):
    def __init__(self, dict=None):
        self.quantization_steps = 256
        self.sampling_rate = 8000
        self.causal_conv_no_bias = True
        self.causal_conv_filter_width = 2
        self.causal_conv_channels = [128]
        self.residual_conv_dilation_no_bias = True
        self.residual_conv_projection_no_bias = True
        self.residual_conv_filter_width = 2
        self.residual_conv_channels = [32, 32, 32, 32, 32, 32, 32, 32, 32]
        self.residual_num_blocks = 2
        self.softmax_conv_no_bias = False
        self.softmax_conv_channels = [128, 256]
        self.optimizer = "adam"
        self.weight_decay = 0
        self.momentum = 0.9
        self.gradient_clipping = 1.0
        if dict:
            self.from_dict(dict)

    def from_dict(self, dict):
        for attr, value in dict.items():
            if hasattr(self, attr):           # unknown keys are ignored, wavenet.py:151-154
                setattr(self, attr, value)

    def to_dict(self):
        return {attr: value for attr, value in self.__dict__.items()}

    def dump(self):
        print("params:")
        for attr, value in self.__dict__.items():
            print("	{}: {}".format(attr, value))

    def check(self):
        base = Params()
        for attr in self.__dict__:
            if not hasattr(base, attr):
                raise Exception("invalid parameter '{}'".format(attr))
        if self.quantization_steps != self.softmax_conv_channels[-1]:
            raise Exception("quantization_steps != softmax_conv_channels[-1]")


def zero_prefix(T: int, d: int, fw: int) -> int:
    """Columns the reference's reshape trick leaves at exactly 0 (wavenet.py:303-340)."""
    if d == 1:
        return 0
    pad = (-T) % d
    if (T + pad) // d < fw:
        pad += (fw - (T + pad) // d) * d
    return max(0, (fw - 1) * d - pad)


# ----------------------------------------------------------------------------------------------
# tensor plumbing
# ----------------------------------------------------------------------------------------------
def _need_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise _lib.WaveNetHipError(
            "this operation runs on the MI355X only: call to_gpu() first (there is no CPU path)")


def _as_view(btc: torch.Tensor) -> torch.Tensor:
    """(B,T,C) storage -> the reference's logical (B,C,1,T) shape, zero copy."""
    B, T, Cc = btc.shape
    return btc.view(B, T, 1, Cc).permute(0, 3, 2, 1)


def _to_btc(x: torch.Tensor) -> torch.Tensor:
    """Logical (B,C,1,T) tensor -> dense (B,T,C) storage; zero copy when x is one of our views."""
    if x.dim() != 4 or x.shape[2] != 1:
        raise Exception("expected a (B, C, 1, T) tensor, got %s" % (tuple(x.shape),))
    B, Cc, _, T = x.shape
    st = x.stride()
    if (st[1] == 1 or Cc == 1) and (st[3] == Cc or T == 1) and (st[0] == T * Cc or B == 1):
        return x.permute(0, 3, 2, 1).reshape(B, T, Cc)          # a view: memory already (B,T,C)
    if x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and not x.requires_grad:
        out = torch.empty((B, T, Cc), device=x.device, dtype=torch.float32)
        check(_lib.lib().wn_nchw_to_btc(ptr(x), ptr(out), B, Cc, T, stream_ptr()), "wn_nchw_to_btc")
        return out
    return x.permute(0, 3, 2, 1).reshape(B, T, Cc).contiguous()


class _Fn(torch.autograd.Function):
    """Base for the autograd nodes below.  Weight gradients are accumulated by the kernels straight
    into the model's flat gradient arena (``p.grad`` are views of it), so backward returns None for
    weights and tensors only for activations."""


class _EmbedFn(_Fn):
    @staticmethod
    def forward(ctx, idx, W, b, fw, net):
        B, T = idx.shape
        Cc, Q = W.shape[0], W.shape[1]
        out = torch.empty((B, T, Cc), device=idx.device, dtype=torch.float32)
        check(_lib.lib().wn_embed_fwd(ptr(idx), ptr(W), ptr(b), ptr(out), B, T, Q, Cc, fw, stream_ptr()),
              "wn_embed_fwd")
        ctx.save_for_backward(idx)
        ctx.W, ctx.b, ctx.fw, ctx.net = W, b, fw, net
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        B, T = idx.shape
        dout = dout.contiguous()
        check(_lib.lib().wn_embed_bwd(ptr(idx), ptr(dout), ptr(W.grad), ptr(None if b is None else b.grad), B, T,
                                      W.shape[1], W.shape[0], ctx.fw, ctx.net._exec(B, T), stream_ptr()), "wn_embed_bwd")
        return None, None, None, None, None


class _ConvFn(_Fn):
    """Dense dilated causal convolution (DilatedConvolution1D.__call__)."""

    @staticmethod
    def forward(ctx, x, W, b, fw, d, Z, hook):
        B, T, Cin = x.shape
        Cout = W.shape[0]
        x = x.contiguous()
        out = torch.empty((B, T, Cout), device=x.device, dtype=torch.float32)
        check(_lib.lib().wn_conv_fwd(ptr(x), ptr(W), ptr(b), ptr(out), B, T, Cin, Cout, fw, d, Z, stream_ptr()),
              "wn_conv_fwd")
        ctx.save_for_backward(x)
        ctx.W, ctx.b, ctx.geom = W, b, (fw, d, Z)
        return out

    @staticmethod
    def backward(ctx, dout):
        (x,) = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        fw, d, Z = ctx.geom
        B, T, Cin = x.shape
        dout = dout.contiguous()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        check(_lib.lib().wn_conv_bwd(ptr(x), ptr(W), ptr(dout), ptr(dx), ptr(W.grad),
                                     ptr(None if b is None else b.grad), B, T, Cin, W.shape[0], fw, d, Z,
                                     stream_ptr()), "wn_conv_bwd")
        return dx, None, None, None, None, None, None


class _PointwiseFn(_Fn):
    """out = W act(x) + b  (head convs, projection convs)."""

    @staticmethod
    def forward(ctx, x, W, b, act, net):
        lead = x.shape[:-1]
        Cin, Cout = x.shape[-1], W.shape[0]
        x2 = x.reshape(-1, Cin).contiguous()
        out = torch.empty((x2.shape[0], Cout), device=x.device, dtype=torch.float32)
        check(_lib.lib().wn_pointwise_fwd(ptr(x2), ptr(W), ptr(b), ptr(out), x2.shape[0], Cin, Cout, act,
                                          net._exec(), stream_ptr()), "wn_pointwise_fwd")
        ctx.save_for_backward(x2)
        ctx.W, ctx.b, ctx.act, ctx.lead, ctx.net = W, b, act, lead, net
        return out.view(*lead, Cout)

    @staticmethod
    def backward(ctx, dout):
        (x2,) = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        Cout, Cin = W.shape[0], x2.shape[1]
        dout2 = dout.reshape(-1, Cout).contiguous()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        check(_lib.lib().wn_pointwise_bwd(ptr(x2), ptr(W), ptr(dout2), ptr(dx), ptr(W.grad),
                                          ptr(None if b is None else b.grad), x2.shape[0], Cin, Cout, ctx.act,
                                          ctx.net._exec(), stream_ptr()), "wn_pointwise_bwd")
        return (None if dx is None else dx.view(*ctx.lead, Cin)), None, None, None, None


class _SoftmaxFn(_Fn):
    @staticmethod
    def forward(ctx, x):
        Q = x.shape[-1]
        x2 = x.reshape(-1, Q).contiguous()
        out = torch.empty_like(x2)
        check(_lib.lib().wn_softmax_fwd(ptr(x2), ptr(out), x2.shape[0], Q, stream_ptr()), "wn_softmax_fwd")
        ctx.save_for_backward(out)
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, dout):   # not on the reference's training path (train.py:76 passes apply_softmax=False)
        (p,) = ctx.saved_tensors
        g = dout.reshape(p.shape)
        return (p * (g - (g * p).sum(-1, keepdim=True))).view(dout.shape)


class _XentFn(_Fn):
    @staticmethod
    def forward(ctx, logits, target, n_norm=0):
        N, Q = logits.shape
        buf = torch.empty((_lib.XENT_LOSS_WORDS,), device=logits.device, dtype=torch.float32)
        dlog = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        check(_lib.lib().wn_softmax_xent(ptr(logits), ptr(target), ptr(buf), ptr(dlog), N, Q, int(n_norm), stream_ptr()),
              "wn_softmax_xent")
        ctx.dlog = dlog
        return buf[0]                                               # 0-dim view: buf[1:] are the per-workgroup sums

    @staticmethod
    def backward(ctx, dloss):
        # dlog was written by the forward for an upstream gradient of 1; scale it in place by the actual one, read from
        # device memory (no host sync, and no pass over the 8.4 M values when it is 1)
        dlog, ctx.dlog = ctx.dlog, None
        if dlog is None:
            raise RuntimeError("the cross-entropy node can be backpropagated once (its gradient buffer is scaled in place)")
        d = dloss.to(torch.float32).reshape(1).contiguous()
        check(_lib.lib().wn_scale_by_dev(ptr(dlog), ptr(d), dlog.numel(), stream_ptr()), "wn_scale_by_dev")
        return dlog, None, None


class _HeadXentFn(_Fn):
    """The last head convolution and the softmax cross-entropy as ONE node and one launch (wn_head_xent): the logits are formed
    and consumed on the chip.  forward_softmax_block(apply_softmax=False) followed by cross_entropy (wavenet.py:584-617) gives
    the same loss and the same gradients through two nodes and a (N, Q) logits tensor in memory."""

    @staticmethod
    def forward(ctx, x, W, b, target, act, n_norm, net):
        lead = x.shape[:-1]
        Cin, Cout = x.shape[-1], W.shape[0]
        x2 = x.reshape(-1, Cin).contiguous()
        N = x2.shape[0]
        buf = torch.empty((_lib.XENT_LOSS_WORDS,), device=x.device, dtype=torch.float32)
        dlog = torch.empty((N, Cout), device=x.device, dtype=torch.float32)
        check(_lib.lib().wn_head_xent(ptr(x2), ptr(W), ptr(b), ptr(target), ptr(buf), ptr(dlog), N, Cin, Cout, act,
                                      int(n_norm), net._exec(), stream_ptr()), "wn_head_xent")
        ctx.save_for_backward(x2)
        ctx.W, ctx.b, ctx.act, ctx.lead, ctx.net, ctx.dlog = W, b, act, lead, net, dlog
        return buf[0]

    @staticmethod
    def backward(ctx, dloss):
        (x2,) = ctx.saved_tensors
        dlog, ctx.dlog = ctx.dlog, None
        if dlog is None:
            raise RuntimeError("the fused head + cross-entropy node can be backpropagated once (its gradient buffer is scaled in place)")
        W, b = ctx.W, ctx.b
        Cout, Cin = W.shape[0], x2.shape[1]
        lib = _lib.lib()
        if not ctx.net._unit_upstream:       # (TrainStepGraph backpropagates a constant 1: not even the launch that would find that out)
            d = dloss.to(torch.float32).reshape(1).contiguous()
            check(lib.wn_scale_by_dev(ptr(dlog), ptr(d), dlog.numel(), stream_ptr()), "wn_scale_by_dev")
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        check(lib.wn_pointwise_bwd(ptr(x2), ptr(W), ptr(dlog), ptr(dx), ptr(W.grad), ptr(None if b is None else b.grad),
                                   x2.shape[0], Cin, Cout, ctx.act, ctx.net._exec(), stream_ptr()), "wn_pointwise_bwd")
        return (None if dx is None else dx.view(*ctx.lead, Cin)), None, None, None, None, None, None


class _StackFn(_Fn):
    """All residual layers + the deferred skip sum as ONE autograd node and ONE library call each way
    (WaveNet.forward_residual_block, wavenet.py:572-582)."""

    @staticmethod
    def forward(ctx, x, anchor, net, t_off, train, window_only=False, cond=None, rows=None):
        # `anchor` is a dummy leaf that requires grad: it keeps this node on the tape even when x
        # does not require grad, because the weights are not tensor inputs of the node.
        # `cond` (conditioning): the block of gate biases of _CondFn / _LocalFn, handed to the library as bias rows
        # (WN_EXEC_BIAS_PER_CLIP); the backward returns the block's gradient.  `rows` is its GateBiasRows -- how the block is
        # addressed -- and goes with it: both or neither.
        ctx.set_materialize_grads(False)
        B, T, Cr = x.shape
        x = x.contiguous()
        if rows is None:
            desc, ex = net._stack_desc(), net._exec(B, T)
        else:
            rows.check(B, T)
            desc, ex, ckeep = rows.call(B, T)
        L = len(net._flat_layers)
        ncd = sum(lay.cd for lay in net._flat_layers)
        dev_ = x.device
        xs = torch.empty((L, B, T, Cr), device=dev_, dtype=torch.float32)
        z = torch.empty((B * T * ncd,), device=dev_, dtype=torch.float32)
        # tanh is saved only when the backward cannot take the chained path (which recovers it as z / sigmoid)
        f = torch.empty_like(z) if train and _lib.lib().wn_stack_saves_tanh(desc, ex) else None
        g = torch.empty_like(z) if train else None
        skip = torch.empty((B, T - t_off, net._Cs), device=dev_, dtype=torch.float32)
        check(_lib.lib().wn_stack_fwd(desc, ptr(x), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(skip), B, T, t_off,
                                      1 if net.compat_zero_prefix else 0, 1 if window_only else 0, ex,
                                      stream_ptr()), "wn_stack_fwd")
        ctx.net, ctx.t_off, ctx.shape, ctx.window_only = net, t_off, (B, T, Cr), bool(window_only)
        ctx.saved = (x, xs, z, f, g) if train else None
        ctx.cond = cond if train else None
        ctx.rows = rows
        net._last_layer_inputs = [x] + [xs[l] for l in range(L - 1)]      # FasterWaveNet seeds its rings from these
        return xs[L - 1], skip

    @staticmethod
    def backward(ctx, dout, dskip):
        net, t_off = ctx.net, ctx.t_off
        B, T, Cr = ctx.shape
        if ctx.saved is None:
            raise _lib.WaveNetHipError("backward through a forward that ran without grad enabled")
        x, xs, z, f, g = ctx.saved
        cond = ctx.cond
        if ctx.window_only and dout is not None:
            raise _lib.WaveNetHipError("forward_residual_block(window_only=True) computed only what the skip window needs: "
                                       "the residual output cannot carry a gradient")
        lib = _lib.lib()
        desc = net._stack_desc()
        gt = net._grad_tables()
        nbytes = lib.wn_stack_bwd_workspace_bytes(desc, B, T)
        ws = torch.empty((nbytes // 4,), device=x.device, dtype=torch.float32)
        dout = None if dout is None else dout.contiguous()
        dskip = None if dskip is None else dskip.contiguous()
        dx = torch.empty((B, T, Cr), device=x.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        dcond, ex, dbf, dbg = None, net._exec(B, T), gt["bf"], gt["bg"]
        if cond is not None:
            # per-clip bias-gradient rows accumulate (+=) into a zeroed block: the gradient of the conditioning block
            dcond = torch.zeros_like(cond)
            desc, ex, ckeep = ctx.rows.call(B, T)
            dbf, dbg = ctx.rows.grad_tables(dcond)
        check(lib.wn_stack_bwd(desc, ptr(x), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(dout), ptr(dskip), ptr(dx),
                               gt["wf"], dbf, gt["wg"], dbg, gt["wp"], gt["bp"], gt["ws"], gt["bs"],
                               ptr(ws), nbytes, B, T, t_off, 1 if net.compat_zero_prefix else 0, ex,
                               stream_ptr()), "wn_stack_bwd")
        ctx.saved = ctx.cond = None
        return dx, None, None, None, None, None, dcond, None


LOCAL_INTERP = ("repeat", "linear")


class LocalPhases(object):
    """A phase per clip, checked and on the device: ``tab`` is an int32 (B,) tensor whose entries lie in [0, ``hop``).  What
    ``_local_features`` makes of a ``local_phase=`` sequence and what the stack node points ``WnStackDesc.bias_phase_tab`` at.
    Passing one as ``local_phase=`` hands the tensor through as it stands -- no copy, no read-back: ``TrainStepGraph`` keeps
    one as the static buffer its captured step reads and refills it (``fill``) between replays."""

    def __init__(self, tab, hop):
        self.tab, self.hop = tab, int(hop)

    def __len__(self):
        return int(self.tab.shape[0])

    def fill(self, values):
        """Refill the device buffer from a checked host array (``check_local_phases``)."""
        self.tab.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.int32)), non_blocking=False)


class GateBiasRows(object):
    """The gate-bias rows one stack call reads (and its backward accumulates), with how they are addressed: what the library
    is told through WN_EXEC_BIAS_PER_CLIP and WnStackDesc.bias_*.  ``block`` (contiguous, on the device) is (B, sum 2 cd), a row
    per clip -- global conditioning, ``hop`` = 0 -- or (B, n, sum 2 cd), a row per (clip, frame of ``hop`` positions), frames
    one block row apart -- local conditioning.  Layer l's filter row lies at ``net._cond_offsets[l][0]`` of a block row, its
    gate row at ``[l][1]``.  ``phase``: an int, or a ``LocalPhases``, whose int32 device tensor becomes
    ``WnStackDesc.bias_phase_tab`` (bias_phase stays 0; this object keeps it alive for the backward).  ``interp`` = 1: linear
    interpolation between the rows (``WnStackDesc.bias_interp``), which reads one row more."""

    def __init__(self, net, block, hop=0, phase=0, interp=0):
        self.net, self.block, self.hop, self.phase, self.interp = net, block, int(hop), phase, int(interp)
        self.tab = phase if isinstance(phase, LocalPhases) else None

    @property
    def worst_phase(self) -> int:
        """The largest phase a clip can have: with a phase per clip, the columns of hop - 1, whatever the phases are."""
        return self.hop - 1 if self.tab is not None else int(self.phase)

    @property
    def clip_stride(self) -> int:
        """Floats between consecutive clips' rows (WnExec.reserved)."""
        return self.net._cond_rows * (int(self.block.shape[1]) if self.hop else 1)

    def check(self, B, T):
        """The block's shape against a call of B clips of T positions."""
        shape, width = tuple(self.block.shape), self.net._cond_rows
        if not self.hop:
            if shape != (B, width):
                raise _lib.WaveNetHipError("conditioning block is %s, expected %s" % (shape, (B, width)))
            return
        need = frames_needed(T, self.hop, self.worst_phase, LOCAL_INTERP[self.interp])
        if len(shape) != 3 or shape[0] != B or shape[2] != width or shape[1] < need:
            raise _lib.WaveNetHipError("local conditioning block is %s, expected (%d, >= %d, %d)" % (shape, B, need, width))

    def grad_tables(self, block):
        """(bf, bg) pointer tables into clip 0's rows of ``block`` (this block, or a gradient block of its shape): layer l's
        filter and gate rows."""
        p0, offsets = block.data_ptr(), self.net._cond_offsets
        bf = (C.c_void_p * len(offsets))(*[p0 + 4 * of for of, _ in offsets])
        bg = (C.c_void_p * len(offsets))(*[p0 + 4 * og for _, og in offsets])
        return bf, bg

    def _descriptor(self):
        """(d, bf, bg): a copy of the model's stack descriptor whose bf / bg tables point into the block, with the frames'
        geometry filled in."""
        net = self.net
        net._stack_desc()
        d = _lib.WnStackDesc()
        for name, _ in _lib.WnStackDesc._fields_:
            setattr(d, name, getattr(net._sdesc, name))
        bf, bg = self.grad_tables(self.block)
        d.bf, d.bg = C.cast(bf, C.POINTER(C.c_void_p)), C.cast(bg, C.POINTER(C.c_void_p))
        if self.hop:
            tab = self.tab
            if tab is not None and (len(tab) != self.block.shape[0] or tab.hop != self.hop or tab.tab.dtype != torch.int32
                                    or tab.tab.device != self.block.device or not tab.tab.is_contiguous()):
                raise _lib.WaveNetHipError("the per-clip phases must be a contiguous int32 (%d,) tensor on the block's device, "
                                           "checked against hop %d" % (self.block.shape[0], self.hop))
            d.bias_hop, d.bias_frame_stride, d.bias_interp = self.hop, net._cond_rows, self.interp
            d.bias_phase = 0 if tab is not None else int(self.phase)
            d.bias_phase_tab = None if tab is None else tab.tab.data_ptr()
        return d, bf, bg

    def call(self, B, T):
        """(descriptor, WnExec, what must stay alive) of a forward or backward call on these rows: the descriptor of
        ``_descriptor`` and the call's WN_EXEC_BIAS_PER_CLIP context."""
        d, bf, bg = self._descriptor()
        ex = self.net._exec(B, T, _lib.WN_EXEC_BIAS_PER_CLIP, bias_stride=self.clip_stride)
        return C.byref(d), ex, (d, bf, bg)

    def call16(self, B, T):
        """(descriptor, what must stay alive) of a bf16-storage call on these rows.  The wn16_* calls take no WnExec: the
        descriptor alone says that there are rows (bf / bg and a row stride, also with one row per clip) and how they are
        addressed, and there is no field for a clip stride -- clip blocks are dense, so a block of frames holds exactly the
        rows the call needs (``forward_residual_block`` trims)."""
        keep = self._descriptor()
        d = keep[0]
        d.bias_frame_stride = self.net._cond_rows
        if self.hop:
            need = frames_needed(T, self.hop, self.worst_phase, LOCAL_INTERP[self.interp])
            if int(self.block.shape[1]) != need:
                raise _lib.WaveNetHipError("bf16 storage takes dense clip blocks: the local conditioning block holds %d rows per "
                                           "clip, the call reads %d" % (int(self.block.shape[1]), need))
        return C.byref(d), keep


def _one_phase(phase) -> bool:
    """True for the int form of ``local_phase=`` (anything 0-dimensional), False for a phase per clip."""
    if isinstance(phase, LocalPhases):
        return False
    return phase.dim() == 0 if isinstance(phase, torch.Tensor) else np.ndim(phase) == 0


def check_local_phases(phase, B, hop):
    """``local_phase=`` given as a 1-D sequence, numpy array or integer torch tensor -> int32 numpy (B,), every entry in
    [0, hop); anything else raises before any device work and names the first offending clip.  (A device tensor is read
    back for the check: pass a ``LocalPhases`` where that matters.)"""
    a = phase.detach().cpu().numpy() if isinstance(phase, torch.Tensor) else np.asarray(phase)
    if a.ndim != 1:
        raise Exception("local_phase= takes an int or one phase per clip (a 1-D sequence), got shape %s" % (tuple(a.shape),))
    if a.shape[0] != B:
        raise Exception("local_phase= holds %d phases for %d clips" % (a.shape[0], B))
    if a.dtype.kind not in "iu":
        raise Exception("local_phase= takes integer phases, got %s (clip 0)" % a.dtype)
    bad = np.nonzero((a < 0) | (a >= hop))[0]
    if bad.size:
        raise Exception("local_phase= must lie in [0, local_hop = %d), got %d for clip %d" % (hop, int(a[bad[0]]), int(bad[0])))
    return a.astype(np.int32)


def frames_needed(T: int, hop: int, phase: int = 0, interp: str = "repeat") -> int:
    """Feature columns a window of ``T`` positions reads at ``hop`` positions per column, the first position ``phase`` positions
    into its column: ceil((T + phase) / hop); one more with ``interp="linear"``, where every position also reads the column
    after its own."""
    if interp not in LOCAL_INTERP:
        raise Exception("interp must be 'repeat' or 'linear', got %r" % (interp,))
    return (int(T) + int(phase) + int(hop) - 1) // int(hop) + (1 if interp == "linear" else 0)


def coarse_frames_needed(T: int, hop: int, upsample: int = 1, phase=0, interp: str = "repeat") -> int:
    """Feature columns at hop ``hop`` that a window of ``T`` positions reads through a learned upsampling layer of factor
    ``upsample`` (``local_upsample``): the layer makes (n - 1) * upsample fine columns at hop' = hop / upsample out of n
    coarse ones, the window starts ``phase`` positions into coarse column 0 -- that is, at fine column c0 = phase // hop',
    phase' = phase % hop' -- and reads nf = ``frames_needed(T, hop', phase', interp)`` fine columns from there:
    ceil((c0 + nf) / upsample) + 1.  ``phase`` None: a phase per clip, sized for the worst case c0 = upsample - 1 and
    phase' = hop' - 1.  ``upsample`` = 1 is ``frames_needed`` itself (no layer, no column more)."""
    T, hop, upsample = int(T), int(hop), int(upsample)
    if upsample < 1 or hop % upsample:
        raise Exception("coarse_frames_needed: upsample must be >= 1 and divide hop = %d, got %d" % (hop, upsample))
    if upsample == 1:
        return frames_needed(T, hop, hop - 1 if phase is None else phase, interp)
    fine = hop // upsample
    c0, ph = (upsample - 1, fine - 1) if phase is None else divmod(int(phase), fine)
    return (c0 + frames_needed(T, fine, ph, interp) + upsample - 1) // upsample + 1


def local_alignment(s0: int, hop: int):
    """THE alignment rule of local conditioning, in one place: network input position t of a clip whose first input sample is
    sample ``s0`` of its file reads feature column (s0 + t) // hop.  Returns (first column, phase) = (s0 // hop, s0 % hop): the
    caller passes the file's columns from the first one on, with ``local_phase=`` the phase.  The decoder follows the same
    rule: the step that consumes the sample at absolute position p reads column p // hop.  Linear interpolation
    (``local_interp="linear"``) keeps the rule: column k is anchored at the FIRST sample of its frame, position k * hop, and a
    position p inside the frame reads column p // hop moved towards column p // hop + 1 by the fraction (p % hop) / hop."""
    if hop <= 0 or s0 < 0:
        raise Exception("local_alignment: hop must be positive and s0 non-negative, got hop = %d, s0 = %d" % (hop, s0))
    return int(s0) // int(hop), int(s0) % int(hop)


class _LocalFn(_Fn):
    """Local conditioning (van den Oord et al. 2016, eq. 4, with y = the features repeated over time -- "use Vf * h and repeat
    these values across time"): features (B, F, n), one column per ``local_hop`` positions -> the block (B, n, sum_l 2 cd_l) of
    per-(clip, frame) gate biases V h, one small projection over the B n rows (``wn_pointwise_*``).  Nothing of size
    B x T x sum 2 cd exists: the layer kernels index the block by (clip, frame of t).  The projection's gradient goes straight
    into the gradient arena; the features receive theirs when they require grad (the hook for a learned feature network)."""

    @staticmethod
    def forward(ctx, feats, V, net):
        B, F, n = feats.shape
        h = feats.permute(0, 2, 1).contiguous().view(B * n, F)
        R = V.shape[0]
        out = torch.empty((B, n, R), device=h.device, dtype=torch.float32)
        check(_lib.lib().wn_pointwise_fwd(ptr(h), ptr(V), None, ptr(out), B * n, F, R, ACT["none"], net._exec(), stream_ptr()),
              "wn_pointwise_fwd")
        ctx.save_for_backward(h)
        ctx.V, ctx.net, ctx.shape = V, net, (B, F, n)
        return out

    @staticmethod
    def backward(ctx, dout):
        (h,) = ctx.saved_tensors
        V = ctx.V
        B, F, n = ctx.shape
        dout = dout.contiguous()
        dh = torch.empty_like(h) if ctx.needs_input_grad[0] else None
        check(_lib.lib().wn_pointwise_bwd(ptr(h), ptr(V), ptr(dout), ptr(dh), ptr(V.grad), None, B * n, F, V.shape[0],
                                          ACT["none"], ctx.net._exec(), stream_ptr()), "wn_pointwise_bwd")
        return (None if dh is None else dh.view(B, n, F).permute(0, 2, 1)), None, None


class _UpsampleFn(_Fn):
    """Learned upsampling ahead of the projection (van den Oord et al. 2016, section 2.5: "a transposed convolutional network
    (learned upsampling)"): features (B, F, n) at hop H -> fine features (B, (n - 1) U, F) at hop H / U, time-major.  A
    transposed convolution of stride U and kernel 2 U over the frame axis, written as ONE channel GEMM (``wn_pointwise_*``,
    the entry point ``_LocalFn`` uses): the input is the (B (n - 1), 2 F) matrix of neighbouring column pairs (h_k ; h_k+1),
    the weight W is (U F, 2 F), and the output (B (n - 1), U F) viewed as (B, (n - 1) U, F) IS the fine sequence -- row
    q F + c of W makes channel c of fine column k U + q.  No bias, no activation.  The weight's gradient goes straight into
    the gradient arena; the coarse features receive theirs when they require grad: the two halves of the pair matrix's
    gradient, added back onto columns k and k + 1."""

    @staticmethod
    def forward(ctx, feats, W, net):
        B, F, n = feats.shape
        U = W.shape[0] // F
        h = feats.permute(0, 2, 1)
        pairs = torch.cat([h[:, :-1], h[:, 1:]], dim=2).contiguous().view(B * (n - 1), 2 * F)
        out = torch.empty((B, (n - 1) * U, F), device=pairs.device, dtype=torch.float32)
        check(_lib.lib().wn_pointwise_fwd(ptr(pairs), ptr(W), None, ptr(out), B * (n - 1), 2 * F, U * F, ACT["none"],
                                          net._exec(), stream_ptr()), "wn_pointwise_fwd")
        ctx.save_for_backward(pairs)
        ctx.W, ctx.net, ctx.shape = W, net, (B, F, n)
        return out

    @staticmethod
    def backward(ctx, dout):
        (pairs,) = ctx.saved_tensors
        W = ctx.W
        B, F, n = ctx.shape
        dout = dout.contiguous()
        dp = torch.empty_like(pairs) if ctx.needs_input_grad[0] else None
        check(_lib.lib().wn_pointwise_bwd(ptr(pairs), ptr(W), ptr(dout), ptr(dp), ptr(W.grad), None, B * (n - 1), 2 * F,
                                          W.shape[0], ACT["none"], ctx.net._exec(), stream_ptr()), "wn_pointwise_bwd")
        if dp is None:
            return None, None, None
        dp = dp.view(B, n - 1, 2 * F)
        dh = torch.zeros((B, n, F), device=dp.device, dtype=torch.float32)
        dh[:, :-1] += dp[:, :, :F]
        dh[:, 1:] += dp[:, :, F:]
        return dh.permute(0, 2, 1), None, None


class _CondFn(_Fn):
    """Global conditioning (van den Oord et al. 2016, eq. 3): class ids (B,) -> the block (B, sum_l 2 cd_l) of per-clip gate
    biases V E[id] -- an embedding gather and one small projection (``wn_pointwise_*``; B x channels x rows, tiny).  The
    projection's gradient goes straight into the gradient arena like every other weight's; the embedding's is formed without
    atomics -- a (classes, B) one-hot mask times the (B, channels) gradient, summed over B in a fixed order -- so it is
    bit-reproducible, and the rows of classes absent from the batch receive exactly 0.  Static shapes: capturable."""

    @staticmethod
    def forward(ctx, ids, E, V, net):
        h = E.view(E.shape[0], E.shape[1]).index_select(0, ids).contiguous()          # (B, channels)
        B, H = h.shape
        R = V.shape[0]
        out = torch.empty((B, R), device=h.device, dtype=torch.float32)
        check(_lib.lib().wn_pointwise_fwd(ptr(h), ptr(V), None, ptr(out), B, H, R, ACT["none"], net._exec(), stream_ptr()),
              "wn_pointwise_fwd")
        ctx.save_for_backward(ids, h)
        ctx.E, ctx.V, ctx.net = E, V, net
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, h = ctx.saved_tensors
        E, V = ctx.E, ctx.V
        B, H = h.shape
        dout = dout.contiguous()
        dh = torch.empty_like(h)
        check(_lib.lib().wn_pointwise_bwd(ptr(h), ptr(V), ptr(dout), ptr(dh), ptr(V.grad), None, B, H, V.shape[0],
                                          ACT["none"], ctx.net._exec(), stream_ptr()), "wn_pointwise_bwd")
        mask = (torch.arange(E.shape[0], device=ids.device).unsqueeze(1) == ids.unsqueeze(0)).to(torch.float32)   # (classes, B)
        E.grad.view(E.shape[0], H).add_((mask.unsqueeze(2) * dh.unsqueeze(0)).sum(dim=1))
        return None, None, None, None


# ----------------------------------------------------------------------------------------------
# bf16-storage nodes (BASELINE config 5; include/wavenet_hip.h "bf16-storage path"): activations are torch.bfloat16
# (B, T, C) tensors, weights and their gradients stay fp32 in the flat arenas
# ----------------------------------------------------------------------------------------------
class _Embed16Fn(_Fn):
    @staticmethod
    def forward(ctx, idx, W, b, fw, net):
        B, T = idx.shape
        Cc, Q = W.shape[0], W.shape[1]
        out = torch.empty((B, T, Cc), device=idx.device, dtype=torch.bfloat16)
        check(_lib.lib().wn16_embed_fwd(ptr(idx), ptr(W), ptr(b), ptr(out), B, T, Q, Cc, fw, stream_ptr()),
              "wn16_embed_fwd")
        ctx.save_for_backward(idx)
        ctx.W, ctx.b, ctx.fw, ctx.net = W, b, fw, net
        return out

    @staticmethod
    def backward(ctx, dout):
        (idx,) = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        B, T = idx.shape
        dout = dout.contiguous()
        lib = _lib.lib()
        if W.shape[0] == 128 and W.shape[1] == 256 and ctx.fw == 2:
            # one-hot contraction on the matrix cores, straight from the bf16 gradient
            nws = lib.wn16_embed_bwd_workspace_bytes(B, T)
            ws = torch.empty((nws,), device=dout.device, dtype=torch.uint8)
            check(lib.wn16_embed_bwd(ptr(idx), ptr(dout), ptr(W.grad), ptr(None if b is None else b.grad), B, T,
                                     W.shape[1], W.shape[0], ctx.fw, ptr(ws), nws, stream_ptr()), "wn16_embed_bwd")
            return None, None, None, None, None
        d32 = torch.empty(dout.shape, device=dout.device, dtype=torch.float32)
        check(lib.wn16_cvt_to_f32(ptr(dout), ptr(d32), dout.numel(), stream_ptr()), "wn16_cvt_to_f32")
        check(lib.wn_embed_bwd(ptr(idx), ptr(d32), ptr(W.grad), ptr(None if b is None else b.grad), B, T,
                               W.shape[1], W.shape[0], ctx.fw, ctx.net._exec(B, T), stream_ptr()), "wn_embed_bwd")
        return None, None, None, None, None


class _Stack16Fn(_Fn):
    """forward_residual_block in bf16 storage: one library call each way (wn16_stack_fwd / wn16_stack_bwd).  The forward
    keeps every layer's output and z only; the backward recomputes tanh / sigmoid.  ``cond`` / ``rows`` as in ``_StackFn``:
    the conditioning block and its ``GateBiasRows``, handed to the library through the descriptor alone (the wn16_* calls
    take no WnExec); the backward returns the block's gradient (``WN16_BWD_ROW_GRADS``)."""

    @staticmethod
    def forward(ctx, x, anchor, net, t_off, train, cond=None, rows=None):
        ctx.set_materialize_grads(False)
        B, T, Cr = x.shape
        x = x.contiguous()
        if rows is None:
            desc = net._stack_desc()
        else:
            rows.check(B, T)
            desc, ckeep = rows.call16(B, T)
        L = len(net._flat_layers)
        dev_ = x.device
        xs = torch.empty((L, B, T, Cr), device=dev_, dtype=torch.bfloat16)
        z = torch.empty((L, B, T, Cr), device=dev_, dtype=torch.bfloat16)
        skip = torch.empty((B, T - t_off, net._Cs), device=dev_, dtype=torch.bfloat16)
        check(_lib.lib().wn16_stack_fwd(desc, ptr(net._pack16), ptr(x), ptr(xs), ptr(z), ptr(skip), B, T, t_off,
                                        1 if net.compat_zero_prefix else 0, stream_ptr()), "wn16_stack_fwd")
        ctx.net, ctx.t_off, ctx.shape = net, t_off, (B, T, Cr)
        ctx.saved = (x, xs, z) if train else None
        ctx.cond = cond if train else None
        ctx.rows = rows
        net._last16 = (x, xs, z, skip)                               # (tests look at the intermediates)
        return xs[L - 1], skip

    @staticmethod
    def backward(ctx, dout, dskip):
        net, t_off = ctx.net, ctx.t_off
        B, T, Cr = ctx.shape
        if ctx.saved is None:
            raise _lib.WaveNetHipError("backward through a forward that ran without grad enabled")
        x, xs, z = ctx.saved
        lib = _lib.lib()
        desc = net._stack_desc()
        gt = net._grad_tables()
        dcond, flags, dwf, dwg = None, 0, gt["wf"], gt["wg"]
        if ctx.cond is not None:
            # the gate-row gradients accumulate (+=) into a zeroed block: the gradient of the conditioning block.  dWf / dWg
            # grow to 2 L entries: the weight gradients, then every layer's gradient row of (clip 0, frame 0)
            dcond = torch.zeros_like(ctx.cond)
            desc, ckeep = ctx.rows.call16(B, T)
            dbf, dbg = ctx.rows.grad_tables(dcond)
            nl = len(net._flat_layers)
            dwf = (C.c_void_p * (2 * nl))(*([gt["wf"][l] for l in range(nl)] + [dbf[l] for l in range(nl)]))
            dwg = (C.c_void_p * (2 * nl))(*([gt["wg"][l] for l in range(nl)] + [dbg[l] for l in range(nl)]))
            flags = _lib.WN16_BWD_ROW_GRADS
        nbytes = lib.wn16_stack_bwd_workspace_bytes(desc, B, T, t_off)
        ws = torch.empty((nbytes,), device=x.device, dtype=torch.uint8)
        dout = None if dout is None else dout.contiguous()
        dskip = None if dskip is None else dskip.contiguous()
        dx = torch.empty((B, T, Cr), device=x.device, dtype=torch.bfloat16) if ctx.needs_input_grad[0] else None
        check(lib.wn16_stack_bwd(desc, ptr(net._pack16), ptr(x), ptr(xs), ptr(z), ptr(dout), ptr(dskip), ptr(dx),
                                 dwf, dwg, gt["wp"], gt["ws"], ptr(ws), nbytes, B, T, t_off,
                                 1 if net.compat_zero_prefix else 0, flags, stream_ptr()), "wn16_stack_bwd")
        net._last16_ws = ws
        ctx.saved = ctx.cond = None
        return dx, None, None, None, None, dcond, None


class _Pointwise16Fn(_Fn):
    """out = W relu(x) + b on bf16 activations; the last head layer writes fp32 logits."""

    @staticmethod
    def forward(ctx, x, W, b, Wb, WbT, act, out_f32, hook):
        lead = x.shape[:-1]
        Cin, Cout = x.shape[-1], W.shape[0]
        x2 = x.reshape(-1, Cin).contiguous()
        out = torch.empty((x2.shape[0], Cout), device=x.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
        check(_lib.lib().wn16_pointwise_fwd(ptr(x2), ptr(Wb), ptr(b), ptr(out), 1 if out_f32 else 0, x2.shape[0], Cin, Cout,
                                            act, stream_ptr()), "wn16_pointwise_fwd")
        ctx.save_for_backward(x2)
        ctx.W, ctx.b, ctx.WbT, ctx.act, ctx.lead = W, b, WbT, act, lead
        return out.view(*lead, Cout)

    @staticmethod
    def backward(ctx, dout):
        (x2,) = ctx.saved_tensors
        W, b = ctx.W, ctx.b
        Cout, Cin = W.shape[0], x2.shape[1]
        N = x2.shape[0]
        lib = _lib.lib()
        d2 = dout.reshape(-1, Cout).contiguous()
        d16 = d32 = scratch = None
        if d2.dtype == torch.float32:
            d32 = d2
            scratch = torch.empty((N, Cout), device=d2.device, dtype=torch.bfloat16)
        else:
            d16 = d2
            if b is not None:                                        # the bias gradient is summed in fp32
                d32 = torch.empty((N, Cout), device=d2.device, dtype=torch.float32)
                check(lib.wn16_cvt_to_f32(ptr(d16), ptr(d32), d16.numel(), stream_ptr()), "wn16_cvt_to_f32")
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        nws = lib.wn16_pointwise_bwd_workspace_bytes(N, Cout)      # per-workgroup partials: gradients without float atomics
        ws = torch.empty((nws,), device=d2.device, dtype=torch.uint8)
        check(lib.wn16_pointwise_bwd(ptr(x2), ptr(ctx.WbT), ptr(d16), ptr(d32), ptr(scratch), ptr(dx), ptr(W.grad),
                                     ptr(None if b is None else b.grad), N, Cin, Cout, ctx.act, ptr(ws), nws, stream_ptr()),
              "wn16_pointwise_bwd")
        return (None if dx is None else dx.view(*ctx.lead, Cin)), None, None, None, None, None, None, None


# ----------------------------------------------------------------------------------------------
# links: objects with the attribute names the reference's scripts touch
# ----------------------------------------------------------------------------------------------
class _Link(object):
    """A parameter holder: ``W`` (reference shape) and ``b`` (or None), views of the flat arena."""

    def __init__(self, name: str, wshape: Tuple[int, ...], bshape: Optional[Tuple[int]]):
        self.name, self.wshape, self.bshape = name, wshape, bshape
        self.W: Optional[torch.Tensor] = None
        self.b: Optional[torch.Tensor] = None


class DilatedConvolution1D(_Link):
    """Drop-in for wavenet.py:263-342 (``__call__`` = whole window, ``_forward`` = newest column)."""

    def __init__(self, net, name, in_channels, out_channels, ksize, filter_width=2, dilation=1, nobias=False):
        shape = (out_channels, in_channels) + tuple(ksize)
        super().__init__(name, shape, None if nobias else (out_channels,))
        self.net = net
        self.in_channels, self.out_channels = in_channels, out_channels
        self.filter_width, self.dilation = filter_width, dilation

    def __call__(self, x):
        x = self.net.to_variable(x)
        _need_gpu(x)
        xb = _to_btc(x)
        Z = self.net._Z(xb.shape[1], self.dilation)
        return _as_view(_ConvFn.apply(xb, self.W, self.b, self.filter_width, self.dilation, Z, self.net._hook))

    def _forward(self, x_batch_data):
        """Newest column only, batch 0 (wavenet.py:281-292); returns (1, Cout, 1, 1)."""
        x = self.net.to_variable(x_batch_data)
        _need_gpu(x)
        need = (self.filter_width - 1) * self.dilation + 1
        if x.shape[3] < need:
            raise IndexError("window of %d columns is shorter than the layer's reach %d" % (x.shape[3], need))
        cols = [x.shape[3] - 1 - (self.filter_width - 1 - k) * self.dilation for k in range(self.filter_width)]
        taps = x[0:1, :, :, cols]                                   # (1, Cin, 1, fw), oldest first
        with torch.no_grad():
            out = _ConvFn.apply(_to_btc(taps), self.W, self.b, self.filter_width, 1, 0, None)
        return _as_view(out[:, -1:, :])


class Convolution1x1(_Link):
    def __init__(self, net, name, in_channels, out_channels, nobias=False):
        super().__init__(name, (out_channels, in_channels, 1, 1), None if nobias else (out_channels,))
        self.net = net
        self.in_channels, self.out_channels = in_channels, out_channels

    def __call__(self, x, act="none"):
        x = self.net.to_variable(x)
        _need_gpu(x)
        return _as_view(_PointwiseFn.apply(_to_btc(x), self.W, self.b, ACT[act], self.net))


class ResidualConvLayer(object):
    """wavenet.py:344-368.  ``__call__`` returns (output, projection_softmax) like the reference."""

    def __init__(self, net):
        self.net = net
        self.wf = self.wg = self.projection_block = self.projection_softmax = None

    @property
    def cd(self):
        return self.wf.out_channels

    @property
    def fw(self):
        return self.wf.filter_width

    @property
    def dilation(self):
        return self.wf.dilation

    def _run(self, xb, save):
        self.net._no_single_layer_condition()
        B, T, Cr = xb.shape
        out = torch.empty_like(xb)
        z = torch.empty((B, T, self.cd), device=xb.device, dtype=torch.float32)
        check(_lib.lib().wn_layer_fwd(ptr(xb), ptr(self.wf.W), ptr(self.wf.b), ptr(self.wg.W), ptr(self.wg.b),
                                      ptr(self.projection_block.W), ptr(self.projection_block.b), ptr(out), ptr(z),
                                      None, None, B, T, Cr, self.cd, self.fw, self.dilation,
                                      self.net._Z(T, self.dilation), self.net._exec(B), stream_ptr()), "wn_layer_fwd")
        return out, z

    def __call__(self, x):
        """Inference-only single-layer call (training goes through forward_residual_block)."""
        x = self.net.to_variable(x)
        _need_gpu(x)
        with torch.no_grad():
            out, z = self._run(_to_btc(x).contiguous(), False)
            skip = _PointwiseFn.apply(z, self.projection_softmax.W, self.projection_softmax.b, ACT["none"], self.net)
        return _as_view(out), _as_view(skip)

    def _forward(self, x):
        """Newest column only (wavenet.py:350-356): (1,Cr,1,1), (1,Cs,1,1)."""
        x = self.net.to_variable(x)
        _need_gpu(x)
        self.net._no_single_layer_condition()
        fw, d = self.fw, self.dilation
        cols = [x.shape[3] - 1 - (fw - 1 - k) * d for k in range(fw)]
        taps = _to_btc(x[0:1, :, :, cols]).contiguous()             # (1, fw, Cr)
        with torch.no_grad():
            B, T, Cr = taps.shape
            out = torch.empty_like(taps)
            z = torch.empty((B, T, self.cd), device=taps.device, dtype=torch.float32)
            check(_lib.lib().wn_layer_fwd(ptr(taps), ptr(self.wf.W), ptr(self.wf.b), ptr(self.wg.W), ptr(self.wg.b),
                                          ptr(self.projection_block.W), ptr(self.projection_block.b), ptr(out),
                                          ptr(z), None, None, B, T, Cr, self.cd, fw, 1, 0, self.net._exec(B),
                                          stream_ptr()), "wn_layer_fwd")
            skip = _PointwiseFn.apply(z[:, -1:, :], self.projection_softmax.W, self.projection_softmax.b,
                                      ACT["none"], self.net)
        return _as_view(out[:, -1:, :]), _as_view(skip)


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
class _StepPlan(object):
    """A step plan handle (include/wavenet_hip.h, "step plan") and the device memory it lays its images out in."""

    def __init__(self, device, nbytes: int):
        self.mem = torch.empty((nbytes,), device=device, dtype=torch.uint8)
        h = C.c_void_p()
        check(_lib.lib().wn_plan_create(C.byref(h), self.mem.data_ptr(), nbytes), "wn_plan_create")
        self.handle = h

    def __del__(self):
        try:
            _lib.lib().wn_plan_destroy(self.handle)
        except Exception:
            pass


EMA_FILE = "wavenet.ema.npz"       # the weight average of enable_ema, next to wavenet.model.npz


class WaveNet(object):
    """Drop-in for wavenet.py:370-639."""

    head_activation = "relu"          # wavenet.py:588

    def __init__(self, params, compat_zero_prefix: bool = True, seed: Optional[int] = None, storage: str = "fp32",
                 condition_classes: int = 0, condition_channels: int = 0, local_channels: int = 0, local_hop: int = 0,
                 local_interp: str = "repeat", local_upsample: int = 1):
        """``storage="bf16"`` (BASELINE config 5; not in the reference): activations in bfloat16, fp32 accumulation, fp32
        master weights; for 128 residual / dilation channels, filter width 2, a multiple of 256 skip channels.

        ``condition_classes`` / ``condition_channels`` (both 0: off, and the model is byte for byte the unconditioned one):
        global conditioning, the open item of the reference's own to-do list.  Every residual layer becomes
        z = tanh(Wf * x + Vf h) sigmoid(Wg * x + Vg h) with h = the learned ``condition_channels``-wide embedding row of the
        clip's integer class id (a speaker).  Two more links, registered AFTER the head so that no existing arena offset or
        seeded draw moves: ``global_condition_embed/W`` (classes, channels, 1, 1) and ``global_condition_projection/W``
        (sum_l 2 cd_l, channels, 1, 1), rows layer-major, a layer's filter rows before its gate rows.  They are not
        ``Params`` fields (``Params().to_dict()`` is the reference's key set).  The forward methods then take
        ``condition=`` -- one class id per clip.

        ``local_channels`` = F / ``local_hop`` = H (both 0: off, and the model is byte for byte what it was; both > 0
        together): local conditioning, the last open item of that list and what makes the network a vocoder.  A sequence of
        features h -- a log-mel spectrogram, say, one F-wide column every H samples -- steers every layer sample by sample:
        z = tanh(Wf * x + Vf y) sigmoid(Wg * x + Vg y) (eq. 4) with y = h repeated over time.  One more link, registered behind
        the global conditioning links so that no existing arena offset or seeded draw moves:
        ``local_condition_projection/W`` (sum_l 2 cd_l, F, 1, 1), rows laid out like the global projection's.  The forward
        methods then take ``local=`` -- float32 features (B, F, n), n >= ceil((T + phase) / H), surplus columns ignored -- and
        ``local_phase=`` (an int, default 0).  Alignment (``local_alignment``): network input position t of a clip whose first
        input sample is sample s0 of its file reads feature column (s0 + t) // H; the caller passes the columns from s0 // H
        on, with phase s0 % H.  With global conditioning also on, the clip's row is added to every frame row of its clip.

        ``local_interp`` ("repeat", the default and the above; or "linear"): how the features reach the sample rate.  "linear"
        interpolates between neighbouring columns instead of repeating one -- the parameter-free form of the paper's learned
        upsampling.  Column k is anchored at the first sample of its frame, position k H (a decision: the alignment rule and
        the decoder's "position p reads column p // H" stay what they are); position p reads
        r[j] + alpha (r[j + 1] - r[j]) with j = p // H and alpha = float32(p % H) / float32(H), r the projected rows (V is
        linear, so interpolating the features is interpolating the rows; nothing of size B x T x sum 2 cd exists).  Every
        window then needs ONE MORE column, ``frames_needed(T, H, phase, "linear")``: the library never clamps, the caller
        supplies the column after the last (the command-line drivers repeat the file's last one).

        A phase per clip: ``local_phase=`` of ``forward_one_step``, ``forward_residual_block``, ``token_nll``,
        ``graph.default_loss`` and ``TrainStepGraph`` also takes a 1-D sequence, numpy array or integer tensor with one entry
        per clip, each in [0, H) (anything else raises before any device work and names the first offending clip).  The
        phases then live in device memory (``WnStackDesc.bias_phase_tab``) and are read when the kernels run, so one batch --
        and one captured step -- holds clips that start at any sample.  Every clip then needs
        ``frames_needed(T, H, H - 1, interp)`` columns, whatever its phase.

        ``local_upsample`` = U (1, the default: none, and the model is byte for byte what it was; U > 1 must divide H): a
        LEARNED upsampling layer ahead of the projection (section 2.5 of the paper).  It takes the features from hop H to hop
        H' = H / U; the projection, the layer kernels and the decoders then run at hop H' in the model's ``local_interp``
        mode.  One more link, last of all in the arena: ``local_condition_upsample/W`` (U F, 2 F, 1, 1).  For coarse columns
        h_k, rows q F .. (q + 1) F of W make fine column m = k U + q, q in [0, U):
        y[:, k U + q] = W[qF:(q+1)F, :F] h_k + W[qF:(q+1)F, F:] h_k+1 -- a transposed convolution of stride U and kernel 2 U over
        the frame axis, one channel GEMM over the (B (n - 1), 2 F) matrix of neighbouring column pairs (``_UpsampleFn``), no
        bias, no activation.  n coarse columns make (n - 1) U fine ones; fine column m is anchored at position m H'.  The
        weight starts, without a draw from the RNG, at linear interpolation between the coarse columns
        (W[qF + c, c] = 1 - float32(q) / float32(U), W[qF + c, F + c] = float32(q) / float32(U), 0 elsewhere), so every other
        tensor equals the same-seed U = 1 model's and a "linear" model starts, in exact arithmetic, as the U = 1 linear
        model at hop H.  The caller's contract does not change: coarse columns from s0 // H on and ``local_phase`` = s0 % H
        in [0, H), an int or one per clip.  The fine sequence is cut at fine column phase // H' (per clip: gathered on the
        device) and the stack runs at phase % H'.  A window needs ``coarse_frames_needed(T, H, U, phase, interp)`` columns
        (a phase per clip: ``phase=None``, the worst case); surplus ones are ignored.  ``upsampled_features`` returns the
        layer's output; ``local_biases`` then holds one row per FINE column."""
        params.check()
        if storage not in ("fp32", "bf16"):
            raise Exception("storage must be 'fp32' or 'bf16'")
        self.local_upsample = int(local_upsample)
        if self.local_upsample < 1:
            raise Exception("local_upsample must be >= 1 (1: no learned upsampling), got %d" % self.local_upsample)
        if self.local_upsample > 1 and not (int(local_channels) > 0 and int(local_hop) > 0):
            raise Exception("local_upsample = %d needs local conditioning (local_channels / local_hop)" % self.local_upsample)
        if self.local_upsample > 1 and int(local_hop) % self.local_upsample:
            raise Exception("local_upsample = %d does not divide local_hop = %d (the fine hop is local_hop / local_upsample)"
                            % (self.local_upsample, int(local_hop)))
        self.condition_classes, self.condition_channels = int(condition_classes), int(condition_channels)
        if (self.condition_classes > 0) != (self.condition_channels > 0) or self.condition_classes < 0 or self.condition_channels < 0:
            raise Exception("global conditioning needs condition_classes > 0 and condition_channels > 0 (or both 0: off), got "
                            "%d and %d" % (self.condition_classes, self.condition_channels))
        if self.condition_classes and storage == "bf16":
            raise Exception("global conditioning is not available with storage='bf16' (the bf16-storage kernels take no gate biases) "
                            "in the constructor: build the conditioned model at storage='fp32' and switch it with "
                            "set_storage('bf16')")
        if self.condition_classes and not params.residual_conv_dilation_no_bias:
            raise Exception("global conditioning needs residual_conv_dilation_no_bias = True (the conditioning term is the gate "
                            "convolutions' bias; a second, shared one is not supported)")
        self.local_channels, self.local_hop = int(local_channels), int(local_hop)
        if (self.local_channels > 0) != (self.local_hop > 0) or self.local_channels < 0 or self.local_hop < 0:
            raise Exception("local conditioning needs local_channels > 0 and local_hop > 0 (or both 0: off), got %d and %d"
                            % (self.local_channels, self.local_hop))
        if self.local_channels and storage == "bf16":
            raise Exception("local conditioning is not available with storage='bf16' (the bf16-storage kernels take no gate biases) "
                            "in the constructor: build the conditioned model at storage='fp32' and switch it with "
                            "set_storage('bf16')")
        if self.local_channels and not params.residual_conv_dilation_no_bias:
            raise Exception("local conditioning needs residual_conv_dilation_no_bias = True (the conditioning term is the gate "
                            "convolutions' bias; a second, shared one is not supported)")
        if local_interp not in LOCAL_INTERP:
            raise Exception("local_interp must be 'repeat' or 'linear', got %r" % (local_interp,))
        if local_interp != "repeat" and not self.local_channels:
            raise Exception("local_interp = %r needs local conditioning (local_channels / local_hop)" % (local_interp,))
        self.local_interp = local_interp
        self.params = params
        self.storage = storage
        self.gemm_precision = None          # None: the module default (wavenet_amd.set_gemm_precision) at call time
        self.exec_flags = None              # None: _lib.default_exec_flags(); else WN_EXEC_* bits for every call of this model
        self.fuse_head_loss = os.environ.get("WAVENET_HIP_NO_FUSED_HEAD_LOSS") != "1"      # head_cross_entropy: one launch when covered
        self.fwd_t1_min_blocks = None       # None: _lib.default_fwd_t1_min_blocks() (WnExec.fwd_t1_min_blocks)
        self._scratch, self._scratch_keep = {}, []
        self._plan, self._plan_obj, self._plan_on = None, None, False     # step plan (wn_plan_*): see plan_begin
        self.use_step_plan = os.environ.get("WAVENET_HIP_NO_STEP_PLAN") != "1"   # TrainStepGraph: weight preparation in two launches
        self._unit_upstream = False         # True while a caller guarantees d loss = 1 (TrainStepGraph)
        self._pack16 = None
        self._w16_stale = True
        self.compat_zero_prefix = compat_zero_prefix
        self._gpu = False
        self._hook = None
        self._anchor = torch.zeros((1,), requires_grad=True)
        self._dp_group = None
        self._last_layer_inputs = None
        self._ema_arena, self._ema_t, self._ema_decay, self._ema_warmup = None, 0, 0.0, True     # enable_ema
        self._ema_swapped = False           # True inside ema_weights()
        self.create_network()
        self._allocate(seed)
        self.setup_optimizer()

    # -- topology (wavenet.py:379-455) --------------------------------------------------------
    def create_network(self):
        p = self.params
        self.causal_conv_layers: List[DilatedConvolution1D] = []
        fw = p.causal_conv_filter_width
        chans = [p.quantization_steps] + list(p.causal_conv_channels)
        for i in range(len(chans) - 1):
            self.causal_conv_layers.append(DilatedConvolution1D(
                self, "causal_%d" % i, chans[i], chans[i + 1], (1, fw), filter_width=fw, dilation=1,
                nobias=p.causal_conv_no_bias))
        self.residual_blocks: List[List[ResidualConvLayer]] = []
        fw = p.residual_conv_filter_width
        n_in = p.causal_conv_channels[-1]
        n_skip = p.softmax_conv_channels[0]
        for blk in range(p.residual_num_blocks):
            layers = []
            for li, n_out in enumerate(p.residual_conv_channels):
                ksize = (1, fw) if li == 0 else (fw, 1)              # wavenet.py:418-424
                lay = ResidualConvLayer(self)
                pre = "residual_%d_block_%d_" % (blk, li)
                lay.wf = DilatedConvolution1D(self, pre + "wf", n_in, n_out, ksize, filter_width=fw,
                                              dilation=fw ** li, nobias=p.residual_conv_dilation_no_bias)
                lay.wg = DilatedConvolution1D(self, pre + "wg", n_in, n_out, ksize, filter_width=fw,
                                              dilation=fw ** li, nobias=p.residual_conv_dilation_no_bias)
                lay.projection_block = Convolution1x1(self, pre + "projection_block", n_out, n_in,
                                                      nobias=p.residual_conv_projection_no_bias)
                lay.projection_softmax = Convolution1x1(self, pre + "projection_softmax", n_out, n_skip,
                                                        nobias=p.residual_conv_projection_no_bias)
                layers.append(lay)
            self.residual_blocks.append(layers)
        self.softmax_conv_layers: List[Convolution1x1] = []
        sc = p.softmax_conv_channels
        for i in range(len(sc) - 1):
            self.softmax_conv_layers.append(Convolution1x1(self, "softmax_%d" % i, sc[i], sc[i + 1],
                                                           nobias=p.softmax_conv_no_bias))
        self._flat_layers = [lay for blk in self.residual_blocks for lay in blk]
        self._Cr, self._Cs = n_in, n_skip
        # global conditioning: layer l's filter biases are rows off .. off + cd_l of the projection, its gate biases the next cd_l
        self.global_condition_embed = self.global_condition_projection = None
        self._cond_offsets, self._cond_rows = [], 0
        if self.condition_classes or self.local_channels:
            for lay in self._flat_layers:
                self._cond_offsets.append((self._cond_rows, self._cond_rows + lay.cd))
                self._cond_rows += 2 * lay.cd
        self.local_condition_projection = None
        if self.local_channels:
            self.local_condition_projection = _Link("local_condition_projection", (self._cond_rows, self.local_channels, 1, 1), None)
        self.local_condition_upsample = None
        if self.local_upsample > 1:
            self.local_condition_upsample = _Link("local_condition_upsample", (self.local_upsample * self.local_channels,
                                                                               2 * self.local_channels, 1, 1), None)
        if self.condition_classes:
            self.global_condition_embed = _Link("global_condition_embed",
                                                (self.condition_classes, self.condition_channels, 1, 1), None)
            self.global_condition_projection = _Link("global_condition_projection",
                                                     (self._cond_rows, self.condition_channels, 1, 1), None)

    def links(self) -> List[_Link]:
        """All parameter holders in the reference's registration order (wavenet.py:461-472)."""
        out: List[_Link] = list(self.causal_conv_layers)
        for lay in self._flat_layers:
            out += [lay.wf, lay.wg, lay.projection_block, lay.projection_softmax]
        out += list(self.softmax_conv_layers)
        if self.condition_classes:                                   # after the head: existing offsets and draws stay put
            out += [self.global_condition_embed, self.global_condition_projection]
        if self.local_channels:                                      # last of all, with or without global conditioning
            out.append(self.local_condition_projection)
        if self.local_upsample > 1:                                  # ... and the learned upsampling layer behind it
            out.append(self.local_condition_upsample)
        return out

    @property
    def local_fine_hop(self) -> int:
        """The hop the projection, the layer kernels and the decoders run at: local_hop / local_upsample."""
        return self.local_hop // self.local_upsample

    def _upsample_init(self) -> np.ndarray:
        """The learned upsampling layer's starting weight (U F, 2 F): linear interpolation between the coarse columns."""
        U, F = self.local_upsample, self.local_channels
        w = np.zeros((U * F, 2 * F), dtype=np.float32)
        c = np.arange(F)
        for q in range(U):
            a = np.float32(q) / np.float32(U)
            w[q * F + c, c] = np.float32(1) - a
            w[q * F + c, F + c] = a
        return w

    # -- parameters: one flat arena (what the DP all-reduce and the optimiser kernel see) -----
    def _allocate(self, seed):
        rs = np.random.RandomState(seed) if seed is not None else np.random
        spans = []
        off = 0
        for ln in self.links():
            n = int(np.prod(ln.wshape))
            spans.append((ln, "W", off, n, ln.wshape))
            off += (n + 63) // 64 * 64                               # keep every tensor 256-byte aligned
            if ln.bshape is not None:
                spans.append((ln, "b", off, ln.bshape[0], ln.bshape))
                off += (ln.bshape[0] + 63) // 64 * 64
        self._spans = spans
        host = np.zeros((off,), dtype=np.float32)
        for ln, kind, o, n, shape in spans:
            if ln is self.local_condition_upsample:                # no draw: every other tensor is the U = 1 model's
                host[o:o + n] = self._upsample_init().reshape(-1)
            elif kind == "W":                                       # LeCunNormal like Chainer's default
                fan_in = shape[1] * shape[2] * shape[3]
                host[o:o + n] = (rs.standard_normal(n) / math.sqrt(fan_in)).astype(np.float32)
        self._arena = torch.from_numpy(host)
        self._grad_arena = torch.zeros_like(self._arena)
        self._bind()

    def _bind(self):
        self._any_requires_grad = True
        for ln, kind, o, n, shape in self._spans:
            t = self._arena[o:o + n].view(shape)
            t.requires_grad_(True)
            t.grad = self._grad_arena[o:o + n].view(shape)
            setattr(ln, kind, t)

    @property
    def receptive_field(self) -> int:
        """train_audio/train.py:36-38."""
        p = self.params
        return (p.residual_conv_filter_width ** len(p.residual_conv_channels) - 1) * p.residual_num_blocks + 1

    @property
    def input_width(self) -> int:
        """Receptive field plus one column per causal layer (train_audio/train.py:42-44)."""
        return self.receptive_field + len(self.params.causal_conv_channels)

    @property
    def num_parameters(self) -> int:
        return sum(n for _, _, _, n, _ in self._spans)

    def state_dict(self) -> Dict[str, np.ndarray]:
        """Reference checkpoint keys (``<link>/W``, ``<link>/b``) and shapes."""
        return {"%s/%s" % (ln.name, kind): self._arena[o:o + n].view(shape).detach().cpu().numpy().copy()
                for ln, kind, o, n, shape in self._spans}

    def _check_condition_keys(self, sd):
        """A conditioned checkpoint does not fit an unconditioned model, nor the reverse: say so instead of a KeyError."""
        cond_keys = sorted(k for k in sd if k.startswith("global_condition_"))
        if cond_keys and not self.condition_classes:
            raise Exception("this checkpoint is globally conditioned (%s) and the model is not: construct the model with "
                            "condition_classes / condition_channels" % ", ".join(cond_keys))
        if self.condition_classes and not cond_keys:
            raise Exception("this model is globally conditioned and the checkpoint is not (it holds no "
                            "global_condition_embed/W and global_condition_projection/W)")
        has_local = any(k.startswith("local_condition_") for k in sd)
        if has_local and not self.local_channels:
            raise Exception("this checkpoint is locally conditioned (local_condition_projection/W) and the model is not: "
                            "construct the model with local_channels / local_hop")
        if self.local_channels and not has_local:
            raise Exception("this model is locally conditioned and the checkpoint is not (it holds no "
                            "local_condition_projection/W)")
        up = sd.get("local_condition_upsample/W")
        have = 1 if up is None else (2 * int(np.shape(up)[0])) // max(int(np.shape(up)[1]), 1)
        if have != self.local_upsample:
            raise Exception("this checkpoint was trained with local_upsample = %d%s and the model is built with local_upsample "
                            "= %d%s: construct the model with the checkpoint's value"
                            % (have, "" if have > 1 else " (it holds no local_condition_upsample/W)", self.local_upsample,
                               "" if self.local_upsample > 1 else " (no learned upsampling)"))

    def load_state_dict(self, sd: Dict[str, np.ndarray]):
        self._check_condition_keys(sd)
        with torch.no_grad():
            for ln, kind, o, n, shape in self._spans:
                key = "%s/%s" % (ln.name, kind)
                if key not in sd:
                    raise KeyError(key)
                a = np.asarray(sd[key], dtype=np.float32)
                if a.shape != tuple(shape):
                    raise Exception("shape of %s is %s, expected %s" % (key, a.shape, tuple(shape)))
                self._arena[o:o + n].copy_(torch.from_numpy(a.reshape(-1)))
        self._weights_changed()

    def _weights_changed(self):
        self._w16_stale = True

    def _exec(self, B: int = 8, T: int = 0, call_flags: int = 0, bias_stride: int = 0):
        """WnExec for a library call on the current stream: this model's GEMM precision (``self.gemm_precision``, or the
        module default), its flags, and a scratch buffer owned by (model, stream), sized by ``wn_exec_workspace_bytes``
        for the largest (B, T) seen so far.  Buffers are never freed or moved once handed out -- a captured graph keeps
        the pointer -- a larger batch or a longer window gets a new, larger one.  ``call_flags``: WN_EXEC_* bits of this one
        call, on top of the model's."""
        lib = _lib.lib()
        key = (stream_ptr() or 0, self._arena.device.index)
        ent = self._scratch.get(key)
        if ent is None or ent[1] < B or ent[2] < T:
            p = self.params
            hc = int_array(p.softmax_conv_channels)
            B, T = max(B, 8, ent[1] if ent else 0), max(T, ent[2] if ent else 0)
            nbytes = lib.wn_exec_workspace_bytes(self._stack_desc(), p.quantization_steps, p.causal_conv_channels[0],
                                                 p.causal_conv_filter_width, hc, len(p.softmax_conv_channels), B, T)
            buf = torch.empty((nbytes,), device=self._arena.device, dtype=torch.uint8)
            self._scratch_keep.append(buf)
            ent = (buf, B, T)
            self._scratch[key] = ent
        ex = _lib.WnExec()
        ex.flags = (_lib.default_exec_flags() if self.exec_flags is None else int(self.exec_flags)) | int(call_flags)
        prec = self.gemm_precision or _lib.get_gemm_precision()
        ex.precision = _lib.GEMM_PRECISIONS.index("fp32" if ex.flags & _lib.WN_EXEC_FORCE_GENERIC else prec)
        ex.ws, ex.ws_bytes = ent[0].data_ptr(), ent[0].numel()
        ex.fwd_t1_min_blocks = (_lib.default_fwd_t1_min_blocks() if self.fwd_t1_min_blocks is None
                                else int(self.fwd_t1_min_blocks))
        ex.plan = self._plan if self._plan_on else None
        ex.reserved = int(bias_stride)          # WN_EXEC_BIAS_PER_CLIP: floats between consecutive clips' bias rows
        return C.byref(ex)

    # -- step plan (include/wavenet_hip.h, "step plan"): the weight-only preparation of a training step in two launches --------
    def plan_begin(self, nbytes: int = 16 << 20):
        """A NEW plan (its own device memory: a captured graph keeps pointers into it) in the RECORDING state: the next training
        step runs as ever and registers its weight-only preparation work.  Returns the plan object; the model's entry points carry
        it until :meth:`plan_off`."""
        self._plan_obj = _StepPlan(self._arena.device, nbytes)
        self._plan = self._plan_obj.handle
        check(_lib.lib().wn_plan_record(self._plan), "wn_plan_record")
        self._plan_on = True
        return self._plan_obj

    def plan_use(self, plan_obj):
        """Carry an existing plan again (the caller vouches that wn_plan_prepare opens every step that does)."""
        self._plan_obj, self._plan, self._plan_on = plan_obj, plan_obj.handle, True

    def plan_finish(self):
        check(_lib.lib().wn_plan_finish(self._plan, stream_ptr()), "wn_plan_finish")

    def plan_prepare(self, zero_grads: bool = True):
        """First call of a step that carries the READY plan: every weight image of the step, and (``zero_grads``) cleargrads."""
        n = self._grad_arena.numel() if zero_grads else 0
        n4 = n // 4 * 4
        check(_lib.lib().wn_plan_prepare(self._plan, ptr(self._grad_arena) if n4 else None, n4, stream_ptr()), "wn_plan_prepare")
        if n4 < n:
            self._grad_arena[n4:].zero_()

    def plan_off(self):
        """Entry points stop carrying the plan (its images go stale with the next weight update a prepare does not follow)."""
        self._plan_on = False

    def plan_stats(self):
        out = (C.c_int64 * 8)()
        check(_lib.lib().wn_plan_stats(self._plan, out), "wn_plan_stats")
        return dict(zip(("state", "weight_images", "layer_images", "plan_words", "device_bytes", "prepare_calls", "served", "not_served"),
                        [int(v) for v in out]))

    def set_storage(self, storage: str):
        """The activation storage of every later call: "fp32", or "bf16" (BASELINE config 5's kernels: bfloat16 activations,
        fp32 accumulation).  A property of how the model RUNS, like ``set_gemm_precision``: weights, gradients, optimiser
        state and checkpoints are fp32 either way, so it may be switched at any time, in both directions, and it is the way a
        conditioned model (global, local, both) gets onto the bf16 kernels -- the constructor builds those at fp32 storage.  A
        shape the bf16 kernels do not take fails at the first call, with the library's text.  The bf16 operand images are
        repacked at the next call; a ``TrainStepGraph`` captured before the switch refuses to step."""
        if storage not in ("fp32", "bf16"):
            raise Exception("storage must be 'fp32' or 'bf16'")
        self.storage = storage
        self._w16_stale = True

    def _pack16_if_stale(self):
        """bf16 operand images of the current weights (one pack per optimiser step; captured with the step in a graph)."""
        if not self._w16_stale:
            return
        lib = _lib.lib()
        desc = self._stack_desc()
        if self._pack16 is None or self._pack16.device != self._arena.device:
            if not lib.wn16_supported(desc):
                lib.wn16_pack_stack(desc, None, None)                  # sets the error text
                raise _lib.WaveNetHipError("storage='bf16': %s" % lib.wn_last_error().decode())
            self._pack16 = torch.empty((lib.wn16_pack_elems(desc),), device=self._arena.device, dtype=torch.bfloat16)
            self._head16 = [(torch.empty(l.W.shape[:2], device=self._arena.device, dtype=torch.bfloat16),
                             torch.empty((l.W.shape[1], l.W.shape[0]), device=self._arena.device, dtype=torch.bfloat16))
                            for l in self.softmax_conv_layers]
        check(lib.wn16_pack_stack(desc, ptr(self._pack16), stream_ptr()), "wn16_pack_stack")
        for l, (wb, wbt) in zip(self.softmax_conv_layers, self._head16):
            check(lib.wn16_pack_pointwise(ptr(l.W), ptr(wb), ptr(wbt), l.W.shape[0], l.W.shape[1], stream_ptr()),
                  "wn16_pack_pointwise")
        self._w16_stale = False

    def _stack_desc(self):
        """WnStackDesc over the current arena (rebuilt when the arena moves, e.g. to_gpu)."""
        key = self._arena.data_ptr()
        if getattr(self, "_desc_key", None) != key:
            L = self._flat_layers
            keep = dict(
                cd=int_array([l.cd for l in L]), dil=int_array([l.dilation for l in L]),
                Wf=ptr_array([l.wf.W for l in L]), bf=ptr_array([l.wf.b for l in L]),
                Wg=ptr_array([l.wg.W for l in L]), bg=ptr_array([l.wg.b for l in L]),
                Wp=ptr_array([l.projection_block.W for l in L]), bp=ptr_array([l.projection_block.b for l in L]),
                Ws=ptr_array([l.projection_softmax.W for l in L]), bs=ptr_array([l.projection_softmax.b for l in L]))
            d = _lib.WnStackDesc()
            d.n_layers, d.Cr, d.Cs, d.fw = len(L), self._Cr, self._Cs, self.params.residual_conv_filter_width
            d.cd, d.dilation = keep["cd"], keep["dil"]
            for k in ("Wf", "bf", "Wg", "bg", "Wp", "bp", "Ws", "bs"):
                setattr(d, k, C.cast(keep[k], C.POINTER(C.c_void_p)))
            g = lambda t: None if t is None else t.grad
            gt = dict(
                wf=ptr_array([l.wf.W.grad for l in L]), bf=ptr_array([g(l.wf.b) for l in L]),
                wg=ptr_array([l.wg.W.grad for l in L]), bg=ptr_array([g(l.wg.b) for l in L]),
                wp=ptr_array([l.projection_block.W.grad for l in L]), bp=ptr_array([g(l.projection_block.b) for l in L]),
                ws=ptr_array([l.projection_softmax.W.grad for l in L]),
                bs=ptr_array([g(l.projection_softmax.b) for l in L]))
            self._desc_key, self._sdesc, self._desc_keep, self._gt = key, d, keep, gt
        return C.byref(self._sdesc)

    def _grad_tables(self):
        self._stack_desc()
        return self._gt

    # -- global conditioning --------------------------------------------------------------------------------------------------
    def _condition_ids(self, condition, B):
        """``condition=`` of the forward methods -> (B,) int64 class ids on the device, or None for an unconditioned model.
        A conditioned model called without ids raises, and so does an unconditioned one called with them."""
        if not self.condition_classes:
            if condition is not None:
                raise Exception("condition= was given, but this model has no global conditioning (condition_classes = 0)")
            return None
        if condition is None:
            raise Exception("this model is globally conditioned (%d classes): pass condition= (one class id per clip)"
                            % self.condition_classes)
        if isinstance(condition, torch.Tensor):
            ids = condition
        else:
            a = np.asarray(condition).reshape(-1)
            if a.dtype.kind not in "iu":
                raise Exception("condition= takes integer class ids, got %s" % a.dtype)
            if a.size and (int(a.min()) < 0 or int(a.max()) >= self.condition_classes):
                raise Exception("condition= class ids must lie in [0, %d)" % self.condition_classes)
            ids = torch.from_numpy(a.astype(np.int64))
        ids = self.to_variable(ids).reshape(-1).to(torch.int64)
        if ids.shape[0] != B:
            raise Exception("condition= holds %d class ids for %d clips" % (ids.shape[0], B))
        return ids

    def _condition_block(self, condition, B):
        """The (B, sum 2 cd) block of per-clip gate biases (an autograd node over the two conditioning links), or None."""
        ids = self._condition_ids(condition, B)
        if ids is None:
            return None
        _need_gpu(ids)
        return _CondFn.apply(ids, self.global_condition_embed.W, self.global_condition_projection.W, self)

    def _no_single_layer_condition(self):
        if self.condition_classes:
            raise Exception("a globally conditioned model runs its layers through forward_residual_block(condition=...) only")
        if self.local_channels:
            raise Exception("a locally conditioned model runs its layers through forward_residual_block(local=...) only")

    # -- local conditioning ---------------------------------------------------------------------------------------------------
    def _local_features(self, local, B, T, phase=0):
        """``local=`` / ``local_phase=`` of the forward methods -> ((B, F, n) float32 features on the device, phase), or
        (None, 0) for a model without local conditioning.  ``phase``: an int, or one phase per clip (a 1-D sequence, numpy
        array or integer tensor; returned as a ``LocalPhases``).  A locally conditioned model called without features raises, and so
        does any other model called with them; so do too few columns (surplus ones are ignored)."""
        if not self.local_channels:
            if local is not None:
                raise Exception("local= was given, but this model has no local conditioning (local_channels = 0)")
            if not _one_phase(phase) or phase:
                raise Exception("local_phase= was given, but this model has no local conditioning (local_channels = 0)")
            return None, 0
        if local is None:
            raise Exception("this model is locally conditioned (%d channels, hop %d): pass local= (features of shape "
                            "(clips, %d, frames))" % (self.local_channels, self.local_hop, self.local_channels))
        # an int: one phase for the call.  A sequence / array / integer tensor: a phase per clip, checked here on the host
        # (before any device work); the call then needs the columns of the worst phase, local_hop - 1, whatever the phases
        # are, so that a captured step stays valid for any later ones.
        tab = None
        if isinstance(phase, LocalPhases):
            if len(phase) != B or phase.hop != self.local_hop:
                raise Exception("local_phase= holds %d phases checked against hop %d for %d clips at hop %d"
                                % (len(phase), phase.hop, B, self.local_hop))
            tab = phase
        elif _one_phase(phase):
            phase = int(phase)
            if not 0 <= phase < self.local_hop:
                raise Exception("local_phase= must lie in [0, local_hop = %d), got %d" % (self.local_hop, phase))
        else:
            tab = check_local_phases(phase, B, self.local_hop)
        f = local if isinstance(local, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(local, dtype=np.float32)))
        f = self.to_variable(f)
        if f.dim() != 3 or f.shape[0] != B or f.shape[1] != self.local_channels or f.dtype != torch.float32:
            raise Exception("local= must be float32 of shape (%d, %d, frames), got %s %s"
                            % (B, self.local_channels, f.dtype, tuple(f.shape)))
        worst = phase if tab is None else self.local_hop - 1
        if self.local_upsample > 1:
            U, fine = self.local_upsample, self.local_fine_hop
            need = coarse_frames_needed(T, self.local_hop, U, None if tab is not None else phase, self.local_interp)
            if f.shape[2] < need:
                c0, ph = (U - 1, fine - 1) if tab is not None else divmod(phase, fine)
                raise Exception("local= holds %d feature columns at hop %d, but %d positions at phase %d read %d fine columns at "
                                "hop %d from fine column %d on (local_upsample = %d), which takes %d%s"
                                % (f.shape[2], self.local_hop, T, worst, frames_needed(T, fine, ph, self.local_interp), fine, c0,
                                   U, need, "" if tab is None else " (a phase per clip is sized for the worst phase)"))
        need = frames_needed(T, self.local_hop, worst, self.local_interp)
        if self.local_upsample == 1 and f.shape[2] < need:
            raise Exception("local= holds %d feature columns, but %d positions at hop %d and phase %d read %d%s%s"
                            % (f.shape[2], T, self.local_hop, worst, need,
                               " (linear interpolation reads the column after the last position's own)"
                               if self.local_interp == "linear" else "",
                               "" if tab is None else " (a phase per clip is sized for the worst phase, local_hop - 1)"))
        if tab is not None and not isinstance(tab, LocalPhases):
            tab = LocalPhases(torch.from_numpy(tab).to(f.device), self.local_hop)
        return f, (phase if tab is None else tab)

    def _local_block(self, feats, glob=None):
        """The (B, n, sum 2 cd) block of per-(clip, frame) gate biases (an autograd node over the projection); with global
        conditioning also on, the clip's row ``glob`` (B, sum 2 cd) is added to every frame row of its clip -- a torch op on a
        small tensor, whose backward sums the block's gradient over frames."""
        _need_gpu(feats)
        blk = _LocalFn.apply(feats, self.local_condition_projection.W, self)
        return blk if glob is None else blk + glob.unsqueeze(1)

    def _upsample(self, feats):
        """(B, F, n) coarse features on the device -> the learned layer's (B, (n - 1) U, F) fine sequence, time-major."""
        _need_gpu(feats)
        return _UpsampleFn.apply(feats, self.local_condition_upsample.W, self)

    def upsampled_features(self, features):
        """The fine features of a batch, on the device: (B, F, n) float32 features at hop ``local_hop`` -> (B, F, (n - 1) U) at
        hop ``local_hop / local_upsample``, fine column m anchored at position m H' of coarse column 0's frame -- a view of the
        learned layer's time-major output, what the projection then reads (cut at fine column phase // H').  An autograd node
        when grad is enabled.  With ``local_upsample`` = 1 there is no layer: the features come back as they are."""
        if not self.local_channels:
            raise Exception("upsampled_features: this model has no local conditioning (local_channels = 0)")
        f = features if isinstance(features, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(features, dtype=np.float32)))
        f = self.to_variable(f)
        if f.dim() != 3 or f.shape[1] != self.local_channels or f.dtype != torch.float32:
            raise Exception("upsampled_features: features must be float32 of shape (clips, %d, frames), got %s %s"
                            % (self.local_channels, f.dtype, tuple(f.shape)))
        if self.local_upsample == 1:
            _need_gpu(f)
            return f
        if f.shape[2] < 2:
            raise Exception("upsampled_features: the layer reads pairs of neighbouring columns, got %d column" % f.shape[2])
        return self._upsample(f).permute(0, 2, 1)

    def _stack_features(self, feats, phase, T):
        """What the projection and the stack take, from what ``_local_features`` checked: (features (B, F, n'), hop, phase).
        Without a learned layer: the arguments and ``local_hop``.  With one (``local_upsample`` = U, H' = H / U): the first
        ``coarse_frames_needed`` columns go through the layer, and the fine sequence is cut where the window starts -- an int
        phase: at fine column phase // H', the stack running at phase % H'; a phase per clip: clip b's
        ``frames_needed(T, H', H' - 1)`` columns are gathered from fine column tab[b] // H' on (torch ops on the device
        buffer: capturable) and the stack gets the derived ``LocalPhases(tab % H', H')``."""
        if self.local_upsample == 1:
            return feats, self.local_hop, phase
        U, fine = self.local_upsample, self.local_fine_hop
        per_clip = isinstance(phase, LocalPhases)
        need = coarse_frames_needed(T, self.local_hop, U, None if per_clip else phase, self.local_interp)
        y = self._upsample(feats[:, :, :need])                                   # (B, (need - 1) U, F)
        if not per_clip:
            c0, ph = divmod(int(phase), fine)
            nf = frames_needed(T, fine, ph, self.local_interp)
            return y[:, c0:c0 + nf].permute(0, 2, 1), fine, ph
        nf = frames_needed(T, fine, fine - 1, self.local_interp)
        c0 = torch.div(phase.tab, fine, rounding_mode="floor").to(torch.int64)
        idx = c0.unsqueeze(1) + torch.arange(nf, device=y.device, dtype=torch.int64).unsqueeze(0)        # (B, nf)
        y = torch.gather(y, 1, idx.unsqueeze(2).expand(-1, -1, y.shape[2]))
        return y.permute(0, 2, 1), fine, LocalPhases(torch.remainder(phase.tab, fine).to(torch.int32).contiguous(), fine)

    def local_biases(self, features, phase: int = 0):
        """(n, sum 2 cd) float32 on the device: the table of one utterance -- row f holds, for flat layer l, its cd filter
        biases at offset sum_{i<l} 2 cd_i and then its cd gate biases, the values V h[:, f] that feature column f adds to
        every layer.  ``features``: (F, n).  Computed on the device by the node the forward uses; ``phase`` is only checked
        (it travels next to the table).  With a learned upsampling layer (``local_upsample`` = U > 1) the table holds one row
        per FINE column -- ((n - 1) U, sum 2 cd), row m the values V y[:, m] of ``upsampled_features`` -- and ``features`` needs
        at least ``coarse_frames_needed(1, H, U, phase, interp)`` columns."""
        f = np.asarray(features, dtype=np.float32) if not isinstance(features, torch.Tensor) else features
        if len(f.shape) != 2:
            raise Exception("local_biases: features must be (F, frames), got %s" % (tuple(f.shape),))
        feats, _ = self._local_features(f[None], 1, 1, phase)
        with torch.no_grad():
            if self.local_upsample > 1:
                feats = self._upsample(feats).permute(0, 2, 1)
            return self._local_block(feats)[0].contiguous()

    def condition_biases(self, class_id: int):
        """[(bf, bg)] per residual layer, each (cd,) float32 on the device: the gate biases V E[class_id] that conditioning on
        ``class_id`` adds to every layer -- what an ordinary biased model (``residual_conv_dilation_no_bias = False``) would
        hold as ``wf/b`` and ``wg/b``.  Computed on the device by the node the forward uses."""
        with torch.no_grad():
            row = self._condition_block([int(class_id)], 1)[0]
        return [(row[of:of + lay.cd].clone(), row[og:og + lay.cd].clone())
                for lay, (of, og) in zip(self._flat_layers, self._cond_offsets)]

    # -- optimiser (wavenet.py:457-519) ---------------------------------------------------------
    def setup_optimizer(self):
        p = self.params
        name = str(p.optimizer).lower()
        if name == "adam":
            self.optimizer = AdamState(self, alpha=0.0001, beta1=p.momentum)     # wavenet.py:475, get_optimizer 81-84
        elif name == "eve":
            self.optimizer = EveState(self, alpha=0.0001, beta1=p.momentum)      # wavenet.py:85-86
        elif name in RuleState.RULES:
            self.optimizer = RuleState(self, name, lr=0.0001, momentum=p.momentum)   # wavenet.py:87-96
        else:
            raise Exception("unknown optimizer %r" % p.optimizer)                # wavenet.py:97

    def update_laerning_rate(self, lr):
        """wavenet.py:482-493: Adam/Eve take it as alpha, AdaDelta has no learning rate, everything else as lr."""
        opt = self.optimizer
        if isinstance(opt, RuleState):
            if opt.name != "adadelta":
                opt.lr = lr
            return
        opt.alpha = lr

    def update_momentum(self, momentum):
        """wavenet.py:495-513: beta1 / rho / momentum / alpha by optimizer; SGD and AdaGrad have none.  (For MomentumSGD the
        reference assigns a misspelt attribute, which changes nothing; here the momentum is really updated.)"""
        opt = self.optimizer
        if isinstance(opt, RuleState):
            if opt.name in ("adadelta", "nesterov", "nesterovag", "rmsprop", "momentumsgd"):
                opt.hyper = momentum
            return
        opt.beta1 = momentum

    def zero_grads(self):
        self._grad_arena.zero_()

    def backprop(self, loss):
        """cleargrads -> backward -> [DP all-reduce] -> WeightDecay, GradientClipping -> Adam -> [weight average].

        With :meth:`enable_ema` the average then takes one step towards the new weights, behind the same non-finite-norm
        guard as the optimiser step: a step skipped on the device moves neither.  Like Adam's ``t``, the host clock
        ``_ema_t`` (the schedule of ``ema.ema_decay_at``) advances for such a skipped step too."""
        if self._ema_swapped:
            raise _lib.WaveNetHipError("backprop() inside ema_weights(): the weights are the average there, not the iterate")
        self.zero_grads()
        if callable(loss):
            loss = loss()
        loss.backward()
        gmult = 1.0
        if self._dp_group is not None:
            gmult = self._dp_group.all_reduce_grads(self._grad_arena)
        if isinstance(self.optimizer, EveState):
            lv = float(loss.detach())                                    # Eve feeds the loss back (wavenet.py:73-79)
            if self._dp_group is not None:
                lv = self._dp_group.mean_loss(lv)                        # ... the global batch's, identical on every rank
            self.optimizer.update(gmult, loss=lv)
        else:
            self.optimizer.update(gmult)
        if self._ema_arena is not None:
            self._ema_step()
            self._ema_t += 1
        self._weights_changed()

    # -- exponential moving average of the weights (new capability; schedule: ema.py) ------------
    def enable_ema(self, decay: float = 0.9999, warmup: bool = True):
        """Keep an exponential moving average of the weights: after every optimiser step (``backprop``,
        ``TrainStepGraph.step``) ``e += (1 - decay_t) (w - e)`` with ``decay_t = ema.ema_decay_at(_ema_t, decay, warmup)``,
        one more elementwise launch on the flat arena.  The average starts at the current weights.  Calling this again
        changes ``decay`` / ``warmup`` and keeps the average and its clock.  Evaluate and generate from it inside
        :meth:`ema_weights`; :meth:`save` / :meth:`load` carry it in ``wavenet.ema.npz``."""
        from . import ema
        decay = ema.check_decay(decay)
        if self._ema_arena is None:
            self._ema_arena = self._arena.detach().clone()
            self._ema_t = 0
        self._ema_decay, self._ema_warmup = decay, bool(warmup)

    def disable_ema(self):
        if self._ema_swapped:
            raise _lib.WaveNetHipError("disable_ema() inside ema_weights()")
        self._ema_arena, self._ema_t = None, 0

    @property
    def ema_enabled(self) -> bool:
        return self._ema_arena is not None

    def _ema_step(self, rate_dev=None):
        """The averaging launch.  The rate is taken by value from the schedule at ``_ema_t``, or read from ``rate_dev`` (a
        1-element device tensor: graph replay).  It gets the norm word and clip of the optimiser step just issued, so that a
        step the optimiser skipped is a step the average skips.  Does not advance ``_ema_t``."""
        from . import ema
        _need_gpu(self._arena)
        p = self.params
        clip = float(p.gradient_clipping) if p.gradient_clipping and p.gradient_clipping > 0 else 0.0
        rate = 0.0 if rate_dev is not None else float(ema.ema_rate_at(self._ema_t, self._ema_decay, self._ema_warmup))
        check(_lib.lib().wn_rule_step(_lib.WN_RULE_EMA, ptr(self._ema_arena), ptr(self._arena), None, None,
                                      self._arena.numel(), rate, ptr(rate_dev) if rate_dev is not None else None,
                                      0.0, 0.0, 0.0, ptr(self.optimizer._norm) if clip > 0 else None, clip, 1.0,
                                      stream_ptr()), "wn_rule_step")

    @contextlib.contextmanager
    def ema_weights(self):
        """``with net.ema_weights(): ...``: the model computes with the averaged weights -- ``score``, ``generate``,
        ``state_dict`` -- and with its own again afterwards.  The CONTENTS of the two arenas are exchanged; the pointers,
        which plans, graphs and decoder handles keep, stay put.  Training inside is refused."""
        if self._ema_arena is None:
            raise _lib.WaveNetHipError("ema_weights(): no average is kept (enable_ema)")
        if self._ema_swapped:
            raise _lib.WaveNetHipError("ema_weights() does not nest")
        self._ema_swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_swapped = False

    def _ema_swap(self):
        with torch.no_grad():
            tmp = self._arena.clone()
            self._arena.copy_(self._ema_arena)
            self._ema_arena.copy_(tmp)
        self._weights_changed()

    def ema_state_dict(self) -> Dict[str, np.ndarray]:
        """The average under the keys of :meth:`state_dict`, plus ``ema/t``, ``ema/decay`` and ``ema/warmup``."""
        if self._ema_arena is None:
            raise _lib.WaveNetHipError("ema_state_dict(): no average is kept (enable_ema)")
        src = self._arena if self._ema_swapped else self._ema_arena          # inside ema_weights() the average sits in _arena
        sd = {"%s/%s" % (ln.name, kind): src[o:o + n].view(shape).detach().cpu().numpy().copy()
              for ln, kind, o, n, shape in self._spans}
        sd.update({"ema/t": np.array(self._ema_t), "ema/decay": np.array(self._ema_decay),
                   "ema/warmup": np.array(self._ema_warmup)})
        return sd

    def load_ema_state_dict(self, sd: Dict[str, np.ndarray]):
        """The inverse of :meth:`ema_state_dict`: average, clock, decay and warm-up switch all come from ``sd``."""
        if self._ema_arena is None:
            raise _lib.WaveNetHipError("load_ema_state_dict(): no average is kept (enable_ema)")
        if self._ema_swapped:
            raise _lib.WaveNetHipError("load_ema_state_dict() inside ema_weights()")
        from . import ema
        decay = ema.check_decay(float(sd["ema/decay"]))
        self._check_condition_keys(sd)
        with torch.no_grad():
            for ln, kind, o, n, shape in self._spans:
                key = "%s/%s" % (ln.name, kind)
                if key not in sd:
                    raise KeyError(key)
                a = np.asarray(sd[key], dtype=np.float32)
                if a.shape != tuple(shape):
                    raise Exception("shape of %s is %s, expected %s" % (key, a.shape, tuple(shape)))
                self._ema_arena[o:o + n].copy_(torch.from_numpy(a.reshape(-1)))
        self._ema_t, self._ema_decay, self._ema_warmup = int(sd["ema/t"]), decay, bool(sd["ema/warmup"])

    def last_update_applied(self) -> bool:
        """False when the most recent optimiser step was SKIPPED on the device because the global gradient norm was not
        finite (wn_adam_step, ABI 4: the weights and the optimiser state are untouched by such a step).  Reads one word back
        (a host synchronisation): for the training loop's occasional health check, not for every step.  A caller that sees
        False after a step of the multi-layer backward can set ``exec_flags |= WN_EXEC_NO_MULTI_LAYER_BWD`` and go on --
        the only thing in the library that produces a NaN on purpose is a dataflow wait of that launch that gave up
        (workgroups not co-resident: another process on the GPU, a CU mask).  Two things to know: the guard lives in the
        clipping hook, so with ``gradient_clipping <= 0`` no norm exists and a NaN gradient reaches m and v as in Chainer; and
        the host-side step counter ``t`` (Adam's bias correction) advances for a skipped step too -- un-advancing it would cost
        a host synchronisation per step; the effect is a step size off by the factor sqrt(1-b2^(t+1))/sqrt(1-b2^t) ~ 1.
        ``train_audio.train`` calls this every 100 updates and stops a run whose checks keep failing."""
        nrm = getattr(self.optimizer, "_norm", None)
        if nrm is None or not self.params.gradient_clipping or self.params.gradient_clipping <= 0:
            return True                                                  # no clipping hook, no norm: nothing is ever skipped
        return bool(torch.isfinite(nrm[0]).item())

    # -- device --------------------------------------------------------------------------------
    def to_gpu(self, device=None):
        if not torch.cuda.is_available():
            raise _lib.WaveNetHipError("to_gpu(): no HIP device is visible")
        _lib.lib()
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self._arena = self._arena.detach().to(dev)
        self._grad_arena = self._grad_arena.to(dev)
        if self._ema_arena is not None:
            self._ema_arena = self._ema_arena.to(dev)
        self._bind()
        self._anchor = torch.zeros((1,), device=dev, requires_grad=True)
        self.optimizer.to(dev)
        self._gpu = True
        self._weights_changed()

    @property
    def gpu_enabled(self):
        return self._gpu and torch.cuda.is_available()

    @property
    def device(self):
        return self._arena.device

    # -- small tensor helpers (wavenet.py:531-554) ---------------------------------------------
    def slice_1d(self, x, cut=0):
        if cut < 1:
            raise Exception("CausalSlice1d: cut cannot be less than one.")      # wavenet.py:235-236
        return self.to_variable(x)[:, :, :, cut:]

    def padding_1d(self, x, pad=0):
        return torch.nn.functional.pad(self.to_variable(x), (pad, 0))

    def to_variable(self, x):
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if not isinstance(x, torch.Tensor):
            raise Exception("expected a numpy array or a torch tensor")
        if self._gpu and not x.is_cuda:
            x = x.to(self.device, non_blocking=True)
        return x

    def to_numpy(self, x):
        if isinstance(x, torch.Tensor):
            return x.detach().cpu().numpy()
        return x

    def get_batchsize(self, x):
        return x.shape[0]

    def _Z(self, T, d):
        fw = self.params.residual_conv_filter_width
        return zero_prefix(T, d, fw) if self.compat_zero_prefix else 0

    # -- forward (wavenet.py:556-593) -----------------------------------------------------------
    def forward_one_step(self, x_batch, apply_softmax=True, as_numpy=False, condition=None, local=None, local_phase=0):
        causal_output = self.forward_causal_block(x_batch)
        _, sum_skip_connections = self.forward_residual_block(causal_output, condition=condition, local=local,
                                                              local_phase=local_phase)
        softmax_output = self.forward_softmax_block(sum_skip_connections, apply_softmax=apply_softmax)
        if as_numpy:
            return self.to_numpy(softmax_output)
        return softmax_output

    def forward_causal_block(self, x_batch):
        """Accepts the reference's one-hot image (B,Q,1,T) float32 *or* integer tokens (B,T): for
        tokens the first layer is a row gather (out = W[:,idx[t-1],0] + W[:,idx[t],1]) instead of a
        dense conv over 256 mostly-zero channels."""
        x = self.to_variable(x_batch)
        _need_gpu(x)
        layers = self.causal_conv_layers
        if self.storage == "bf16":
            if x.is_floating_point() or x.dim() != 2 or len(layers) != 1:
                raise Exception("storage='bf16' takes integer (B, T) tokens and one causal layer")
            l0 = layers[0]
            out = _Embed16Fn.apply(x.to(torch.int32).contiguous(), l0.W, l0.b, l0.filter_width, self)
            self._last_causal_outputs = [out]
            return _as_view(out)
        if not x.is_floating_point():
            if x.dim() != 2:
                raise Exception("integer input must be (B, T) tokens")
            l0 = layers[0]
            out = _EmbedFn.apply(x.to(torch.int32).contiguous(), l0.W, l0.b, l0.filter_width, self)
            start = 1
        else:
            out = _to_btc(x.to(torch.float32))
            start = 0
        outs = [out] if start == 1 else []
        for lay in layers[start:]:
            out = _ConvFn.apply(out, lay.W, lay.b, lay.filter_width, 1, 0, self._hook)
            outs.append(out)
        self._last_causal_outputs = outs                          # FasterWaveNet seeds its rings from these
        return _as_view(out)

    def forward_residual_block(self, x_batch, t_off: int = 0, window_only: bool = False, condition=None, local=None,
                               local_phase: int = 0):
        """(output, sum_skip_connections).  ``t_off`` > 0 (an extension) computes the skip sum for
        columns t_off.. only -- what train.py:73 keeps -- instead of slicing it afterwards.
        ``window_only`` (training, where train.py:72 discards the residual output): columns that cannot influence
        ``skip[t_off:]`` are not computed at all, so the returned residual output is UNDEFINED below the window's
        receptive field and must not be used; loss and gradients are unchanged.
        ``condition``: one class id per clip, for a globally conditioned model (and only for one).
        ``local`` / ``local_phase``: (B, F, n) float32 features and the phase of position 0 inside its feature column, for a
        locally conditioned model (and only for one); see ``local_alignment``.  ``local_phase`` is an int (every clip at that
        phase) or one phase per clip -- a 1-D sequence, numpy array or integer tensor, each entry in [0, local_hop): the
        phases then travel in device memory (``WnStackDesc.bias_phase_tab``) and every clip needs
        ``frames_needed(T, H, H - 1, interp)`` columns, whatever its phase.  With a learned upsampling layer
        (``local_upsample`` = U > 1) ``local`` and ``local_phase`` mean the same -- coarse columns at hop H, phases in [0, H) --
        and the call needs ``coarse_frames_needed(T, H, U, phase, interp)`` columns (``phase=None`` for a phase per clip)."""
        x = self.to_variable(x_batch)
        _need_gpu(x)
        cond = self._condition_block(condition, int(x.shape[0]))
        feats, phase = self._local_features(local, int(x.shape[0]), int(x.shape[3]), local_phase)
        rows = None
        if feats is not None:
            feats, hop, phase = self._stack_features(feats, phase, int(x.shape[3]))
            cond = self._local_block(feats, cond)
            if self.storage == "bf16":
                # the bf16 calls carry no clip stride: clip blocks are dense, surplus columns are trimmed (a slice autograd
                # sees, so the gradient finds its way back)
                worst = hop - 1 if isinstance(phase, LocalPhases) else int(phase)
                cond = cond[:, :frames_needed(int(x.shape[3]), hop, worst, self.local_interp)]
            cond = cond.contiguous()
            rows = GateBiasRows(self, cond, hop, phase, LOCAL_INTERP.index(self.local_interp))
        elif cond is not None:
            cond = cond.contiguous()
            rows = GateBiasRows(self, cond)
        if self.storage == "bf16":
            self._pack16_if_stale()
            out, skip = _Stack16Fn.apply(_to_btc(x), self._anchor, self, int(t_off), torch.is_grad_enabled(), cond, rows)
            return _as_view(out), _as_view(skip)
        out, skip = _StackFn.apply(_to_btc(x), self._anchor, self, int(t_off), torch.is_grad_enabled(),
                                   bool(window_only), cond, rows)
        return _as_view(out), _as_view(skip)

    def forward_softmax_block(self, x_batch, apply_softmax=True, activation: Optional[str] = None):
        x = self.to_variable(x_batch)
        _need_gpu(x)
        act = ACT[activation or self.head_activation]
        out = _to_btc(x)
        if self.storage == "bf16":
            self._pack16_if_stale()
            n = len(self.softmax_conv_layers)
            for i, (lay, (wb, wbt)) in enumerate(zip(self.softmax_conv_layers, self._head16)):
                out = _Pointwise16Fn.apply(out, lay.W, lay.b, wb, wbt, act, i == n - 1, self._hook)
            if apply_softmax:
                out = _SoftmaxFn.apply(out)
            return _as_view(out)
        for lay in self.softmax_conv_layers:
            out = _PointwiseFn.apply(out, lay.W, lay.b, act, self)
        if apply_softmax:
            out = _SoftmaxFn.apply(out)
        return _as_view(out)

    # -- loss (wavenet.py:597-617) ----------------------------------------------------------------
    def cross_entropy(self, raw_network_output, target_signal_data):
        if isinstance(target_signal_data, torch.Tensor) and target_signal_data.requires_grad:
            raise Exception("target_signal_data cannot be Variable")
        raw = self.to_variable(raw_network_output)
        _need_gpu(raw)
        n_norm = -1            # device-resident targets: the rows that count (label != -1) are counted on the device
        if not isinstance(target_signal_data, torch.Tensor):
            # a host array (what the reference requires): labels are checked here -- Chainer type-checks them too -- and
            # -1 is chainer's ignore_label: such rows carry no loss and do not count in the mean
            lab = np.asarray(target_signal_data)
            Q = raw.shape[1]
            if lab.size and (lab.min() < -1 or lab.max() >= Q):
                raise Exception("cross_entropy: labels must lie in [0, %d) or be -1 (ignored)" % Q)
            n_norm = max(int((lab != -1).sum()), 1)
        tgt = self.to_variable(np.asarray(target_signal_data) if not isinstance(target_signal_data, torch.Tensor)
                               else target_signal_data)
        if raw.shape[3] != tgt.shape[1]:
            raise Exception("raw_network_output.width != target.width")
        rows = _to_btc(raw)                                        # row b*T'+t, as after the reference's transpose
        B, Tw, Q = rows.shape
        return _XentFn.apply(rows.reshape(B * Tw, Q).contiguous(), tgt.to(torch.int32).reshape(-1).contiguous(), n_norm)

    def head_cross_entropy(self, sum_skip, target_signal_data):
        """``cross_entropy(forward_softmax_block(sum_skip, apply_softmax=False), target)`` (wavenet.py:584-617), with the LAST head
        convolution and the loss as one launch when the library covers it (fp32 storage, fp16x2 arithmetic, 256 quantisation
        steps: ``wn_head_xent``) -- the (B, Q, 1, T') logits then never reach memory (200 MB less traffic per step at config 2).
        Same loss, same gradients (the products are the skip path's fp16x2 split instead of the head's six-term split: 1e-6);
        anything the fused launch does not cover runs the two calls.  New capability: the reference has no such method; the
        captured training step (``TrainStepGraph`` / ``graph.default_loss``) uses it."""
        x = self.to_variable(sum_skip)
        _need_gpu(x)
        tensor_target = isinstance(target_signal_data, torch.Tensor)
        if tensor_target and target_signal_data.requires_grad:
            raise Exception("target_signal_data cannot be Variable")
        lay = self.softmax_conv_layers[-1]
        n_rows = int(x.shape[0]) * int(x.shape[-1])                 # (B, C, 1, T') -> B * T' rows of the loss
        fused = (self.storage != "bf16" and self.fuse_head_loss and
                 _lib.lib().wn_head_xent_supported(n_rows, lay.W.shape[1], lay.W.shape[0], self._exec()) == 1)
        if not fused:
            return self.cross_entropy(self.forward_softmax_block(x, apply_softmax=False), target_signal_data)
        act = ACT[self.head_activation]
        out = _to_btc(x)
        for l2 in self.softmax_conv_layers[:-1]:
            out = _PointwiseFn.apply(out, l2.W, l2.b, act, self)
        n_norm = -1
        if not tensor_target:
            lab = np.asarray(target_signal_data)
            Q = lay.W.shape[0]
            if lab.size and (lab.min() < -1 or lab.max() >= Q):
                raise Exception("cross_entropy: labels must lie in [0, %d) or be -1 (ignored)" % Q)
            n_norm = max(int((lab != -1).sum()), 1)
        tgt = self.to_variable(np.asarray(target_signal_data) if not tensor_target else target_signal_data)
        if out.shape[1] != tgt.shape[1]:
            raise Exception("raw_network_output.width != target.width")
        return _HeadXentFn.apply(out, lay.W, lay.b, tgt.to(torch.int32).reshape(-1).contiguous(), act, n_norm, self)

    # -- scoring: per-position negative log-likelihoods, no autograd (new capability; wavenet_amd/scoring.py) -------------------
    def head_token_nll(self, sum_skip, target):
        """The per-position form of :meth:`head_cross_entropy`: (B, T') float32 on the device, entry (b, t) the negative
        log-likelihood in nats of ``target[b, t]`` under the head's softmax at that column, and 0 for a label outside
        [0, Q) (the ignore label -1).  Runs without autograd.  Where ``head_cross_entropy`` would fuse (fp32 storage,
        ``fuse_head_loss``, ``wn_head_xent_supported``) the last head convolution and the rows are ONE launch,
        ``wn_head_xent`` under WN_EXEC_HEAD_ROW_NLL: neither logits nor a gradient reach memory.  Everywhere else:
        ``forward_softmax_block(apply_softmax=False)``, then logsumexp - gather in torch."""
        with torch.no_grad():
            x = self.to_variable(sum_skip)
            _need_gpu(x)
            tgt = self.to_variable(np.asarray(target) if not isinstance(target, torch.Tensor) else target)
            if tgt.dim() != 2 or x.shape[0] != tgt.shape[0] or x.shape[3] != tgt.shape[1]:
                raise Exception("head_token_nll: target must be (B, T') like the skip sum, got %s for %s"
                                % (tuple(tgt.shape), tuple(x.shape)))
            B, Tw = int(tgt.shape[0]), int(tgt.shape[1])
            lay = self.softmax_conv_layers[-1]
            Q = lay.W.shape[0]
            fused = (self.storage != "bf16" and self.fuse_head_loss and B * Tw > 0 and
                     _lib.lib().wn_head_xent_supported(B * Tw, lay.W.shape[1], Q, self._exec()) == 1)
            if not fused:
                rows = _to_btc(self.forward_softmax_block(x, apply_softmax=False)).to(torch.float32)      # (B, T', Q)
                lab = tgt.to(torch.int64)
                counts = (lab >= 0) & (lab < Q)
                picked = rows.gather(2, lab.clamp(0, Q - 1).unsqueeze(2)).squeeze(2)
                return torch.where(counts, torch.logsumexp(rows, dim=2) - picked, torch.zeros_like(picked))
            act = ACT[self.head_activation]
            out = _to_btc(x)
            for l2 in self.softmax_conv_layers[:-1]:
                out = _PointwiseFn.apply(out, l2.W, l2.b, act, self)
            x2 = out.reshape(B * Tw, out.shape[-1]).contiguous()
            buf = torch.empty((_lib.XENT_LOSS_WORDS,), device=x.device, dtype=torch.float32)
            nll = torch.empty((B, Tw), device=x.device, dtype=torch.float32)
            # n_norm = 0: the mean in buf[0] runs over all rows (nobody reads it here; no counting launch)
            check(_lib.lib().wn_head_xent(ptr(x2), ptr(lay.W), ptr(lay.b), ptr(tgt.to(torch.int32).reshape(-1).contiguous()),
                                          ptr(buf), ptr(nll), B * Tw, x2.shape[1], Q, act, 0,
                                          self._exec(call_flags=_lib.WN_EXEC_HEAD_ROW_NLL), stream_ptr()), "wn_head_xent")
            return nll

    def token_nll(self, x, tgt, condition=None, local=None, local_phase=0):
        """The per-position form of ``graph.default_loss``: (B, tgt.shape[1]) float32 negative log-likelihoods of ``tgt``
        under the last ``tgt.shape[1]`` output columns of the window ``x`` (tokens (B, T) or a one-hot image).  Inference
        form: nothing is saved for a backward."""
        with torch.no_grad():
            c = self.forward_causal_block(x)
            _, s = self.forward_residual_block(c, t_off=int(c.shape[3]) - int(tgt.shape[1]), condition=condition, local=local,
                                               local_phase=local_phase)
            return self.head_token_nll(s, tgt)

    def score(self, tokens, chunk_width: int = 16384, batch_size: int = 8, condition=None, local=None):
        """(n,) float32 on the device: the negative log-likelihood in nats of every sample of the 1-D token sequence
        ``tokens``, each given all samples before it (silence before the first), teacher-forced.  See
        :func:`wavenet_amd.scoring.score` for the definition and the two knobs, which do not change the result beyond
        arithmetic.  ``condition``: the class id of the whole sequence, for a globally conditioned model.  ``local``: the
        sequence's (F, frames) features, for a locally conditioned one."""
        from . import scoring
        return scoring.score(self, tokens, chunk_width=chunk_width, batch_size=batch_size, condition=condition, local=local)

    # -- the deferred skip projection -----------------------------------------------------------
    def _skip_sum(self, zs: Sequence[torch.Tensor], skip: torch.Tensor, B, T, t_off, Tw):
        L = self._flat_layers
        check(_lib.lib().wn_skip_sum_fwd(
            len(L), ptr_array(zs), ptr_array([lay.projection_softmax.W for lay in L]),
            ptr_array([lay.projection_softmax.b for lay in L]), int_array([lay.cd for lay in L]), ptr(skip), B, T,
            t_off, Tw, self._Cs, 0, self._exec(B), stream_ptr()), "wn_skip_sum_fwd")

    # -- checkpoints (wavenet.py:619-639): reference key names; .npz for weights + optimizer, and the reference's own
    #    HDF5 container for the weights (read and written through h5py when importable, else through the HDF5 C library:
    #    hdf5_io.py) --
    def save(self, model_dir="./"):
        """When an HDF5 library is at hand, the weights as ``wavenet.model`` in the reference's own container -- the file its
        ``load`` opens (wavenet.py:627-633) -- and THEN ``wavenet.model.npz`` + ``wavenet.opt.npz``: written last, the .npz is
        the newer of the two weight files, so :meth:`load` takes it after every ``save`` and needs no HDF5 library for a
        checkpoint this package wrote.  With :meth:`enable_ema`, also the average as ``wavenet.ema.npz``."""
        if self._ema_swapped:
            raise _lib.WaveNetHipError("save() inside ema_weights(): the two weight files would change places")
        os.makedirs(model_dir, exist_ok=True)
        from . import hdf5_io
        if hdf5_io.available():
            self.save_hdf5(os.path.join(model_dir, "wavenet.model"))
        np.savez(os.path.join(model_dir, "wavenet.model.npz"), **self.state_dict())
        np.savez(os.path.join(model_dir, "wavenet.opt.npz"), **self.optimizer.state_dict())
        if self._ema_arena is not None:
            np.savez(os.path.join(model_dir, EMA_FILE), **self.ema_state_dict())

    def save_hdf5(self, filename):
        """The weights in the file format and layout of the reference's ``serializers.save_hdf5(model_dir +
        "/wavenet.model", self.chain)`` (wavenet.py:619-625): one group per link, datasets ``W`` and ``b``, gzip 4 --
        a file the reference's ``load`` (wavenet.py:627-639) reads."""
        from . import hdf5_io
        hdf5_io.write_datasets(filename, self.state_dict(), compression=4)

    def load_hdf5(self, filename):
        """Weights saved by the reference itself (``serializers.save_hdf5(model_dir + "/wavenet.model", self.chain)``,
        wavenet.py:619-625): Chainer writes one dataset per parameter at ``<link name>/W`` and ``<link name>/b`` -- the
        key names of :meth:`state_dict`.  Read with h5py when it is importable, otherwise with the HDF5 C library through
        ``hdf5_io`` (ImportError, naming what was looked for, when neither exists).  A file that lacks one of the model's
        parameters, or holds it in another shape, is refused (KeyError / Exception from :meth:`load_state_dict`) -- the
        reference's deserializer fails on such a file too."""
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            sd = {}
            with h5py.File(filename, "r") as f:
                def visit(name, obj):
                    if isinstance(obj, h5py.Dataset):
                        sd[name] = np.asarray(obj)
                f.visititems(visit)
        else:
            from . import hdf5_io
            sd = hdf5_io.read_datasets(filename)
        self._check_condition_keys(sd)
        self.load_state_dict({k: v for k, v in sd.items() if k in self.state_dict()})

    def load(self, model_dir="./", weights: str = "model"):
        """wavenet.py:627-639.  Two weight files may sit in the directory: the reference's own HDF5 ``wavenet.model`` and this
        package's ``wavenet.model.npz``.  The HDF5 file is loaded when it is the only one or the NEWER one (modification time:
        a reference-written checkpoint dropped next to an older .npz must not be ignored silently -- that case is announced);
        :meth:`save` writes the .npz last, so a directory this package saved loads from the .npz without a word and without an
        HDF5 library.  If the HDF5 file is newer but no HDF5 library can be found, the .npz next to it is loaded with a
        warning instead of failing.

        With :meth:`enable_ema` the average comes from ``wavenet.ema.npz``; when weights were loaded and that file is not
        there, the average starts again from them (``_ema_t = 0``), which is announced.  Without it the file is ignored.
        ``weights="ema"`` loads the AVERAGED weights of that file as the model's weights -- evaluation and generation from a
        checkpoint -- and nothing else (no optimiser state: it belongs to the iterate); it raises when the file is absent."""
        if weights not in ("model", "ema"):
            raise ValueError("weights must be 'model' or 'ema', got %r" % (weights,))
        if self._ema_swapped:
            raise _lib.WaveNetHipError("load() inside ema_weights()")
        ema_fn = os.path.join(model_dir, EMA_FILE)
        if weights == "ema":
            if not os.path.isfile(ema_fn):
                raise FileNotFoundError("%s: this checkpoint holds no averaged weights (it was trained without --ema-decay / "
                                        "enable_ema)" % ema_fn)
            print("loading", ema_fn, "...")
            with np.load(ema_fn) as z:
                sd = {k: z[k] for k in z.files}
            self.load_state_dict(sd)
            if self._ema_arena is not None:
                self.load_ema_state_dict(sd)
            return
        h5 = os.path.join(model_dir, "wavenet.model")
        nz = os.path.join(model_dir, "wavenet.model.npz")
        have_h5, have_nz = os.path.isfile(h5), os.path.isfile(nz)
        use_h5 = have_h5 and (not have_nz or os.path.getmtime(h5) > os.path.getmtime(nz))
        if use_h5 and have_nz:
            print("both %s and %s exist: loading the newer one (%s)" % (h5, nz, h5))
        if use_h5:
            print("loading", h5, "...")
            try:
                self.load_hdf5(h5)
            except ImportError as e:
                if not have_nz:
                    raise
                print("cannot read %s (%s): loading the OLDER %s instead" % (h5, e, nz))
                use_h5 = False
        if not use_h5 and have_nz:                                              # silently skipped when absent, like the reference
            print("loading", nz, "...")
            with np.load(nz) as z:
                self.load_state_dict({k: z[k] for k in z.files})
        fn = os.path.join(model_dir, "wavenet.opt.npz")
        if os.path.isfile(fn):
            print("loading", fn, "...")
            with np.load(fn) as z:
                self.optimizer.load_state_dict({k: z[k] for k in z.files})
        if self._ema_arena is not None:
            if os.path.isfile(ema_fn):
                print("loading", ema_fn, "...")
                with np.load(ema_fn) as z:
                    self.load_ema_state_dict({k: z[k] for k in z.files})
            elif use_h5 or have_nz:
                print("no %s: the weight average starts again from the weights just loaded" % ema_fn)
                with torch.no_grad():
                    self._ema_arena.copy_(self._arena)
                self._ema_t = 0

    # -- data parallel (new capability) -----------------------------------
    def enable_data_parallel(self, group=None, always_reduce: bool = False):
        from .dp import DataParallel
        self._dp_group = DataParallel(self, group, always_reduce=always_reduce)
        return self._dp_group


class AdamState(object):
    """Chainer's Adam on the flat arena, with the reference's hook order (WeightDecay, then
    GradientClipping; wavenet.py:477-480), as two kernel launches per step."""

    def __init__(self, net: WaveNet, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8):
        self.net = net
        self.alpha, self.beta1, self.beta2, self.eps = alpha, beta1, beta2, eps
        self.t = 0
        self.m = torch.zeros_like(net._arena)
        self.v = torch.zeros_like(net._arena)
        self._norm = torch.zeros((_lib.SQNORM_WORDS,), dtype=torch.float32)

    def to(self, dev):
        self.m, self.v, self._norm = self.m.to(dev), self.v.to(dev), self._norm.to(dev)

    @property
    def lr(self):
        fix1 = 1.0 - self.beta1 ** self.t
        fix2 = 1.0 - self.beta2 ** self.t
        return self.alpha * math.sqrt(fix2) / fix1

    def update(self, grad_mult: float = 1.0, lr_dev=None):
        """One optimiser step.  ``lr_dev`` (1-element device tensor) makes the kernel read the bias-corrected
        step size from device memory instead of taking ``self.lr`` by value (graph.TrainStepGraph)."""
        net = self.net
        _need_gpu(net._arena)
        self.t += 1
        p = net.params
        lib, st = _lib.lib(), stream_ptr()
        n = net._arena.numel()
        clip = float(p.gradient_clipping) if p.gradient_clipping and p.gradient_clipping > 0 else 0.0
        wd = float(p.weight_decay) if p.weight_decay and p.weight_decay > 0 else 0.0
        norm_ptr = None
        if clip > 0:
            check(lib.wn_sqnorm(ptr(net._grad_arena), ptr(net._arena), n, grad_mult, wd, ptr(self._norm), st),
                  "wn_sqnorm")
            norm_ptr = ptr(self._norm)
        if lr_dev is not None:
            check(lib.wn_adam_step_dev(ptr(net._arena), ptr(net._grad_arena), ptr(self.m), ptr(self.v), n, ptr(lr_dev),
                                       self.beta1, self.beta2, self.eps, wd, norm_ptr, clip, grad_mult, st),
                  "wn_adam_step_dev")
            return
        check(lib.wn_adam_step(ptr(net._arena), ptr(net._grad_arena), ptr(self.m), ptr(self.v), n, self.lr,
                               self.beta1, self.beta2, self.eps, wd, norm_ptr, clip, grad_mult, st), "wn_adam_step")

    def state_dict(self):
        return {"t": np.array(self.t), "alpha": np.array(self.alpha), "m": self.m.cpu().numpy(),
                "v": self.v.cpu().numpy()}

    def _hooks(self, grad_mult):
        """WeightDecay then GradientClipping (wavenet.py:477-480): returns (norm pointer or None, clip, wd)."""
        net = self.net
        p = net.params
        clip = float(p.gradient_clipping) if p.gradient_clipping and p.gradient_clipping > 0 else 0.0
        wd = float(p.weight_decay) if p.weight_decay and p.weight_decay > 0 else 0.0
        norm_ptr = None
        if clip > 0:
            check(_lib.lib().wn_sqnorm(ptr(net._grad_arena), ptr(net._arena), net._arena.numel(), grad_mult, wd,
                                       ptr(self._norm), stream_ptr()), "wn_sqnorm")
            norm_ptr = ptr(self._norm)
        return norm_ptr, clip, wd

    def load_state_dict(self, sd):
        self.t = int(sd["t"])
        self.alpha = float(sd["alpha"])
        self.m.copy_(torch.from_numpy(np.asarray(sd["m"])))
        self.v.copy_(torch.from_numpy(np.asarray(sd["v"])))


class EveState(AdamState):
    """The reference's Eve optimizer (wavenet.py:10-79; Koushik & Hayashi 2016) on the flat arena: Adam's moments, the
    update divided by ``d * sqrt(v) + eps`` where the scalar ``d`` tracks the relative change of the (clamped) loss.
    Every parameter of the reference carries its own copy of (d, f) and updates it with the same loss at the same t
    (wavenet.py:27-44 is called per parameter), so they are one pair of host scalars here."""

    def __init__(self, net, alpha=0.001, beta1=0.9, beta2=0.999, beta3=0.999, eps=1e-8, lower_threshold=0.1,
                 upper_threshold=10):
        super().__init__(net, alpha, beta1, beta2, eps)
        self.beta3, self.lower_threshold, self.upper_threshold = beta3, lower_threshold, upper_threshold
        self.d, self.f = 1.0, 0.0                                    # wavenet.py:25-26

    def _update_d_and_f(self, loss: float):
        d32, f32 = np.float32(self.d), np.float32(self.f)            # the reference keeps both in float32 arrays
        if self.t > 1:
            old_f = float(f32)
            if loss > old_f:
                delta, Delta = self.lower_threshold + 1.0, self.upper_threshold + 1.0
            else:
                delta, Delta = 1.0 / (self.upper_threshold + 1.0), 1.0 / (self.lower_threshold + 1.0)
            c = min(max(delta, loss / (old_f + 1e-12)), Delta)
            new_f = c * old_f
            r = abs(new_f - old_f) / (min(new_f, old_f) + 1e-12)
            d32 = np.float32(d32 + np.float32((1 - self.beta3) * (r - float(d32))))
            f32 = np.float32(new_f)
        else:
            f32 = np.float32(loss)
        self.d, self.f = float(d32), float(f32)

    def update(self, grad_mult: float = 1.0, loss=None, lr_dev=None):
        if loss is None:
            raise RuntimeError("Eve.update requires the loss value")            # wavenet.py:75-76
        if lr_dev is not None:
            raise RuntimeError("Eve needs the loss on the host every step: it cannot run inside a replayed graph")
        net = self.net
        _need_gpu(net._arena)
        self.t += 1
        self._update_d_and_f(float(loss))
        norm_ptr, clip, wd = self._hooks(grad_mult)
        check(_lib.lib().wn_eve_step(ptr(net._arena), ptr(net._grad_arena), ptr(self.m), ptr(self.v), net._arena.numel(),
                                     self.lr, self.beta1, self.beta2, self.eps, self.d, wd, norm_ptr, clip, grad_mult,
                                     stream_ptr()), "wn_eve_step")

    def state_dict(self):
        sd = super().state_dict()
        sd.update(d=np.array(self.d), f=np.array(self.f))
        return sd

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        self.d, self.f = float(sd["d"]), float(sd["f"])


class RuleState(object):
    """The other optimizers ``get_optimizer`` names (wavenet.py:87-96): Chainer's SGD, MomentumSGD, AdaGrad, AdaDelta,
    NesterovAG and RMSprop on the flat arena, behind the same hooks as Adam (``wn_rule_step``).  Constructor arguments
    follow get_optimizer: ``lr`` where the rule has one, the model's ``momentum`` as momentum / rho (AdaDelta) / alpha
    (RMSprop).  The reference's "momentumsgd" line misspells two names and raises NameError before it can train; the
    rule itself is implemented here."""

    #            rule id, uses momentum hyper, eps (Chainer defaults)
    RULES = {"sgd": (0, False, 0.0), "momentumsgd": (1, True, 0.0), "adagrad": (2, False, 1e-8),
             "adadelta": (3, True, 1e-6), "nesterov": (4, True, 0.0), "nesterovag": (4, True, 0.0),
             "rmsprop": (5, True, 1e-8)}

    def __init__(self, net, name: str, lr=0.0001, momentum=0.9):
        self.net, self.name = net, name.lower()
        self.rule, uses_hyper, self.eps = self.RULES[self.name]
        self.lr = lr
        self.hyper = momentum if uses_hyper else 0.0
        self.t = 0
        # m = first state array (v / h / ms / msg), v = second (AdaDelta's msdx): the names TrainStepGraph snapshots
        self.m = torch.zeros_like(net._arena) if self.rule != 0 else torch.zeros((1,), dtype=torch.float32)
        self.v = torch.zeros_like(net._arena) if self.rule == 3 else torch.zeros((1,), dtype=torch.float32)
        self._norm = torch.zeros((_lib.SQNORM_WORDS,), dtype=torch.float32)

    def to(self, dev):
        self.m, self.v, self._norm = self.m.to(dev), self.v.to(dev), self._norm.to(dev)

    _hooks = AdamState._hooks

    def update(self, grad_mult: float = 1.0, lr_dev=None):
        net = self.net
        _need_gpu(net._arena)
        self.t += 1
        norm_ptr, clip, wd = self._hooks(grad_mult)
        check(_lib.lib().wn_rule_step(self.rule, ptr(net._arena), ptr(net._grad_arena),
                                      ptr(self.m) if self.rule != 0 else None, ptr(self.v) if self.rule == 3 else None,
                                      net._arena.numel(), self.lr, ptr(lr_dev) if lr_dev is not None else None,
                                      self.hyper, self.eps, wd, norm_ptr, clip, grad_mult, stream_ptr()), "wn_rule_step")

    def state_dict(self):
        return {"t": np.array(self.t), "lr": np.array(self.lr), "hyper": np.array(self.hyper),
                "m": self.m.cpu().numpy(), "v": self.v.cpu().numpy()}

    def load_state_dict(self, sd):
        self.t, self.lr, self.hyper = int(sd["t"]), float(sd["lr"]), float(sd["hyper"])
        self.m.copy_(torch.from_numpy(np.asarray(sd["m"])))
        self.v.copy_(torch.from_numpy(np.asarray(sd["v"])))
