"""`FasterWaveNet` with the reference's face (faster_wavenet.py:11-113), backed by the HIP decoder.

The reference caches every layer's full-window output and rolls all caches by one column per
generated sample.  Here the state is a handle owned by libwavenet_hip.so: per-layer rings of the
last (fw-1)*d input columns in HBM, advanced by one persistent kernel (csrc/decoder.hip).

What a caller can observe:
* ``_forward_one_step`` returns the reference's ``(1, Q, 1, W)`` -- every column of the rolled window under the ELU head,
  the newest last (faster_wavenet.py:105-113) -- from a device-side ring of the window's logits (``keep_window``, on by
  default since round 6).  The reference's caller reads ``[0, :, 0, -1]`` only (train_audio/generate.py:38);
  ``full_window=False`` (or ``keep_window = False`` before the prefill) returns just that newest column as
  ``(1, Q, 1, 1)`` and skips the per-call window concatenation + W-row softmax.  ``generate()`` never builds the window.
* only the newest token of ``x_batch_data`` is read (the reference also reads nothing else of it:
  wavenet.py:286), and an integer token may be passed instead of the one-hot window.
"""
from __future__ import annotations

import collections
import contextlib
import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

from . import _lib, sampling
from ._lib import check, ptr, ptr_array, int_array, stream_ptr, ACT
from .wavenet import WaveNet, _as_view, _need_gpu


class _RingState(object):
    """Marker stored in prev_causal_outputs / prev_residual_outputs (the state itself is on the GPU)."""

    def __init__(self, what):
        self.what = what

    def __repr__(self):
        return "<device ring state: %s>" % self.what


def deal_launches(lengths, limit, longest_first=True):
    """Deal utterances of ``lengths[i]`` decode steps to launches of at most ``limit`` utterances each: sorted longest first
    (stable: equal lengths keep the caller's order), then cut into runs of ``limit``.  Returns ``[(n, [i, ...]), ...]`` -- a
    launch's step count ``n`` (its longest utterance's) and the caller's indices of its utterances in the order their handles
    are passed, longest first.  Every index appears exactly once, so results go back to the caller's order by index.  Utterances
    of similar length share a launch: the launch lasts as long as its longest one.  ``longest_first=False`` (the other side of
    tools/time_ragged_decode.py's comparison) keeps the same launches and passes each one's handles in the caller's order."""
    lengths = [int(v) for v in lengths]
    limit = int(limit)
    if limit < 1:
        raise ValueError("deal_launches: limit must be at least 1, got %d" % limit)
    order = sorted(range(len(lengths)), key=lambda i: -lengths[i])             # sorted() is stable
    launches = [(lengths[order[c0]], order[c0:c0 + limit]) for c0 in range(0, len(order), limit)]
    return launches if longest_first else [(n, sorted(idx)) for n, idx in launches]


TILE_SIZES = (2, 4, 8, 16)             # wn_decoder_run_batch's same_weights values that are tile sizes (up to WN_DECODER_TILE_MAX)
_TILE_LDS_BYTES = 150 * 1024           # the library's bound on a decode workgroup's LDS (csrc/decoder.hip)


def tile_lds_bytes(params, U):
    """LDS of a tile of ``U`` utterances, as the library counts it: U x (7 maxc + 16) floats, maxc the widest channel count
    of the model (Q, causal, dilated and head channels)."""
    maxc = max([int(params.quantization_steps)] + [int(c) for c in params.causal_conv_channels] +
               [int(c) for c in params.residual_conv_channels] + [int(c) for c in params.softmax_conv_channels])
    return int(U) * (7 * maxc + 16) * 4


def tile_fit(params):
    """The largest U in {1, 2, 4, 8, 16} whose tile fits the LDS bound: the host's restatement of the rule
    ``wn_decoder_run_batch`` refuses a tile by (``WN_ESHAPE``).  1: this model decodes one utterance per workgroup only."""
    return max([1] + [U for U in TILE_SIZES if tile_lds_bytes(params, U) <= _TILE_LDS_BYTES])


def pick_tile(n_utterances, n_cu, fit):
    """``tile="auto"``: the tile size of a launch of ``n_utterances`` on a device of ``n_cu`` compute units for a model whose
    ``tile_fit`` is ``fit``; 0 = off.  A pure function.  The rule is read off profiles/tiled_decode.json (DESIGN "Decoding in
    utterance tiles"): on both measured shapes and at every measured N from 16 to 1,024 -- 8 to 512 workgroups on 256 CUs --
    U = 2 was the fastest by far and every larger U slower than it, because a step of ``k_decode_tile`` costs more the more slots
    a workgroup holds while a launch of at most 1,024 utterances never runs out of CUs.  So: 2 wherever a tile applies.  The
    starting rule -- the largest fitting U with ceil(N / U) >= n_cu -- picked off or 4 where 2 was 2 to 15 times faster.
    ``n_cu`` stays an argument: a rule for launches that outnumber what the device holds would need it."""
    return 2 if int(n_utterances) >= 2 and int(fit) >= 2 and int(n_cu) >= 1 else 0


def check_tile(tile, params=None, what="generate_batch"):
    """``tile=`` as ``generate_batch`` / ``open_stream`` take it -> 0 (off), a tile size or ``"auto"``.  Raises ``ValueError`` for
    anything else and, given ``params``, for a U that does not fit the model -- naming ``tile_fit``'s value --, all without a
    device."""
    if isinstance(tile, str):
        if tile != "auto":
            raise ValueError("%s: tile= takes 0 / 1 (off), 2, 4, 8, 16 or \"auto\", got %r" % (what, tile))
        return "auto"
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or int(tile) not in (0, 1) + TILE_SIZES:
        raise ValueError("%s: tile= takes 0 / 1 (off), 2, 4, 8, 16 or \"auto\", got %r" % (what, tile))
    U = 0 if int(tile) < 2 else int(tile)
    if U and params is not None and U > tile_fit(params):
        raise ValueError("%s: tile=%d does not fit this model: a tile keeps %d bytes in LDS, the bound is %d; the largest tile that "
                         "fits (tile_fit) is %d" % (what, U, tile_lds_bytes(params, U), _TILE_LDS_BYTES, tile_fit(params)))
    return U


StreamFrames = collections.namedtuple("StreamFrames", "steps current reads min_ring")


def stream_frames(hop, linear, phase, fed=0, done=0, pull=0):
    """THE arithmetic of a frame ring (``WN_DECODER_FRAME_RING``, ``DecodeStream``), in one place.  A decoder whose table was set
    with phase ``phase`` in [0, hop) reads, at its k-th step (k = 0, 1, ...), frame (phase + k) // hop -- and, with ``linear``
    interpolation, the frame after it.  With frames 0 .. ``fed`` - 1 fed so far and ``done`` steps run:

    * ``steps``: how many more steps the frames fed allow -- max(0, (fed - linear) * hop - phase - done);
    * ``current``: the frame of the next step, (phase + done) // hop -- every frame before it is consumed, and a ring of R rows
      may be fed up to frame ``current`` + R - 1 without overwriting a row that is still to be read;
    * ``reads``: the frames a run of ``pull`` more steps reads at once (0 for ``pull`` = 0) -- the library refuses a run that
      reads more than R, because a launch cannot be refilled while it runs;
    * ``min_ring``: the smallest R that takes a run of ``pull`` steps wherever it starts: ceil((pull - 1) / hop) + 1 + linear
      (0 for ``pull`` = 0)."""
    hop, lin, phase, fed, done, pull = int(hop), 1 if linear else 0, int(phase), int(fed), int(done), int(pull)
    if hop < 1 or not 0 <= phase < hop or fed < 0 or done < 0 or pull < 0:
        raise ValueError("stream_frames: needs hop >= 1, 0 <= phase < hop and non-negative counts, got hop %d, phase %d, fed %d, "
                         "done %d, pull %d" % (hop, phase, fed, done, pull))
    p0 = phase + done
    return StreamFrames(steps=max(0, (fed - lin) * hop - p0), current=p0 // hop,
                        reads=(p0 + pull - 1) // hop - p0 // hop + 1 + lin if pull else 0,
                        min_ring=(pull - 1 + hop - 1) // hop + 1 + lin if pull else 0)


def _ragged_lengths(n_samples, uniforms):
    """``generate_batch``'s sequence form: (lengths, one 1-D float64 array of uniforms per utterance), every check made and
    every message naming the first offending utterance."""
    if np.ndim(n_samples) != 1:
        raise Exception("generate_batch: n_samples must be an int or a sequence of one positive int per utterance")
    ns = list(n_samples)
    if isinstance(uniforms, np.ndarray) or isinstance(uniforms, torch.Tensor):
        rows = np.asarray(uniforms.cpu() if isinstance(uniforms, torch.Tensor) else uniforms, dtype=np.float64)
        if rows.ndim != 2:
            raise Exception("generate_batch: uniforms must be an (N, >= max(n_samples)) array or a list of N 1-D arrays")
        rows = list(rows)
    else:
        rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in uniforms]
    N = len(rows)
    if len(ns) != N:
        raise Exception("generate_batch: n_samples holds %d lengths for %d utterances (utterance %d has %s)"
                        % (len(ns), N, min(len(ns), N), "no length" if len(ns) < N else "no uniforms"))
    for i, v in enumerate(ns):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise Exception("generate_batch: n_samples of utterance %d must be a positive integer, got %r" % (i, v))
    ns = [int(v) for v in ns]
    for i in range(N):
        if rows[i].size < ns[i]:
            raise Exception("generate_batch: utterance %d has %d uniforms for its %d samples: one per emitted sample"
                            % (i, rows[i].size, ns[i]))
    return ns, [np.ascontiguousarray(rows[i][:ns[i]]) for i in range(N)]


def silence_window(params_or_Q, width):
    """``width`` tokens of silence, what a generation starts from (generate.py:21); ``params_or_Q``: the params or their
    ``quantization_steps``."""
    Q = params_or_Q if isinstance(params_or_Q, (int, np.integer)) else params_or_Q.quantization_steps
    return np.full((width,), 127 if Q > 127 else Q // 2, dtype=np.int32)


class _Handle(object):
    """A decoder handle of the library and what the host knows about it: whether the weights changed since it was packed
    (``stale``; a handle that holds a step limit stays stale, so that the next call takes the limit off), the class whose
    folded gate biases it holds, whether it holds a frame table, and its form ``(chosen, forced)`` -- ``chosen``: created with
    ``WN_DECODER_TRACE_CHOSEN``, its probability trace is one float per step; ``forced``: created with
    ``WN_DECODER_FORCED_TOKENS``, its runs read the token buffer before they write it."""

    def __init__(self):
        self.h, self.stale, self.class_id, self.has_table, self.chosen, self.forced = None, True, None, False, False, False

    @property
    def form(self):
        return (self.chosen, self.forced)

    def bring(self, net, class_id, cond_of, table=None, step_limit=None, chosen=False, forced=False):
        """Create the handle, or update it when it is stale, holds another class, or is given a table or a limit (the
        update is the library's one way to set either and to start their step count again; it also re-packs the weights);
        otherwise nothing.  ``cond_of(class_id)``: the class's folded biases, asked for only when they are packed.
        ``chosen`` / ``forced``: the form asked for; a handle of another form is destroyed and created anew (a handle's form
        is fixed at create)."""
        if self.h is not None and self.form != (bool(chosen), bool(forced)):
            self.destroy()
            self.stale, self.class_id, self.has_table = True, None, False
        if self.h is not None and not (self.stale or self.class_id != class_id or table is not None or step_limit is not None):
            return
        d, keep = net._desc(cond_of(class_id), table, step_limit or 0, chosen, forced=forced)
        self.chosen, self.forced = bool(chosen), bool(forced)
        if self.h is None:
            h = C.c_void_p()
            check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), stream_ptr()), "wn_decoder_create")
            self.h = h
        else:
            check(_lib.lib().wn_decoder_update_weights(self.h, C.byref(d), stream_ptr()), "wn_decoder_update_weights")
        self.stale, self.class_id, self.has_table = bool(step_limit), class_id, self.has_table or table is not None

    def destroy(self):
        if self.h is not None:
            _lib.lib().wn_decoder_destroy(self.h)
            self.h = None


# one utterance of a generate_batch call: its length, uniforms, controls, class id, features as the caller gave them and their
# phase, its window, and ``group`` -- (index of the distinct window, class, index of the distinct feature array by identity,
# phase): utterances of one group share a prefill
# ``forced``: its given samples (int32, -1: draw; ``sampling.check_forced``'s answer), or None
_Utterance = collections.namedtuple("_Utterance", "n u temperature top_k top_p class_id local phase window group forced")
_Utterance.__new__.__defaults__ = (None,)


class FasterWaveNet(WaveNet):
    fast_head_activation = "elu"       # faster_wavenet.py:108 (the normal head is ReLU, wavenet.py:588)
    batch_longest_first = True         # generate_batch: a launch's handles longest first (deal_launches; False: caller's order)
    batch_tile = 0                     # generate_batch / open_stream without tile=: 0 (off), 2, 4, 8, 16 or "auto" (pick_tile)

    def __init__(self, params, compat_zero_prefix: bool = True, seed: Optional[int] = None, storage: str = "fp32",
                 condition_classes: int = 0, condition_channels: int = 0, local_channels: int = 0, local_hop: int = 0,
                 local_interp: str = "repeat", local_upsample: int = 1):
        self._dec = _Handle()              # the batch-1 handle
        self._handles = []                 # generate_batch's handles (one per utterance), created on demand
        self._trace_chosen = False         # the form of the batch-1 handle: generate(..., return_chosen=True) alone sets it
        self._forced = False               # ... and generate(..., forced=...)
        self.prev_causal_outputs = None
        self.prev_residual_outputs = None
        self.keep_window = True            # keep the logits of the whole window on the device: _forward_one_step's reference shape
        self._hist = None                  # (W, Q) ring of ELU-head logits, oldest column at _hist_pos
        self._hist_pos = 0
        super().__init__(params, compat_zero_prefix=compat_zero_prefix, seed=seed, storage=storage,
                         condition_classes=condition_classes, condition_channels=condition_channels,
                         local_channels=local_channels, local_hop=local_hop, local_interp=local_interp,
                         local_upsample=local_upsample)

    def close(self):
        """Destroy every decoder handle (under the library that is loaded now) and forget them."""
        for h in [self._dec] + self._handles:
            h.destroy()
        self._dec, self._handles = _Handle(), []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def _batch_decs(self):
        """generate_batch's raw handles, in creation order."""
        return [h.h for h in self._handles]

    def _weights_changed(self):
        super()._weights_changed()
        for h in [self._dec] + self._handles:
            h.stale = True

    @contextlib.contextmanager
    def _fp32_storage(self):
        """The decoder state and the first row come from fp32 activations, whatever the model's storage."""
        storage, self.storage = self.storage, "fp32"
        try:
            yield
        finally:
            self.storage = storage

    # -- decoder handle -------------------------------------------------------------------------
    def _desc(self, cond=None, table=None, step_limit=0, chosen=False, forced=False, ring=False):
        """``ring``: ``WN_DECODER_FRAME_RING`` -- ``table``'s rows are a ring the handle reads in place and the caller keeps
        refilling (``open_stream``), not a table it copies; it selects no other decoder.
        ``forced``: ``WN_DECODER_FORCED_TOKENS`` -- a run of the handle reads its token buffer before it writes it and emits
        the tokens it finds there instead of drawing (``forced=`` of ``generate``); it selects no other decoder.
        ``chosen``: ``WN_DECODER_TRACE_CHOSEN`` -- the handle's probability trace is the probability of each token it emits,
        one float per step (``return_chosen``); it selects no other decoder and changes no token.
        ``step_limit``: ``WnDecoderDesc.step_limit`` -- a handle of a ragged ``generate_batch`` call ends after its own
        utterance's steps (0: no limit).
        ``table``: (rows (n, sum 2 cd) float32 on the device, hop, phase) -- a locally conditioned model's handle copies one
        utterance's frame table (``WnDecoderDesc.frame_bias``) at create / update time and counts its steps from there.
        ``cond``: [(bf, bg)] per residual layer (``condition_biases``) -- a globally conditioned model's handle holds ONE
        class's folded gate biases, copied like any bias at create / update time.
        A conditioned model (either kind) sets ``WN_DECODER_GATE_ROWS``: on config 4's shape its handles are then the
        specialised decoder's -- wave 1 of the chain workgroup adds the biases and the table rows -- and on every other
        shape the flag changes nothing.  An ordinary model with bias tensors sets no flag and keeps the any-shape decoder."""
        p = self.params
        L = self._flat_layers
        keep = dict(
            causal_ch=int_array(p.causal_conv_channels), cd=int_array(p.residual_conv_channels),
            head_ch=int_array(p.softmax_conv_channels),
            causal_W=ptr_array([l.W for l in self.causal_conv_layers]),
            causal_b=ptr_array([l.b for l in self.causal_conv_layers]),
            Wf=ptr_array([l.wf.W for l in L]), bf=ptr_array([l.wf.b for l in L]),
            Wg=ptr_array([l.wg.W for l in L]), bg=ptr_array([l.wg.b for l in L]),
            Wp=ptr_array([l.projection_block.W for l in L]), bp=ptr_array([l.projection_block.b for l in L]),
            Ws=ptr_array([l.projection_softmax.W for l in L]), bs=ptr_array([l.projection_softmax.b for l in L]),
            head_W=ptr_array([l.W for l in self.softmax_conv_layers]),
            head_b=ptr_array([l.b for l in self.softmax_conv_layers]))
        if cond is not None:
            keep.update(bf=ptr_array([b[0] for b in cond]), bg=ptr_array([b[1] for b in cond]), cond=cond)
        d = _lib.WnDecoderDesc()
        d.Q, d.fw_causal, d.n_causal = p.quantization_steps, p.causal_conv_filter_width, len(p.causal_conv_channels)
        d.fw, d.n_blocks, d.n_layers = p.residual_conv_filter_width, p.residual_num_blocks, len(p.residual_conv_channels)
        d.Cr, d.Cs, d.n_head = self._Cr, self._Cs, len(self.softmax_conv_layers)
        d.causal_channels, d.cd, d.head_channels = keep["causal_ch"], keep["cd"], keep["head_ch"]
        for k in ("causal_W", "causal_b", "Wf", "bf", "Wg", "bg", "Wp", "bp", "Ws", "bs", "head_W", "head_b"):
            setattr(d, k, C.cast(keep[k], C.POINTER(C.c_void_p)))
        d.head_act = ACT[self.fast_head_activation]
        d.flags = _lib.default_exec_flags() if self.exec_flags is None else int(self.exec_flags)
        if self.condition_classes or self.local_channels:
            d.flags |= _lib.WN_DECODER_GATE_ROWS
        if chosen:
            d.flags |= _lib.WN_DECODER_TRACE_CHOSEN
        if forced:
            d.flags |= _lib.WN_DECODER_FORCED_TOKENS
        if ring:
            d.flags |= _lib.WN_DECODER_FRAME_RING
        d.step_limit = int(step_limit)
        if table is not None:
            rows, hop, phase = table
            keep["table"] = rows
            d.frame_bias, d.n_frames, d.frame_stride = rows.data_ptr(), int(rows.shape[0]), int(rows.shape[1])
            d.frame_hop, d.frame_phase = int(hop), int(phase)
            d.frame_interp = 1 if self.local_interp == "linear" else 0
        return d, keep

    # -- local conditioning: one utterance's features -> what the prefill and the decoder handle take ------------------------
    def _utterance_local(self, local, local_phase, W, n_samples, what="generate"):
        """``local=`` (F, n) of one utterance, covering it from its first sample (prompt included), ``local_phase`` the
        position of that sample inside column 0 -> (features (1, F, n) on the device, phase) or (None, 0).  Raises when the
        features do not cover the W prompt positions and the n_samples - 1 decoded ones -- before anything runs."""
        if not self.local_channels:
            self._local_features(local, 1, W, local_phase)                    # raises when features were given
            return None, 0
        if local is not None and not isinstance(local, torch.Tensor):
            local = np.asarray(local, dtype=np.float32)
        if local is not None and len(local.shape) == 2:
            local = local[None]
        total = W + max(int(n_samples) - 1, 0)
        try:
            return self._local_features(local, 1, total, local_phase)
        except Exception as e:
            if local is None or "feature columns" not in str(e):
                raise
            raise Exception("%s: the features cover fewer samples than asked for (%d prompt + %d generated): %s"
                            % (what, W, max(int(n_samples) - 1, 0), e))

    def _decoder_table(self, feats, phase, W):
        """The decoder's table after a prefill over W positions: the step that consumes the sample at absolute position
        p = phase + W + k reads column p // hop, so the handle gets the rows from column (phase + W) // hop on and the phase
        (phase + W) % hop.  With linear interpolation a step also reads the column after its own; the rows go on to the last
        column given, so the one after the last that is needed is there (``_utterance_local`` has checked it).  With a learned
        upsampling layer (``local_upsample`` > 1) the utterance's features go through it once, ``hop`` is the fine hop
        H' = local_hop / local_upsample and the table holds the fine columns' rows: the decoders run at hop H'."""
        hop = self.local_fine_hop
        col, ph = divmod(int(phase) + int(W), hop)
        rows = self.local_biases(feats[0], phase)
        col = min(col, int(rows.shape[0]) - 1)            # (n_samples == 1: nothing is decoded, any row will do)
        return rows[col:].contiguous(), hop, ph

    def _class_id(self, condition):
        """``condition=`` of the batch-1 methods (an id, or a sequence holding one) -> int, or None for an unconditioned model."""
        if condition is not None and np.ndim(condition) > 0:
            c = np.asarray(condition).reshape(-1)
            if c.size != 1:
                raise Exception("one utterance takes ONE class id, got %d" % c.size)
            condition = c[0]
        ids = self._condition_ids(None if condition is None else [int(condition)], 1)
        return None if ids is None else int(condition)

    def _decoder(self, class_id=None, table=None):
        """The batch-1 handle; for a conditioned model holding ``class_id``'s biases (default: the class it holds already); for
        a locally conditioned one ``table`` (``_decoder_table``) is copied into it and its step count starts again (default:
        the table it holds, continued)."""
        dec = self._dec
        if self.local_channels and table is None and not dec.has_table:
            raise Exception("this model is locally conditioned: prefill with local= first")
        if self.condition_classes and class_id is None:
            class_id = dec.class_id
            if class_id is None:
                raise Exception("this model is globally conditioned: prefill with condition= first")
        if self.local_channels and table is None and dec.stale:
            raise Exception("the weights changed since the last prefill: prefill with local= again")
        if dec.h is not None and dec.form != (self._trace_chosen, self._forced) and self.local_channels and table is None:
            raise Exception("the batch-1 handle changes its form (return_chosen / forced): prefill with local= again")
        dec.bring(self, class_id, self.condition_biases if self.condition_classes else lambda c: None, table,
                  chosen=self._trace_chosen, forced=self._forced)
        return dec.h

    # -- the reference's face -------------------------------------------------------------------
    def forward_one_step(self, x_batch, apply_softmax=True, as_numpy=False, condition=None, local=None, local_phase=0):
        """Full forward over the window that also seeds the decoder state (faster_wavenet.py:13-47).  ``condition``: the
        utterance's class id (globally conditioned models): the prefill runs the ordinary forward with it and the decoder
        handle is created or updated with that class's folded biases.  ``local`` / ``local_phase`` (locally conditioned
        models): the utterance's features (F, n) from the window's first sample on -- as many columns as the steps that follow
        will read -- and the position of that sample inside column 0; the prefill runs the ordinary forward over the window
        with them, and the handle receives the table of the columns behind the window (``local_alignment``'s rule)."""
        x = self.to_variable(x_batch)
        _need_gpu(x)
        if x.shape[0] != 1:
            raise Exception("FasterWaveNet generates one utterance at a time (batch 1), like the reference")
        class_id = self._class_id(condition)
        feats, phase = self._utterance_local(local, local_phase, int(x.shape[1] if x.dim() == 2 else x.shape[3]), 1, "forward_one_step")
        with self._fp32_storage():
            return self._prefill(x, apply_softmax, as_numpy, class_id, feats, phase)

    def _seed(self, tok, class_id, feats, phase, handles, apply_softmax=True):
        """The one prefill: the forward over a window (tokens or one-hot, batch 1) at fp32 storage -- causal block, residual
        block, head -- and the state of every handle in ``handles`` (raw ones; or a function giving them, called after the
        forward) loaded from it.  -> (the head's output over the window, the skip sum)."""
        with self._fp32_storage(), torch.no_grad():
            causal_output = self.forward_causal_block(tok)
            _, sum_skip = self.forward_residual_block(causal_output, condition=None if class_id is None else [class_id],
                                                      local=feats, local_phase=phase)
            p0 = self.forward_softmax_block(sum_skip, apply_softmax=apply_softmax)
        tokens = (tok if not tok.is_floating_point() else tok[:, :, 0, :].argmax(dim=1)).to(torch.int32).contiguous()
        handles = handles() if callable(handles) else handles
        if handles:
            causal_outs = ptr_array([t.contiguous() for t in self._last_causal_outputs])
            layer_ins = ptr_array(self._last_layer_inputs)
            for h in handles:
                check(_lib.lib().wn_decoder_load_state(h, ptr(tokens), tokens.shape[1], causal_outs, layer_ins, stream_ptr()),
                      "wn_decoder_load_state")
        return p0, sum_skip

    def _prefill(self, x, apply_softmax, as_numpy, class_id=None, feats=None, phase=0):
        W = int(x.shape[1] if x.dim() == 2 else x.shape[3])
        # (the batch-1 handle is created or updated behind the forward: a function)
        out, sum_skip = self._seed(x, class_id, feats, phase, lambda: [
            self._decoder(class_id, None if feats is None else self._decoder_table(feats, phase, W))], apply_softmax)
        self._last_sum_skip = sum_skip                                           # generate(): the first row under a temperature
        self._hist = None
        if self.keep_window:
            # the reference's next step re-evaluates EVERY cached column with the fast path's ELU head
            # (faster_wavenet.py:100-112): the window's logits under that head, once, from the skip sum just computed
            with torch.no_grad():
                lg = self.forward_softmax_block(sum_skip, apply_softmax=False, activation=self.fast_head_activation)
            self._hist = lg[0, :, 0, :].t().contiguous()                     # (W, Q), column 0 = oldest
            self._hist_pos = 0
        self.prev_causal_outputs = _RingState("causal")
        self.prev_residual_outputs = _RingState("residual")
        return self.to_numpy(out) if as_numpy else out

    def _forward_one_step(self, x_batch_data, apply_softmax=True, as_numpy=False, full_window=None):
        """One incremental step (faster_wavenet.py:50-63); falls back to the full forward when the
        state was reset by ``prev_causal_outputs = None``.  Returns the reference's ``(1, Q, 1, W)`` -- every column of the
        rolled window under the ELU head, the newest last (faster_wavenet.py:105-113; one concatenation + one softmax over W
        rows per call) -- unless ``full_window=False`` (or ``keep_window`` was False at the prefill): then the newest
        column only, ``(1, Q, 1, 1)``; ``[0, :, 0, -1]`` reads the same values from either."""
        if full_window is None:
            full_window = bool(self.keep_window)
        if full_window and not self.keep_window:
            raise Exception("full_window=True needs keep_window = True before the first (prefill) call")
        if getattr(self, "prev_causal_outputs", None) is None:
            return self.forward_one_step(x_batch_data, apply_softmax=apply_softmax, as_numpy=as_numpy)
        if isinstance(x_batch_data, (int, np.integer)):
            token = int(x_batch_data)
        else:
            x = x_batch_data
            if isinstance(x, np.ndarray):
                token = int(x[0, -1]) if x.ndim == 2 else int(np.argmax(x[0, :, 0, -1]))
            else:
                token = int(x[0, -1]) if x.dim() == 2 else int(x[0, :, 0, -1].argmax())
        Q = self.params.quantization_steps
        lib = _lib.lib()
        prob = torch.empty((1, 1, Q), device=self.device, dtype=torch.float32)
        if self._hist is None:
            if full_window:
                raise Exception("the window history was dropped (generate() advanced the decoder on the device, or keep_window "
                                "was False at the prefill): pass full_window=False for the newest column, or set "
                                "prev_causal_outputs = None and prefill again")
            check(lib.wn_decoder_step(self._decoder(), token, ptr(prob), 1 if apply_softmax else 0, stream_ptr()),
                  "wn_decoder_step")
            out = _as_view(prob)
            return self.to_numpy(out) if as_numpy else out
        # window history: the step leaves its logits in the ring slot of the column that drops out of the window
        W = self._hist.shape[0]
        slot = self._hist[self._hist_pos]
        check(lib.wn_decoder_step(self._decoder(), token, ptr(slot), 0, stream_ptr()), "wn_decoder_step")
        self._hist_pos = (self._hist_pos + 1) % W
        if not full_window:
            if apply_softmax:
                check(lib.wn_softmax_fwd(ptr(slot), ptr(prob), 1, Q, stream_ptr()), "wn_softmax_fwd")
            else:
                prob.view(-1).copy_(slot)
            out = _as_view(prob)
            return self.to_numpy(out) if as_numpy else out
        win = torch.cat((self._hist[self._hist_pos:], self._hist[:self._hist_pos]), dim=0)      # oldest ... newest
        if apply_softmax:
            res = torch.empty_like(win)
            check(lib.wn_softmax_fwd(ptr(win), ptr(res), W, Q, stream_ptr()), "wn_softmax_fwd")
            win = res
        out = _as_view(win.view(1, W, Q))
        return self.to_numpy(out) if as_numpy else out

    # -- the whole generate loop on the device (train_audio/generate.py:9-60 with --fast) --------
    def _first_row(self, sum_skip, p0, temperature):
        """(1, Q) probabilities of the first emitted sample (full forward, ReLU head).  Temperature 1: the newest column of
        the window's softmax ``p0``, as ever; otherwise the same contract as on the device -- the fp32 logits of that
        column times ``1.0f / temperature``, then ``wn_softmax_fwd``."""
        Q = self.params.quantization_steps
        if float(temperature) == 1.0:
            return p0[0, :, 0, -1].contiguous().view(1, Q)
        with self._fp32_storage(), torch.no_grad():
            lg = self.forward_softmax_block(sum_skip, apply_softmax=False)
        row = (lg[0, :, 0, -1].contiguous().view(1, Q) * float(sampling.inv_temperature(temperature))).contiguous()
        out = torch.empty_like(row)
        check(_lib.lib().wn_softmax_fwd(ptr(row), ptr(out), 1, Q, stream_ptr()), "wn_softmax_fwd")
        return out

    def generate(self, n_samples: int, uniforms, initial_tokens=None, return_probs: bool = False,
                 temperature=1.0, top_k=0, top_p=1.0, condition=None, local=None, local_phase=0, return_chosen: bool = False,
                 forced=None):
        """Emit ``n_samples`` tokens.  Step 1 is the full forward over the initial window (ReLU head,
        like the reference's first ``_forward_one_step`` call); steps 2.. run inside one persistent
        kernel with the ELU head.  ``uniforms[i]`` is the float64 draw numpy's ``choice`` would make
        at step i (``RandomState.random_sample``).

        ``temperature`` / ``top_k`` / ``top_p`` (off at 1 / 0 / 1; the rule is wavenet_amd/sampling.py's) act on every
        draw, on the device; ``return_probs`` then holds the post-temperature, pre-truncation rows.  With all three off the
        run is the one it was before they existed, bit for bit.

        ``condition``: the class id (speaker) of a globally conditioned model.  Tokens and probabilities are those of an
        ordinary biased model holding ``condition_biases(condition)``, bit for bit.

        ``local`` (locally conditioned models): the utterance's (F, n) features from its first sample on, prompt included;
        ``local_phase``: where that sample lies inside column 0.  Generating more samples than the features cover raises
        before anything runs.

        ``return_chosen``: also return ``chosen``, (n_samples,) float32 on the device -- the probability the model gave each
        token it emitted, ``chosen[i] == probs[i, tokens[i]]`` of a ``return_probs`` run bit for bit (element 0 from the
        prefill row the first draw consumed, the rest written by the decoder, one float per step:
        ``WN_DECODER_TRACE_CHOSEN``).  ``sampling.chosen_nll(chosen)`` is the utterance's nats per sample.  The tokens are
        those of a run without it.  Returns ``(tokens, chosen)``; with ``return_probs`` as well ``(tokens, probs, chosen)``,
        on the full-row handle, ``chosen`` gathered from ``probs``.

        ``forced``: a 1-D integer array of ``n_samples`` entries -- sample i is emitted as given where ``forced[i]`` is a token
        of ``[0, Q)`` and drawn where it is -1 (``sampling.check_forced``; anything else raises before any device work).  A
        given sample enters the next step as a drawn one does; its uniform is not looked at; a drawn sample is drawn exactly as
        without ``forced``.  ``probs`` rows are the post-temperature, pre-truncation rows as ever, and ``chosen[i]`` of a given
        sample is ``probs[i, forced[i]]``: with every sample given, ``sampling.chosen_nll(chosen)`` is the decoder's own
        likelihood of that audio.  Element 0 is the prefill's.  The handle is a ``WN_DECODER_FORCED_TOKENS`` one, created
        anew when the last call's was not; ``forced=None`` is every call as it was."""
        Q = self.params.quantization_steps
        class_id = self._class_id(condition)
        if forced is not None:
            forced = sampling.check_forced(forced, n_samples, Q)
        self._trace_chosen = bool(return_chosen) and not return_probs
        self._forced = forced is not None
        sampling.check_controls(temperature, top_k, top_p)
        top_k, top_p = int(top_k), float(top_p)
        if initial_tokens is None:
            initial_tokens = silence_window(Q, self.input_width)
        tok = torch.as_tensor(np.asarray(initial_tokens, dtype=np.int32).reshape(1, -1)).to(self.device)
        u = torch.as_tensor(np.asarray(uniforms, dtype=np.float64)).to(self.device)
        if u.numel() < n_samples:
            raise Exception("need one uniform per emitted sample")
        feats, phase = self._utterance_local(local, local_phase, int(tok.shape[1]), n_samples)
        lib = _lib.lib()
        self.prev_causal_outputs = None
        keep, self.keep_window = self.keep_window, False             # the run below never builds the window (and drops it)
        try:
            p0 = self.forward_one_step(tok, apply_softmax=True, condition=class_id, local=None if feats is None else feats[0],
                                       local_phase=phase)      # (1,Q,1,W)
        finally:
            self.keep_window = keep
        first_prob = self._first_row(self._last_sum_skip, p0, temperature)
        # (given samples: the token buffer holds them before the run, element 0 -- the prefill's -- included)
        out = torch.empty((n_samples,), device=self.device, dtype=torch.int32) if forced is None else torch.as_tensor(forced).to(self.device)
        if forced is None or forced[0] < 0:
            check(lib.wn_sample_categorical_filtered(ptr(first_prob), ptr(u), ptr(out), 1, Q, top_k, top_p, stream_ptr()),
                  "wn_sample_categorical_filtered")
        probs = torch.empty((n_samples, Q), device=self.device, dtype=torch.float32) if return_probs else None
        if return_probs:
            probs[0] = first_prob[0]
        chosen = torch.empty((n_samples,), device=self.device, dtype=torch.float32) if self._trace_chosen else None
        if chosen is not None:
            chosen[:1] = first_prob[0].gather(0, out[:1].long())
        if n_samples > 1:
            first = int(out[0].item())
            check(lib.wn_decoder_set_sampling(self._decoder(), float(temperature), top_k, top_p), "wn_decoder_set_sampling")
            check(lib.wn_decoder_run(self._decoder(), first, ptr(u[1:]), n_samples - 1, ptr(out[1:]),
                                     ptr(probs[1:]) if return_probs else ptr(chosen[1:]) if chosen is not None else None,
                                     stream_ptr()), "wn_decoder_run")
            # the nine-workgroup run reports a wait that gave up (workgroups not all resident) instead of trapping: its
            # tokens would be void.  One 8-byte read-back; generate() hands tokens to the host anyway.
            check(lib.wn_decoder_status(self._decoder(), stream_ptr()), "wn_decoder_status")
            # the decoder advanced n_samples - 1 steps on the device (its rings are current: step-by-step decoding may go
            # on from here), but the host-side window history -- what _forward_one_step(..., full_window=True) returns
            # the older columns from -- still holds the prefill state: drop it rather than answer with a stale window
            self._hist = None
        if return_chosen and return_probs:
            chosen = probs.gather(1, out.long()[:, None])[:, 0].contiguous()
        res = (out,) + ((probs,) if return_probs else ()) + ((chosen,) if return_chosen else ())
        return res if len(res) > 1 else out

    # -- N utterances at once (new capability: the reference generates one utterance per process) ------------------------
    def _nine_workgroup_shape(self, flags) -> bool:
        """Whether ``wn_decoder_create`` gives this model the specialised decoder (csrc/decoder.hip ``fast_shape``: BASELINE
        config 4's shape with the reference's default biases; global and local conditioning do not change the answer, their
        handles carry ``WN_DECODER_GATE_ROWS``).  Only a forecast -- it picks the batch limit and the
        ``n_samples == 2`` rule before any work; the library decides, and refuses a launch it does not take."""
        p = self.params
        L = self._flat_layers
        return (not (flags & _lib.WN_EXEC_FORCE_GENERIC) and p.quantization_steps == 256 and
                len(p.causal_conv_channels) == 1 and p.causal_conv_filter_width == 2 and p.residual_conv_filter_width == 2 and
                self._Cr == 32 and self._Cs == 256 and list(p.softmax_conv_channels) == [256, 256] and len(L) <= 128 and
                all(int(c) == 32 for c in p.residual_conv_channels) and self.causal_conv_layers[0].bshape is None and
                all(k.bshape is None for l in L for k in (l.wf, l.wg, l.projection_block, l.projection_softmax)))

    def _launch_tile(self, tile, n_launch_utterances, nine):
        """``same_weights`` of one any-shape launch from a checked ``tile`` (``check_tile``), or None where tiles do not apply --
        config 4's shape, ``WAVENET_HIP_BATCH_OWN_WEIGHTS=1``, a single utterance, tile off -- and the call passes what it
        always passed."""
        if nine or not tile or n_launch_utterances < 2 or os.environ.get("WAVENET_HIP_BATCH_OWN_WEIGHTS") == "1":
            return None
        if tile == "auto":
            n_cu = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
            tile = pick_tile(n_launch_utterances, n_cu, tile_fit(self.params))
        return tile or None

    def _batch_prompts(self, initial_tokens, N):
        """``generate_batch``'s ``initial_tokens`` -> (the distinct windows, 1-D int32 each; the window index of every
        utterance).  Raises on anything but None, one 1-D window or an (N, W) integer array."""
        Q = self.params.quantization_steps
        if initial_tokens is None:
            return [silence_window(Q, self.input_width)], [0] * N
        try:
            a = np.asarray(initial_tokens)
        except ValueError:
            a = None                                                   # a ragged list
        if a is None or a.dtype == object or a.ndim not in (1, 2) or a.size == 0:
            raise Exception("generate_batch: initial_tokens must be None, one 1-D window, or an (N, W) integer array")
        if a.ndim == 2 and a.dtype.kind not in "iu":
            raise Exception("generate_batch: an (N, W) initial_tokens must hold integer tokens, got %s" % a.dtype)
        if a.ndim == 2 and a.shape[0] != N:
            raise Exception("generate_batch: initial_tokens has %d rows for %d utterances" % (a.shape[0], N))
        a = np.ascontiguousarray(a.astype(np.int32))
        if int(a.min()) < 0 or int(a.max()) >= Q:
            raise Exception("generate_batch: initial_tokens outside [0, %d)" % Q)
        if a.ndim == 1:
            return [a], [0] * N
        seen, prompts, which = {}, [], []
        for row in a:                                                  # equal rows share one prefill
            k = row.tobytes()
            if k not in seen:
                seen[k] = len(prompts)
                prompts.append(row)
            which.append(seen[k])
        return prompts, which

    def generate_batch(self, n_samples, uniforms, initial_tokens=None, temperature=1.0, top_k=0, top_p=1.0,
                       condition=None, local=None, local_phase=0, return_chosen: bool = False, forced=None, tile=None):
        """N independent utterances at once.  ``n_samples`` an int: ``uniforms`` is (N, >= n_samples) float64, utterance u draws
        with ``uniforms[u]``, and (N, n_samples) int32 tokens on the device come back.  ``n_samples`` a sequence of N positive
        ints -- a length per utterance: ``uniforms`` is an (N, >= max) array or a list of N 1-D arrays, and a LIST of N 1-D int32
        device tensors comes back, tensor u of length ``n_samples[u]``.  Either way row u equals ``generate(<u's length>,
        <u's uniforms>, initial_tokens=<u's window>, <u's controls, class, features, phase>)`` bit for bit.

        ``initial_tokens``: None (silence), one 1-D window for every utterance, or an (N, W) integer array -- a prompt per
        utterance.  ``temperature`` / ``top_k`` / ``top_p``: as for ``generate``, each a scalar or one value per utterance.
        ``condition`` (globally conditioned models): one class id for all utterances or one each -- a voice per utterance.
        ``local`` / ``local_phase`` (locally conditioned models): one (F, n) array for all utterances or a list of one per
        utterance, each covering its utterance from its first sample on, prompt included; the phases likewise.  Whatever is
        wrong with the arguments -- the features not covering an utterance's own length included -- raises before any device
        work; with a length per utterance the message names the first such utterance.

        A single utterance is a strict sample-to-sample chain (generate.py:9-60, batch 1: wavenet.py:286,290,354); the
        batched launch (``wn_decoder_run_batch``) runs such chains side by side, each with a decoder handle of its own: nine
        workgroups per utterance and up to ``wn_decoder_batch_max()`` = 28 utterances per launch for config 4's shape, one
        workgroup per utterance and up to ``WN_DECODER_BATCH_MAX_ANY`` for every other model (any channels, filter widths,
        causal layers, Q; ``WN_EXEC_FORCE_GENERIC``; ``storage="bf16"``).  A conditioned model of config 4's shape is on the
        nine-workgroup form too: a class, a table and a phase per utterance, all reading one copy of the weights.
        More utterances run as several launches, one after another, dealt
        longest first (``deal_launches``): a launch's step count is its longest utterance's, and with a length per utterance
        every handle carries ``step_limit`` = its own ``n_samples[u] - 1`` and its workgroups end there.  An utterance of
        length 1 decodes nothing and joins no launch.  Step 1 -- the full forward over the window, at batch 1 exactly as
        ``generate`` runs it -- runs once per distinct (window, class, features, phase).  What still runs as a loop over
        ``generate()``: ``WN_DECODER_ONE_WORKGROUP``, any utterance of length 2 on the nine-workgroup form, and a device the
        nine-workgroup launch does not fit.

        ``return_chosen``: ``(tokens, chosen)`` comes back, ``chosen`` float32 on the device in the shape of the tokens --
        (N, n_samples), or a list of N 1-D tensors -- row u the probabilities ``generate(..., return_chosen=True)`` gives for
        utterance u, bit for bit.  The handles of such a call are ``WN_DECODER_TRACE_CHOSEN`` ones (a trace of one float per
        step and utterance, not a row of Q); handles of the other form are created anew, and a launch never mixes the two.

        ``forced``: None, one 1-D integer array for all utterances (at least as long as the longest; utterance u takes its first
        ``n_u`` entries), or a list of N entries, each such an array of the utterance's own length or None (= all -1).  Row u is
        ``generate(..., forced=<u's entries>)`` bit for bit, tokens and ``chosen``; the handles of such a call are
        ``WN_DECODER_FORCED_TOKENS`` ones, all of them.

        ``tile``: None (= ``self.batch_tile``, 0 by default), 0 / 1 (off), 2, 4, 8, 16 or ``"auto"`` (``pick_tile`` per launch).  With
        U >= 2 a workgroup of the any-shape decoder takes U utterances of a launch and reads ONE copy of the weights for them
        (``same_weights = U``) -- also when classes, tables, phases, controls, prompts or lengths differ within the call, which
        stay per utterance.  The result is the same, bit for bit.  A U that does not fit the model's LDS (``tile_fit``) raises
        before any device work.  On config 4's shape, under ``WAVENET_HIP_BATCH_OWN_WEIGHTS=1`` and for a single live utterance
        ``tile`` changes nothing."""
        tile = check_tile(self.batch_tile if tile is None else tile, self.params)
        ragged = not isinstance(n_samples, (int, np.integer))
        recs, feats = self._batch_plan(n_samples, uniforms, initial_tokens, temperature, top_k, top_p, condition, local, local_phase,
                                       forced)
        given = forced is not None                                 # the form of every handle of the call
        N, Q, lib = len(recs), self.params.quantization_steps, _lib.lib()
        # what the batched launch does not cover runs as a loop over generate() -- same tokens, one utterance at a time --
        # decided BEFORE any work is done
        flags = _lib.default_exec_flags() if self.exec_flags is None else int(self.exec_flags)
        nine = self._nine_workgroup_shape(flags)
        if nine and (any(r.n == 2 for r in recs) or flags & _lib.WN_DECODER_ONE_WORKGROUP):
            return self._generate_batch_loop(recs, ragged, return_chosen)
        # given samples: the token buffers hold them before the launch (an utterance without any: -1 throughout)
        held = [r.forced if r.forced is not None else np.full((r.n,), -1, np.int32) for r in recs] if given else None
        limit = int(lib.wn_decoder_batch_max()) if nine else _lib.WN_DECODER_BATCH_MAX_ANY
        live = [i for i in range(N) if recs[i].n > 1]                  # the utterances that decode at all
        # a result is a 1-D tensor per utterance, its uniforms likewise: rows of one (N, n) tensor and of one upload for
        # equal lengths, tensors and uploads of their own otherwise.  (Every upload here, ahead of the device work: one
        # behind the prefills would have the host wait for them.)
        if ragged:
            u_dev = [torch.as_tensor(r.u).to(self.device) for r in recs]
            u0 = torch.as_tensor(np.array([r.u[0] for r in recs], dtype=np.float64)).to(self.device)
            res = [torch.empty((r.n,), device=self.device, dtype=torch.int32) if not given else
                   torch.as_tensor(held[i]).to(self.device) for i, r in enumerate(recs)]
            ch = [torch.empty((r.n,), device=self.device, dtype=torch.float32) for r in recs] if return_chosen else None
        else:
            u = torch.as_tensor(np.stack([r.u for r in recs])).to(self.device)
            u_dev, u0 = list(u), u[:, 0].contiguous()
            out = torch.empty((N, recs[0].n), device=self.device, dtype=torch.int32) if not given else \
                torch.as_tensor(np.stack(held)).to(self.device)
            res = list(out)
            ch_all = torch.empty((N, recs[0].n), device=self.device, dtype=torch.float32) if return_chosen else None
            ch = list(ch_all) if return_chosen else None
        if live:
            self._batch_handles(recs, feats, ragged, return_chosen, given)
        # one prefill per group, at batch 1 as generate() runs it; the decoder states of its utterances are seeded from it,
        # and its first row (one per distinct temperature) is what generate() draws the first token from
        self.prev_causal_outputs = None
        rows = {}
        for g in sorted({r.group for r in recs}, key=lambda g: (g[0], -1 if g[1] is None else g[1], g[2], g[3])):
            mine = [i for i in range(N) if recs[i].group == g]
            r = recs[mine[0]]
            tok = torch.as_tensor(r.window.reshape(1, -1)).to(self.device)
            p0, sum_skip = self._seed(tok, r.class_id, feats[g][0], r.phase, [self._handles[i].h for i in mine] if live else [])
            for t in sorted({recs[i].temperature for i in mine}):
                rows[g + (t,)] = self._first_row(sum_skip, p0, t)
        first_rows = [rows[r.group + (r.temperature,)] for r in recs]
        first = torch.empty((N,), device=self.device, dtype=torch.int32)
        if all(sampling.controls_off(r.temperature, r.top_k, r.top_p, Q) for r in recs):
            first_prob = torch.cat(first_rows, dim=0).contiguous()
            check(lib.wn_sample_categorical(ptr(first_prob), ptr(u0), ptr(first), N, Q, stream_ptr()), "wn_sample_categorical")
        else:
            for i, r in enumerate(recs):                             # the truncation per utterance, as generate() draws
                check(lib.wn_sample_categorical_filtered(ptr(first_rows[i]), ptr(u0[i:i + 1]), ptr(first[i:i + 1]), 1, Q,
                                                         r.top_k, r.top_p, stream_ptr()), "wn_sample_categorical_filtered")
        if given:                                                    # a given first sample replaces the draw
            f0 = torch.as_tensor(np.array([h[0] for h in held], dtype=np.int32)).to(self.device)
            first = torch.where(f0 >= 0, f0, first)
        if ragged:
            for i in range(N):
                res[i][:1] = first[i:i + 1]
        else:
            out[:, 0] = first                                        # (one copy: a copy per row costs 20 us a row)
        if return_chosen:                                            # element 0: the prefill row the first draw consumed
            ch0 = torch.cat(first_rows, dim=0).gather(1, first.long()[:, None])[:, 0]
            if ragged:
                for i in range(N):
                    ch[i][:1] = ch0[i:i + 1]
            else:
                ch_all[:, 0] = ch0
        if live:
            firsts = [int(v) for v in first.cpu().tolist()]
            # the any-shape kernel writes each utterance's tokens where they belong; the nine-workgroup form keeps its buffers
            outs = [(res[i][1:].clone() if given else torch.empty((r.n - 1,), device=self.device, dtype=torch.int32)) if nine else
                    res[i][1:] for i, r in enumerate(recs)]
            same = 0 if os.environ.get("WAVENET_HIP_BATCH_OWN_WEIGHTS") == "1" else 1      # the handles ARE copies of this model's weights
            # (nine-workgroup form: gate biases and frame tables are not part of the shared weights -- every utterance reads its own)
            if not nine and len({r.class_id for r in recs}) > 1:
                same = 0                                              # ... but hold different classes' biases
            if not nine and self.local_channels and len({r.group[:1] + r.group[2:] for r in recs}) > 1:
                same = 0                                              # ... or different frame tables
            # launches of at most `limit` utterances, one after another; a launch's handles go longest first: on the any-shape
            # form that is roughly the order workgroups are dispatched in when they outnumber what the device holds
            for n_launch, idx in deal_launches([recs[i].n - 1 for i in live], limit, self.batch_longest_first):
                sel = [live[j] for j in idx]
                U = self._launch_tile(tile, len(sel), nine) if len(live) > 1 else None      # a tile size, or None: `same` as ever
                rc = lib.wn_decoder_run_batch((C.c_void_p * len(sel))(*[self._handles[i].h.value for i in sel]), len(sel),
                                              (C.c_int32 * len(sel))(*[firsts[i] for i in sel]), ptr_array([u_dev[i][1:] for i in sel]),
                                              n_launch, ptr_array([outs[i] for i in sel]),
                                              ptr_array([ch[i][1:] for i in sel]) if return_chosen else None,
                                              same if U is None else U, stream_ptr())
                if rc == _lib.WN_ESHAPE and nine:     # refused before any device work: the nine workgroups per utterance do not fit the device
                    return self._generate_batch_loop(recs, ragged, return_chosen)
                check(rc, "wn_decoder_run_batch")
            for i in (live if nine else live[:1]):                    # any-shape: nothing can give up; one synchronise
                check(lib.wn_decoder_status(self._handles[i].h, stream_ptr()), "wn_decoder_status")
            if nine:
                for i in live:
                    res[i][1:] = outs[i]
        if return_chosen:
            return (res, ch) if ragged else (out, ch_all)
        return res if ragged else out

    # -- one long utterance as overlapping segments of ONE batched call (wavenet_amd/fold.py states the rule) -----------------
    def fold_capacity(self, tile=None, utterances=1):
        """The segments per utterance that ``body="auto"`` aims at: what one launch decodes side by side -- ``wn_decoder_batch_max()``
        on config 4's shape, else the device's compute units times the tile size (1 with tiles off) -- divided by
        ``utterances``; at least 1."""
        flags = _lib.default_exec_flags() if self.exec_flags is None else int(self.exec_flags)
        if self._nine_workgroup_shape(flags):
            cap = int(_lib.lib().wn_decoder_batch_max())
        else:
            n_cu = int(torch.cuda.get_device_properties(self.device).multi_processor_count)
            tile = check_tile(self.batch_tile if tile is None else tile, self.params, "generate_folded")
            cap = n_cu * max(1, pick_tile(2 * n_cu, n_cu, tile_fit(self.params)) if tile == "auto" else tile)
        return max(1, cap // max(1, int(utterances)))

    def generate_folded(self, n_samples, uniforms, body, overlap=None, warmup=None, initial_tokens=None, condition=None,
                        local=None, local_phase=0, temperature=1.0, top_k=0, top_p=1.0, return_chosen: bool = False,
                        return_segments: bool = False, tile=None, **other):
        """One long utterance of a locally conditioned model, decoded as overlapping segments side by side and cross-faded:
        ``fold.fold_plan(n_samples, body, overlap, warmup)`` cuts it, every segment is an utterance of ONE ragged
        ``generate_batch`` call, and ``fold.unfold`` joins them -- here on the device, bit for bit.  Returns the (n_samples,)
        int16 signal on the device: the values ``data.save_audio_file`` writes for tokens (``data.pcm_table``), cross-faded inside
        the seams; ``data.save_pcm_file`` writes it.

        ``n_samples`` an int and ``uniforms`` one row of >= n_samples float64: one utterance.  ``n_samples`` a sequence of N
        lengths and ``uniforms`` a list of N rows (or an (N, >= max) array): N utterances, folded in the same call, and lists come
        back.  ``initial_tokens``, ``condition``, ``local`` / ``local_phase`` and the sampling controls are ``generate_batch``'s,
        per utterance; a segment repeats its utterance's speaker and controls.

        ``body``: samples per segment, or ``"auto"`` = ``fold.auto_body(n, fold_capacity(tile, N), overlap, warmup)`` per
        utterance.  ``overlap`` (default ``local_hop`` samples: one feature column) and ``warmup`` (default ``input_width``:
        after that many generated samples no token of the silent window is inside the receptive field) are design defaults,
        not tuned values; ``metrics.copy_synthesis(..., fold=)`` reads what a choice costs on a trained model.

        The contract: segment u's row equals its own ``generate(e_u - s_u, U[s_u:e_u], initial_tokens=<the utterance's window
        where s_u = 0, else silence>, local=<its columns>, local_phase=<its phase>, ...)`` call, tokens and ``chosen``, bit
        for bit (``generate_batch``'s contract; the prefill runs once per segment at batch 1).  The uniforms are keyed by
        position, so segment 0 draws what the sequential chain draws, a plan of one segment (``body >= n_samples``) is
        ``pcm_table[generate(n_samples, uniforms, ...)]``, and both sides of a seam see the same draw at the same position.
        (Segment 0's tokens ARE the chain's first ones where a projected feature row does not depend on the columns projected
        with it -- ``open_stream``'s caveat about ``push``.)

        ``return_chosen``: also the (n_samples,) float32 probability the owning segment gave each position's token.
        ``return_segments``: also ``(plan, token rows, chosen rows)`` -- lists of those for N utterances.
        ``tile``: ``generate_batch``'s.

        Refused before any device work, naming the value: a model without local conditioning (nothing makes segments agree);
        overlap > body, body < 1, warmup < 0; ``forced=`` (given samples are not part of a folded run); features that do not
        cover a segment (the segment and both column counts are named).  Streams, ``--best-of`` and several GPUs are left out."""
        from . import data, fold
        what = "generate_folded"
        if "forced" in other:
            raise ValueError("%s: forced= is not an argument of this method (got %r): given samples would have to be cut and "
                             "joined like drawn ones; use generate / generate_batch" % (what, other["forced"]))
        if other:
            raise TypeError("%s: unexpected argument %s" % (what, ", ".join(sorted(other))))
        if not self.local_channels:
            raise ValueError("%s: this model has no local conditioning (local_channels = 0): nothing makes segments of one "
                             "utterance agree; use generate" % what)
        single = isinstance(n_samples, (int, np.integer)) and not isinstance(n_samples, (bool, np.bool_))
        if single:
            ns, u_rows = _ragged_lengths([n_samples], [np.asarray(uniforms, dtype=np.float64).reshape(-1)])
        else:
            ns, u_rows = _ragged_lengths(n_samples, uniforms)
        N, Q = len(ns), self.params.quantization_steps
        if N < 1:
            raise ValueError("%s: no utterance" % what)
        O = self.local_hop if overlap is None else overlap
        Wm = self.input_width if warmup is None else warmup
        tile = check_tile(self.batch_tile if tile is None else tile, self.params, what)
        if isinstance(body, str):
            if body != "auto":
                raise ValueError("%s: body= takes samples per segment or \"auto\", got %r" % (what, body))
            fold.check_fold(max(1, O), O, Wm)                                     # (the body is not known yet)
            cap = self.fold_capacity(tile, N)
            bodies = [fold.auto_body(n, cap, O, Wm) for n in ns]
        else:
            bodies = [body] * N
        plans = [fold.fold_plan(ns[i], bodies[i], O, Wm) for i in range(N)]
        temps = sampling.per_utterance(temperature, N, "temperature")
        top_ks = sampling.per_utterance(top_k, N, "top_k")
        top_ps = sampling.per_utterance(top_p, N, "top_p")
        for i in range(N):
            sampling.check_controls(temps[i], top_ks[i], top_ps[i])
        cids = None if condition is None else list(sampling.per_utterance(condition, N, "condition"))
        prompts, which = self._batch_prompts(initial_tokens if not single or initial_tokens is None else
                                             np.asarray(initial_tokens).reshape(-1), N)
        Wd = len(prompts[0])
        silence = silence_window(Q, Wd)
        if isinstance(local, (list, tuple)):
            if len(local) != N:
                raise ValueError("%s: local= holds %d feature arrays for %d utterances" % (what, len(local), N))
            per = list(local)
        else:
            per = [local] * N
        phs = [int(v) for v in sampling.per_utterance(local_phase, N, "local_phase")]
        seg_of, lengths, us, wins, feats, phases = [], [], [], [], [], []
        for i in range(N):
            f = per[i]
            if f is None:
                self._local_features(None, 1, 1, 0)                                   # raises: the model needs features
            if not isinstance(f, torch.Tensor):
                f = np.asarray(f, dtype=np.float32)
            if len(f.shape) == 3 and f.shape[0] == 1:
                f = f[0]
            if len(f.shape) != 2 or int(f.shape[0]) != self.local_channels:
                raise ValueError("%s: utterance %d: local= must be (%d, frames), got %s" % (what, i, self.local_channels, tuple(f.shape)))
            if not 0 <= phs[i] < self.local_hop:
                raise ValueError("%s: utterance %d: local_phase must lie in [0, local_hop = %d), got %d" % (what, i, self.local_hop, phs[i]))
            cols = fold.check_columns(plans[i], Wd, phs[i], self.local_hop, self.local_interp, self.local_upsample,
                                      int(f.shape[1]), what if single else "%s: utterance %d" % (what, i))
            for g, (first, count, ph) in zip(plans[i].segments, cols):
                part = f[:, first:first + count]
                seg_of.append(i)
                lengths.append(g.e - g.s)
                us.append(u_rows[i][g.s:g.e])
                wins.append(prompts[which[i]] if g.s == 0 else silence)
                feats.append(part.contiguous() if isinstance(part, torch.Tensor) else np.ascontiguousarray(part))
                phases.append(ph)
        want = bool(return_chosen) or bool(return_segments)
        rep = lambda xs: [xs[i] for i in seg_of]
        # ---- device work from here on: every segment of every utterance in ONE ragged call ------------------------------------
        got = self.generate_batch(lengths, us, initial_tokens=np.stack(wins), temperature=rep(temps), top_k=rep(top_ks),
                                  top_p=rep(top_ps), condition=None if cids is None else rep(cids), local=feats,
                                  local_phase=phases, return_chosen=want, tile=tile)
        rows, chosen = got if want else (got, None)
        table = data.pcm_table(Q)
        pcm, own_ch, segs, at = [], [], [], 0
        for i in range(N):
            S = len(plans[i].segments)
            mine, mine_ch = rows[at:at + S], (chosen[at:at + S] if want else None)
            at += S
            pcm.append(self._unfold(mine, plans[i], table))
            if return_chosen:
                own_idx = self._fold_indices(plans[i])[0]
                own_ch.append(torch.cat(list(mine_ch))[torch.as_tensor(own_idx).to(self.device)])
            segs.append((plans[i], list(mine), list(mine_ch) if want else None))
        res = (pcm[0] if single else pcm,)
        if return_chosen:
            res += (own_ch[0] if single else own_ch,)
        if return_segments:
            res += (segs[0] if single else segs,)
        return res if len(res) > 1 else res[0]

    @staticmethod
    def _fold_indices(plan):
        """Indices into the concatenation of a plan's segment rows: (owner index of every position; the positions inside seams,
        their tail-side and head-side indices, their seam index i) -- int64 numpy arrays."""
        starts = np.cumsum([0] + [g.e - g.s for g in plan.segments])
        own = np.concatenate([np.arange(g.a - g.s, g.b - g.s, dtype=np.int64) + starts[u] for u, g in enumerate(plan.segments)])
        O, S = plan.overlap, len(plan.segments)
        i = np.arange(O, dtype=np.int64)
        ends = [plan.segments[u].b for u in range(S - 1)] if O else []
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros((0,), np.int64)
        pos = cat([b + i for b in ends])
        tail = cat([starts[u] + b - plan.segments[u].s + i for u, b in enumerate(ends)])
        head = cat([starts[u + 1] + b - plan.segments[u + 1].s + i for u, b in enumerate(ends)])
        return own, pos, tail, head, cat([i for _ in ends])

    def _unfold(self, rows, plan, table):
        """``fold.unfold`` on the device, bit for bit: ``rows`` the plan's int32 token rows, ``table`` ``data.pcm_table``'s values.
        The lookup is ``wn_mulaw_decode`` with the table's values as floats; the cross-fade is elementwise float32 torch
        operations in ``fold.unfold``'s order -- d = h - t; m = w * d; y = t + m, each rounded on its own -- then round half to
        even and clip."""
        from . import data, fold
        dev = self.device
        own, pos, tail, head, seam_i = (torch.as_tensor(a).to(dev) for a in self._fold_indices(plan))
        vals = data.pcm_lookup_device(torch.cat([r.to(torch.int32) for r in rows]).contiguous(), table)
        out = vals[own]
        if pos.numel():
            w = torch.as_tensor(fold.seam_weights(plan.overlap)).to(dev)[seam_i]
            t, h = vals[tail], vals[head]
            d = h - t
            m = w * d
            y = t + m
            out[pos] = y
        return torch.round(out).clamp_(-32768.0, 32767.0).to(torch.int16)

    def open_stream(self, utterances=1, initial_tokens=None, condition=None, local=None, local_phase=0, temperature=1.0,
                    top_k=0, top_p=1.0, return_chosen: bool = False, ring_frames=None, max_pull=4096, tile=None):
        """Streaming synthesis: a ``DecodeStream`` over ``utterances`` utterances -- features go in by ``push``, samples come out
        by ``pull``, in pieces of any size, and the concatenation of everything pulled equals row for row, bit for bit, what ONE
        ``generate_batch`` call with the same arguments and a table of the same rows returns (tokens, and ``chosen`` with
        ``return_chosen``, element 0 from the prefill row included).

        The call runs the prefill ``generate_batch`` runs -- the same rules per utterance for ``initial_tokens``, ``condition``,
        ``local`` / ``local_phase`` and the controls, the same refusals and messages -- and creates one decoder handle per
        utterance, which the stream keeps until ``close()``.  For a locally conditioned model ``local=`` is required: one
        (F, n) array or one per utterance, covering at least the window; columns beyond the window go into the ring.  Every
        utterance owns a ring of ``ring_frames`` = R rows on the device that its handle reads in place
        (``WN_DECODER_FRAME_RING``); R defaults to the smallest ring that serves pulls of ``max_pull`` samples with one pull's
        worth of rows fed ahead, and an R too small for ``max_pull`` raises, naming the minimum (``stream_frames``).
        Unconditioned and globally conditioned models take the same interface without a ring: ``pull`` only.  Given samples
        (``forced=``) are not part of a stream.

        Rows fed with ``push_rows`` are the table's rows by construction.  Rows made by ``push(features)`` come from a projection
        GEMM over fewer columns per call than the whole utterance's: in the default fp16 x 2 arithmetic the per-tile scales
        depend on a row's tile mates, so such rows agree with the whole-utterance rows to that GEMM's product error only, and a
        token can differ at a near-tie of the cumulative distribution -- the caveat of ``WN_DECODER_ONE_WORKGROUP``.

        Audio in: ``st.push(an.feed(chunk))`` with ``an = features.LogMel(...).stream()`` makes the next columns on the device, where
        the ring lives, and feeds them; column k needs the samples up to k hop + win / 2, a look-ahead of win / 2 samples.

        ``tile``: as for ``generate_batch``; the stream keeps its tile size for every ``pull``."""
        return DecodeStream(self, utterances, initial_tokens, condition, local, local_phase, temperature, top_k, top_p,
                            return_chosen, ring_frames, max_pull, tile)

    def _batch_plan(self, n_samples, uniforms, initial_tokens, temperature, top_k, top_p, condition, local, local_phase,
                    forced=None):
        """``generate_batch``'s arguments -> (one ``_Utterance`` per utterance, {group: (features on the device or None,
        phase)}), every check that needs no decoder made, in the order the messages always came in."""
        ragged = not isinstance(n_samples, (int, np.integer))
        if ragged:
            ns, u_rows = _ragged_lengths(n_samples, uniforms)
        else:
            u_rows = np.ascontiguousarray(np.asarray(uniforms, dtype=np.float64))
            if u_rows.ndim != 2 or u_rows.shape[1] < n_samples:
                raise Exception("uniforms must be (N, >= n_samples)")
            ns = [int(n_samples)] * u_rows.shape[0]
        N = len(ns)
        temps = [float(t) for t in sampling.per_utterance(temperature, N, "temperature")]
        top_ks = [int(k) for k in sampling.per_utterance(top_k, N, "top_k")]
        top_ps = [float(v) for v in sampling.per_utterance(top_p, N, "top_p")]
        for i in range(N):
            sampling.check_controls(temps[i], top_ks[i], top_ps[i])
        if not ragged and n_samples < 1:
            raise Exception("generate_batch: n_samples must be positive")
        if N < 1:
            raise Exception("generate_batch: no utterance")
        prompts, which = self._batch_prompts(initial_tokens, N)
        if self.condition_classes:
            if condition is None:
                self._condition_ids(None, N)                                      # raises: a conditioned model needs ids
            cids = [self._class_id(c) for c in sampling.per_utterance(condition, N, "condition")]
        else:
            self._condition_ids(condition, N)                                     # raises when ids were given
            cids = [None] * N
        if isinstance(local, (list, tuple)):
            if len(local) != N:
                raise Exception("generate_batch: local= holds %d feature arrays for %d utterances" % (len(local), N))
            per = list(local)
        else:
            per = [local] * N
        phs = [int(v) for v in sampling.per_utterance(local_phase, N, "local_phase")]
        given = self._batch_forced(forced, ns)
        seen = {}                                                                 # the distinct feature arrays, by identity
        recs = [_Utterance(ns[i], u_rows[i], temps[i], top_ks[i], top_ps[i], cids[i], per[i], phs[i], prompts[which[i]],
                           (which[i], cids[i], seen.setdefault(id(per[i]), len(seen)), phs[i]), given[i]) for i in range(N)]
        # the features are checked against each utterance's own length: again only for a longer utterance than the longest so
        # far of the same (window, features, phase), so the first utterance they do not cover is the one that raises
        checked, covered = {}, {}
        for i, r in enumerate(recs):
            key = r.group[:1] + r.group[2:]
            if key not in checked or r.n > covered[key]:
                try:
                    checked[key] = self._utterance_local(r.local, r.phase, len(r.window), r.n, "generate_batch")
                except Exception as e:
                    if not ragged:
                        raise
                    raise Exception("generate_batch: utterance %d: %s" % (i, e))
                covered[key] = r.n
        return recs, {r.group: checked[r.group[:1] + r.group[2:]] for r in recs}

    def _batch_forced(self, forced, ns):
        """``generate_batch``'s ``forced`` -> one checked int32 array or None per utterance (``ns``: their lengths); the message
        of whatever is wrong names the utterance."""
        N, Q = len(ns), self.params.quantization_steps
        if forced is None:
            return [None] * N
        if isinstance(forced, (list, tuple)) and any(e is None or np.ndim(e) > 0 for e in forced):
            if len(forced) != N:
                raise ValueError("generate_batch: forced= holds %d entries for %d utterances" % (len(forced), N))
            per = list(forced)
        else:
            one = np.asarray(forced.detach().cpu() if hasattr(forced, "detach") else forced)
            if one.ndim != 1 or one.shape[0] < max(ns):
                raise ValueError("generate_batch: one forced= array for all utterances must be 1-D and hold the longest "
                                 "utterance's %d entries, got shape %s" % (max(ns), one.shape))
            per = [one[:n] for n in ns]
        out = []
        for i, (e, n) in enumerate(zip(per, ns)):
            try:
                out.append(None if e is None else sampling.check_forced(e, n, Q))
            except ValueError as err:
                raise ValueError("generate_batch: utterance %d: %s" % (i, err))
        return out

    def _batch_handles(self, recs, feats, ragged, chosen=False, forced=False):
        """``chosen`` / ``forced``: the form of every handle of the call (``_Handle.bring`` creates a handle of another form anew).
        A handle per utterance with its sampling controls, holding its class's biases, its frame table and, in a ragged
        call, its step limit (its decode steps: the first sample comes from the prefill).  Tables and limits belong to the
        utterance, so such handles are updated in every call; a handle created here holds all of it already."""
        lib = _lib.lib()
        biases = {c: self.condition_biases(c) for c in sorted({r.class_id for r in recs})} if self.condition_classes else {None: None}

        def bring(h, r):
            ft, ph = feats[r.group]       # (a handle is created WITH its table)
            h.bring(self, r.class_id, biases.get, None if ft is None else self._decoder_table(ft, ph, len(r.window)),
                    r.n - 1 if ragged else None, chosen, forced)
        held = len(self._handles)
        for r in recs[held:]:
            self._handles.append(_Handle())
            bring(self._handles[-1], r)
        for i, r in enumerate(recs):
            if i < held:
                bring(self._handles[i], r)
            check(lib.wn_decoder_set_sampling(self._handles[i].h, r.temperature, r.top_k, r.top_p), "wn_decoder_set_sampling")

    def _generate_batch_loop(self, recs, ragged, return_chosen=False):
        """generate_batch for what ``wn_decoder_run_batch`` does not cover: ``generate()`` per utterance (row u is
        ``generate(<utterance u's length>, uniforms[u], initial_tokens=<utterance u's window>)`` with utterance u's controls
        by definition); ``ragged``: a list of rows comes back."""
        rows = [self.generate(r.n, r.u, initial_tokens=r.window, temperature=r.temperature, top_k=r.top_k, top_p=r.top_p,
                              condition=r.class_id, local=r.local, local_phase=r.phase, return_chosen=return_chosen,
                              forced=r.forced) for r in recs]
        if return_chosen:
            toks, ch = [t for t, _ in rows], [c for _, c in rows]
            return (toks, ch) if ragged else (torch.stack(toks), torch.stack(ch))
        return rows if ragged else torch.stack(rows)


class StreamBook(object):
    """The host's books of a ``DecodeStream``: per utterance the frames fed and the decoder steps run, and every refusal of
    ``push`` and ``pull`` -- plain integers, no device (``stream_frames`` is the arithmetic).  ``ring``: R, or 0 for a stream
    without a ring (a model without local conditioning); ``phases``: the decoders' ``frame_phase`` per utterance; ``two_steps``:
    the launches are the nine-workgroup decoder's, which runs two steps at least."""

    def __init__(self, phases, hop=0, linear=False, ring=0, two_steps=False):
        self.phases, self.hop, self.linear, self.ring, self.two_steps = [int(p) for p in phases], int(hop), bool(linear), int(ring), bool(two_steps)
        self.n = len(self.phases)
        self.fed, self.done, self.started = [0] * self.n, [0] * self.n, False

    def frames(self, u, pull=0):
        return stream_frames(self.hop, self.linear, self.phases[u], self.fed[u], self.done[u], pull)

    def available(self):
        """Samples that can be pulled per utterance from the rows present (None: no ring, no bound): the steps the frames fed
        allow, and before the first pull one more -- the prefill's sample, which takes no step."""
        if not self.ring:
            return [None] * self.n
        return [self.frames(u).steps + (0 if self.started else 1) for u in range(self.n)]

    def check_push(self, counts):
        """``counts[u]`` more frames for utterance u: refused when they would overwrite a row that is still to be read."""
        if not self.ring:
            raise Exception("push: this stream has no ring (the model has no local conditioning): pull only")
        if len(counts) != self.n:
            raise Exception("push: %d arrays for %d utterances" % (len(counts), self.n))
        for u, k in enumerate(counts):
            cur = self.frames(u).current
            if self.fed[u] + int(k) > cur + self.ring:
                raise Exception("push: utterance %d: %d more rows on top of the %d fed would overwrite a row not yet consumed: the "
                                "ring holds %d rows and the decoder has consumed %d (pull first, or open the stream with a larger "
                                "ring_frames)" % (u, int(k), self.fed[u], self.ring, cur))

    def pushed(self, counts):
        for u, k in enumerate(counts):
            self.fed[u] += int(k)

    def steps_of(self, n):
        """A pull of ``n`` samples runs n decoder steps -- n - 1 when it is the first: its element 0 is the prefill's."""
        return int(n) - (0 if self.started else 1)

    def check_pull(self, n):
        n = int(n)
        if n < 1:
            raise Exception("pull: n must be positive, got %d" % n)
        steps = self.steps_of(n)
        if self.two_steps and steps == 1:
            raise Exception("pull: %d sample%s here is ONE decoder step, and the nine-workgroup decoder of this model's shape runs two "
                            "at least (n >= 2 per launch): pull %s" % (n, "" if n == 1 else "s (the first is the prefill's)",
                                                                      "1, or 3 and more" if not self.started else "2 and more"))
        for u in range(self.n if self.ring else 0):
            f = self.frames(u, steps)
            if steps > f.steps:
                raise Exception("pull: utterance %d: %d samples asked for, the rows present allow %d (%d frames fed, %d steps run, "
                                "hop %d, phase %d%s): push more first"
                                % (u, n, f.steps + (0 if self.started else 1), self.fed[u], self.done[u], self.hop, self.phases[u],
                                   "; linear interpolation reads the frame after a step's own" if self.linear else ""))
            if f.reads > self.ring:
                raise Exception("pull: utterance %d: %d samples read %d frames at once, the ring holds %d: pull less, or open the "
                                "stream with a larger ring_frames" % (u, n, f.reads, self.ring))
        return steps

    def pulled(self, steps):
        self.started = True
        for u in range(self.n):
            self.done[u] += int(steps)


class DecodeStream(object):
    """What ``FasterWaveNet.open_stream`` returns (see there): ``push`` / ``push_rows`` feed frames, ``available`` says how many
    samples they allow, ``pull`` draws them, ``close`` destroys the handles and then drops the rings.  Also a context manager.
    The stream holds the weights as they were when it was opened."""

    def __init__(self, net, utterances, initial_tokens, condition, local, local_phase, temperature, top_k, top_p, return_chosen,
                 ring_frames, max_pull, tile=None):
        self.net, self._hs, self._rings, self.closed = net, [], [], False
        self.tile = check_tile(net.batch_tile if tile is None else tile, net.params, "open_stream")      # kept for every pull
        N = int(utterances)
        if N < 1:
            raise Exception("open_stream: utterances must be positive, got %d" % N)
        # generate_batch's own plan over one sample per utterance: its rules, refusals and messages (the features must cover
        # the window), and the groups that share a prefill
        recs, feats = net._batch_plan(1, np.zeros((N, 1)), initial_tokens, temperature, top_k, top_p, condition, local, local_phase)
        self._recs, self.return_chosen = recs, bool(return_chosen)
        flags = _lib.default_exec_flags() if net.exec_flags is None else int(net.exec_flags)
        nine = net._nine_workgroup_shape(flags)
        self._nine, self._one_wg = nine, bool(nine and flags & _lib.WN_DECODER_ONE_WORKGROUP)
        self.max_pull = int(max_pull)
        if self.max_pull < 1:
            raise Exception("open_stream: max_pull must be positive, got %d" % self.max_pull)
        hop, linear, R = 0, False, 0
        if net.local_channels:
            hop, linear = net.local_fine_hop, net.local_interp == "linear"
            least = stream_frames(hop, linear, 0, pull=self.max_pull).min_ring
            R = least + (self.max_pull + hop - 1) // hop if ring_frames is None else int(ring_frames)
            if R < least:
                raise Exception("open_stream: ring_frames = %d is too small for max_pull = %d: a pull of %d samples at hop %d reads up "
                                "to %d frames at once%s, the minimum" % (R, self.max_pull, self.max_pull, hop, least,
                                                                          " (linear interpolation: one more)" if linear else ""))
        elif ring_frames is not None:
            raise Exception("open_stream: ring_frames= was given, but this model has no local conditioning: its streams have no ring")
        W = [len(r.window) for r in recs]
        starts = [divmod(r.phase + W[i], hop) if R else (0, 0) for i, r in enumerate(recs)]      # (first frame of the ring, frame_phase)
        self.book = StreamBook([ph for _, ph in starts], hop, linear, R, nine and not self._one_wg)
        self.ring_frames = R
        lib, dev = _lib.lib(), net.device
        # ---- device work from here on -----------------------------------------------------------------------------------------
        first_rows_of = {}
        if R:
            # the rows the features given here make -- the table generate_batch would build --, from the decoder's first frame on
            rows_of = {g: net.local_biases(feats[g][0][0], feats[g][1]) for g in sorted({r.group for r in recs}, key=self._group_key)}
            width = int(next(iter(rows_of.values())).shape[1])
            self._last_col = [feats[r.group][0][0][:, -1:].clone() for r in recs]      # the learned layer reads neighbouring pairs
            for i, r in enumerate(recs):
                self._rings.append(torch.zeros((R, width), device=dev, dtype=torch.float32))
            head = [rows_of[r.group][starts[i][0]:] for i, r in enumerate(recs)]
            self.book.check_push([int(h.shape[0]) for h in head])
        biases = {c: net.condition_biases(c) for c in sorted({r.class_id for r in recs})} if net.condition_classes else {None: None}
        for i, r in enumerate(recs):
            d, _keep = net._desc(biases[r.class_id], (self._rings[i], hop, starts[i][1]) if R else None, 0, self.return_chosen,
                                 ring=bool(R))
            h = C.c_void_p()
            check(lib.wn_decoder_create(C.byref(h), C.byref(d), stream_ptr()), "wn_decoder_create")
            self._hs.append(h)
            check(lib.wn_decoder_set_sampling(h, r.temperature, r.top_k, r.top_p), "wn_decoder_set_sampling")
        if R:
            self._write(head)
        net.prev_causal_outputs = None
        for g in sorted({r.group for r in recs}, key=self._group_key):
            mine = [i for i in range(N) if recs[i].group == g]
            r = recs[mine[0]]
            tok = torch.as_tensor(r.window.reshape(1, -1)).to(dev)
            p0, sum_skip = net._seed(tok, r.class_id, feats[g][0], r.phase, [self._hs[i] for i in mine])
            for t in sorted({recs[i].temperature for i in mine}):
                first_rows_of[g + (t,)] = net._first_row(sum_skip, p0, t)
        self._first_rows = [first_rows_of[r.group + (r.temperature,)] for r in recs]
        self._last = None                  # the newest token of every utterance, on the host

    @staticmethod
    def _group_key(g):
        return (g[0], -1 if g[1] is None else g[1], g[2], g[3])

    # -- feeding ------------------------------------------------------------------------------------------------------------------
    def _write(self, rows):
        """rows[u] (k_u, width) on the device -> ring slots (fed + i) mod R of utterance u, in stream order; the books follow."""
        R = self.ring_frames
        for u, x in enumerate(rows):
            k, at = int(x.shape[0]), self.book.fed[u] % R
            first = min(k, R - at)
            if first:
                self._rings[u][at:at + first].copy_(x[:first])
            if k > first:
                self._rings[u][:k - first].copy_(x[first:])
        self.book.pushed([int(x.shape[0]) for x in rows])

    def _per_utterance(self, what, x, ndim):
        per = list(x) if isinstance(x, (list, tuple)) else [x]
        if not isinstance(x, (list, tuple)) and self.book.n != 1:
            raise Exception("%s: one array serves a stream of one utterance; this one has %d: pass a list of one per utterance"
                            % (what, self.book.n))
        if len(per) != self.book.n:
            raise Exception("%s: %d arrays for %d utterances" % (what, len(per), self.book.n))
        out = []
        for u, a in enumerate(per):
            a = a if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float32)
            if len(a.shape) != ndim:
                raise Exception("%s: utterance %d: a %d-D array is needed, got shape %s" % (what, u, ndim, tuple(a.shape)))
            out.append(a)
        return out

    def push_rows(self, rows):
        """Projected fine rows, what ``net.local_biases`` returns: (k, row width) for a stream of one utterance, else a list of
        one array per utterance; k may differ between utterances and may be 0.  They become frames fed .. fed + k - 1 of their
        utterance, written to ring slots J mod R.  A push that would overwrite a row not yet consumed raises before any device
        work, naming the utterance and both counts."""
        self._open()
        per = self._per_utterance("push_rows", rows, 2)
        self.book.check_push([int(a.shape[0]) for a in per])      # (also: a stream without a ring takes no rows)
        width = int(self._rings[0].shape[1])
        for u, a in enumerate(per):
            if int(a.shape[1]) != width:
                raise Exception("push_rows: utterance %d: rows of %d floats, the model's rows hold %d (sum of 2 cd over the layers)"
                                % (u, int(a.shape[1]), width))
        dev = self.net.device
        self._write([(a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float32) for a in per])

    def push(self, features):
        """The next coarse feature columns: (F, k) for a stream of one utterance, else a list of one array per utterance; k may
        differ between utterances and may be 0.  They go through the learned upsampling layer when ``local_upsample`` > 1 (the
        stream keeps every utterance's last coarse column: the layer reads neighbouring pairs, so k columns make k U fine ones)
        and through the projection -- the path of ``net.local_biases`` --, and the rows are fed as ``push_rows`` feeds them."""
        self._open()
        net = self.net
        per = self._per_utterance("push", features, 2)
        for u, a in enumerate(per):
            if self.book.ring and int(a.shape[0]) != net.local_channels:
                raise Exception("push: utterance %d: features of %d channels, the model takes %d" % (u, int(a.shape[0]), net.local_channels))
        U = net.local_upsample if self.book.ring else 1
        self.book.check_push([int(a.shape[1]) * U for a in per])
        rows, dev = [], net.device
        width = int(self._rings[0].shape[1])
        made = {}                                  # utterances given the same array (behind the same last column) share a projection
        for u, a in enumerate(per):
            if int(a.shape[1]) == 0:
                rows.append(torch.empty((0, width), device=dev, dtype=torch.float32))
                continue
            key = (id(a), id(self._last_col[u]) if U > 1 else None)
            if key not in made:
                x = (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev, torch.float32)
                # net.local_biases' own path, without its check that the columns cover a window: these are columns in the middle
                with torch.no_grad():
                    f = (torch.cat([self._last_col[u], x], dim=1) if U > 1 else x)[None]
                    if U > 1:
                        f = net._upsample(f).permute(0, 2, 1)
                    made[key] = (net._local_block(f)[0].contiguous(), x[:, -1:].clone())
            rows.append(made[key][0])
            self._last_col[u] = made[key][1]
        self._write(rows)

    def available(self):
        """Per utterance: how many samples can be pulled from the rows present (``stream_frames``; linear interpolation needs
        the row after a step's own).  None per utterance on a stream without a ring."""
        return self.book.available()

    # -- drawing ------------------------------------------------------------------------------------------------------------------
    def pull(self, n, uniforms):
        """``n`` more samples of every utterance: (utterances, n) int32 on the device -- with ``return_chosen`` ``(tokens,
        chosen)``, chosen float32 of the same shape.  ``uniforms``: (utterances, n) float64, one per emitted sample, as in
        ``generate_batch``.  Raises before any device work, naming the utterance, when n exceeds what ``available()`` allows.
        One utterance runs ``wn_decoder_run``, several ``wn_decoder_run_batch`` -- over several launches when there are more
        than a launch takes (``deal_launches``).  The nine-workgroup decoder (config 4's shape) runs two steps at least per
        launch: there a pull must not come to exactly one decoder step (n >= 2; the first pull, whose element 0 is the
        prefill's, n = 1 or n >= 3)."""
        self._open()
        net, book, recs = self.net, self.book, self._recs
        N, Q, lib, dev = book.n, net.params.quantization_steps, _lib.lib(), net.device
        u_host = np.ascontiguousarray(np.asarray(uniforms.cpu() if isinstance(uniforms, torch.Tensor) else uniforms, dtype=np.float64))
        if u_host.shape != (N, int(n)):
            raise Exception("pull: uniforms must be (%d, %d) float64, one per emitted sample, got %s" % (N, int(n), u_host.shape))
        steps = book.check_pull(n)
        n = int(n)
        u = torch.as_tensor(u_host).to(dev)
        out = torch.empty((N, n), device=dev, dtype=torch.int32)
        ch = torch.empty((N, n), device=dev, dtype=torch.float32) if self.return_chosen else None
        off = n - steps                                            # 1 on the first pull: element 0 is the prefill's
        if off:
            first = torch.empty((N,), device=dev, dtype=torch.int32)
            u0 = u[:, 0].contiguous()
            if all(sampling.controls_off(r.temperature, r.top_k, r.top_p, Q) for r in recs):
                first_prob = torch.cat(self._first_rows, dim=0).contiguous()
                check(lib.wn_sample_categorical(ptr(first_prob), ptr(u0), ptr(first), N, Q, stream_ptr()), "wn_sample_categorical")
            else:
                for i, r in enumerate(recs):
                    check(lib.wn_sample_categorical_filtered(ptr(self._first_rows[i]), ptr(u0[i:i + 1]), ptr(first[i:i + 1]), 1, Q,
                                                             r.top_k, r.top_p, stream_ptr()), "wn_sample_categorical_filtered")
            out[:, 0] = first
            if ch is not None:
                ch[:, 0] = torch.cat(self._first_rows, dim=0).gather(1, first.long()[:, None])[:, 0]
            self._last = [int(v) for v in first.cpu().tolist()]
        if steps:
            # (the nine-workgroup form keeps its token buffers, as in generate_batch)
            outs = [torch.empty((steps,), device=dev, dtype=torch.int32) if self._nine else out[i][off:] for i in range(N)]
            us = [u[i][off:] for i in range(N)]
            chs = [ch[i][off:] for i in range(N)] if ch is not None else None
            batched = N > 1 and not self._one_wg
            if batched:
                limit = int(lib.wn_decoder_batch_max()) if self._nine else _lib.WN_DECODER_BATCH_MAX_ANY
                same = 1 if self._nine and os.environ.get("WAVENET_HIP_BATCH_OWN_WEIGHTS") != "1" else 0
                launched = 0
                for n_launch, sel in deal_launches([steps] * N, limit):
                    U = net._launch_tile(self.tile, len(sel), self._nine)      # a tile size, or None: `same` as ever
                    rc = lib.wn_decoder_run_batch((C.c_void_p * len(sel))(*[self._hs[i].value for i in sel]), len(sel),
                                                  (C.c_int32 * len(sel))(*[self._last[i] for i in sel]), ptr_array([us[i] for i in sel]),
                                                  n_launch, ptr_array([outs[i] for i in sel]),
                                                  ptr_array([chs[i] for i in sel]) if chs is not None else None,
                                                  same if U is None else U, stream_ptr())
                    if rc == _lib.WN_ESHAPE and self._nine and not launched:
                        batched = False            # refused before any device work: nine workgroups per utterance do not fit the device
                        break
                    check(rc, "wn_decoder_run_batch")
                    launched += 1
            if not batched:
                for i in range(N):
                    check(lib.wn_decoder_run(self._hs[i], self._last[i], ptr(us[i]), steps, ptr(outs[i]),
                                             ptr(chs[i]) if chs is not None else None, stream_ptr()), "wn_decoder_run")
            for i in (range(N) if self._nine else range(1)):
                check(lib.wn_decoder_status(self._hs[i], stream_ptr()), "wn_decoder_status")
            if self._nine:
                for i in range(N):
                    out[i][off:] = outs[i]
            self._last = [int(v) for v in out[:, -1].cpu().tolist()]
        book.pulled(steps)
        return (out, ch) if self.return_chosen else out

    # -- the end ------------------------------------------------------------------------------------------------------------------
    def _open(self):
        if self.closed:
            raise Exception("this stream is closed")

    def close(self):
        """Destroy the handles, then drop the rings they read (in that order: a handle reads its ring in place)."""
        hs, self._hs = self._hs, []
        for h in hs:
            _lib.lib().wn_decoder_destroy(h)
        self._rings, self.closed = [], True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
