"""Local conditioning on the GPU: per-(clip, frame) bias rows through the C ABI (WnStackDesc.bias_hop / bias_phase /
bias_frame_stride under WN_EXEC_BIAS_PER_CLIP) against the float64 reference of tests/local_cond_ref.py and, bit for bit,
against the per-clip form where a frame covers a clip; then the locally conditioned model -- loss and every gradient, the
replayed training step, scoring, checkpoints and the weight average.

The tiny case (cond_ref.TINY, B = 3, T = 70, F = 5, hop = 12, phase = 5): three 32-column tiles per clip, the last one
partial, one four-wave workgroup holding tiles of two clips; 7 frames whose borders fall inside tiles, a partial first and
last frame, and the d = 4 layers' zero prefix (Z = 2) cutting into the first frame."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from gpu_util import btc, dev, to_np
from oracle import wavenet_ref as R
from test_gpu_condition import _Stack, _ex, _split_z
from wavenet_amd import Params, TrainStepGraph, WaveNet, _lib
from wavenet_amd._lib import ptr
from wavenet_amd.graph import default_loss

pytestmark = pytest.mark.gpu

PER_CLIP = _lib.WN_EXEC_BIAS_PER_CLIP
GENERIC = _lib.WN_EXEC_FORCE_GENERIC
ATOL = 1e-4                      # tests/test_gpu_parity.py: fp32 activations and logits within 1e-4 absolute
U32 = 2.0 ** -24                 # unit round-off of float32
B, T = LR.B, LR.T


# ---- the residual stack through the C ABI ---------------------------------------------------------------------------------
class _FrameStack(_Stack):
    """test_gpu_condition's stack with the three trailing descriptor fields; ``frames`` = (hop, phase, frame stride) or None."""
    frames = None

    def desc(self, bias=None):
        d, keep = super().desc(bias)
        if self.frames is not None:
            d.bias_hop, d.bias_phase, d.bias_frame_stride = self.frames
        return d, keep

    def bwd_ws(self, x, acts, dout, dskip, dblock, ex, t_off=0):
        """_Stack.bwd that also hands back the workspace (layer 0's (da | dg) scratch lies behind the dz tables)."""
        Bn, Tn, _ = x.shape
        xs, z, f, g, _ = acts
        d, keep = self.desc(torch.zeros_like(dblock))
        lib = _lib.lib()
        gW = {k: [torch.zeros_like(t) for t in self.W[k]] for k in self.W}
        tabs = {k: self._tab([t.data_ptr() for t in gW[k]]) for k in gW}
        p0 = dblock.data_ptr()
        dbf = self._tab([p0 + 4 * r[0] for r in self.rows])
        dbg = self._tab([p0 + 4 * r[1] for r in self.rows])
        nbytes = lib.wn_stack_bwd_workspace_bytes(C.byref(d), Bn, Tn)
        ws = torch.zeros((nbytes // 4,), device="cuda")
        dx = torch.zeros_like(x)
        rc = lib.wn_stack_bwd(C.byref(d), ptr(x), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(dout), ptr(dskip), ptr(dx),
                              tabs["Wf"][1], dbf[1], tabs["Wg"][1], dbg[1], tabs["Wp"][1], None, tabs["Ws"][1], None,
                              ptr(ws), nbytes, Bn, Tn, t_off, 1, ex, None)
        torch.cuda.synchronize()
        return rc, dx, gW, ws


def _case(over=LR.TINY, seed=0, hop=LR.HOP, phase=LR.PHASE, bias_scale=0.5, pad=0, Bn=B, Tn=T):
    """Stack, input (B, Cr, 1, T) and a (B, n, R + pad) block of random rows; st.frames is set."""
    st = _FrameStack(over)
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((Bn, st.Cr, 1, Tn)).astype(np.float32)
    n = LR.frames_needed(Tn, hop, phase)
    block = (rs.standard_normal((Bn, n, st.R + pad)) * bias_scale).astype(np.float32)
    st.frames = (hop, phase, st.R + pad)
    return st, x, block


def _run(st, x, block, prec, flags, t1, t_off=0, window_only=0):
    n, rs = block.shape[1], block.shape[2]
    rc, got = st.fwd(dev(btc(x)), dev(block), _ex(prec, flags | PER_CLIP, n * rs, t1), t_off, window_only)
    assert rc == 0, _lib.lib().wn_last_error()
    return got


def _against_reference(st, x, block, hop, phase, got, t_off=0, saved=True):
    Bn, Tn = x.shape[0], x.shape[3]
    layers, skip, amax = LR.stack_forward(st.p, st.w, x, block[:, :, :st.R], hop, phase)
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL, err_msg="out %d" % l)
        for k in ((1, 2, 3) if saved else (1,)):
            np.testing.assert_allclose(to_np(_split_z(st, got[k], Bn, Tn)[l]), btc(layers[l][k]), atol=ATOL,
                                       err_msg="%s %d" % (("z", "tanh", "sigmoid")[k - 1], l))
    np.testing.assert_allclose(to_np(got[4]), btc(skip)[:, t_off:], atol=ATOL)
    return amax


PATHS = [("fp32", 0, 1), ("fp32", 0, -1), ("bf16x3", 0, 1), ("fp32", GENERIC, 0), ("fp16x2", 0, 1)]


@pytest.mark.parametrize("prec,flags,t1", PATHS)
def test_per_frame_rows_against_the_reference_on_every_path(prec, flags, t1):
    """wn_stack_fwd with bias_hop = 12, bias_phase = 5 against the float64 reference within ATOL: every layer's out, z, tanh,
    sigmoid and the skip sum -- exact fp32 with the one-tile-per-wave kernel on and off, bf16x3, WN_EXEC_FORCE_GENERIC, and
    fp16 x 2 (k_layer_fwd_h2_t1<1, kCondFrame>).  Clips and frames hold different rows, so a wrong clip or frame index shows."""
    st, x, block = _case()
    got = _run(st, x, block, prec, flags, t1)
    _against_reference(st, x, block, LR.HOP, LR.PHASE, got)
    z2 = _split_z(st, got[1], B, T)[2]                       # the d = 4 layer: zero prefix, neither convolution nor bias
    Z = R.conv_pad_and_prefix(T, 4, 2)[1]
    assert Z == 2 and float(z2[:, :Z].abs().max()) == 0.0 and float(z2[:, Z].abs().max()) > 0.0


def _fwd_save(st, x, block, ex, save):
    """wn_stack_fwd with nothing (0), tanh + sigmoid (1) or sigmoid only (2) saved -- the three SAVE forms."""
    Bn, Tn = x.shape[0], x.shape[3]
    xd, bd = dev(btc(x)), dev(block)
    d, keep = st.desc(bd)
    xs = torch.zeros((st.L, Bn, Tn, st.Cr), device="cuda")
    z = torch.zeros((Bn * Tn * st.ncd,), device="cuda")
    f = torch.zeros_like(z) if save == 1 else None
    g = torch.zeros_like(z) if save >= 1 else None
    skip = torch.zeros((Bn, Tn, st.Cs), device="cuda")
    rc = _lib.lib().wn_stack_fwd(C.byref(d), ptr(xd), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(skip), Bn, Tn, 0, 1, 0, ex, None)
    torch.cuda.synchronize()
    return rc, (xs, z, f, g, skip)


@pytest.mark.parametrize("save", [0, 1, 2])
def test_fp16x2_per_frame_kernels_in_their_two_save_forms_and_the_refusal_of_the_third(save):
    """k_layer_fwd_h2_t1<SAVE, kCondFrame>, SAVE = 0 / 1, against the reference within ATOL.  SAVE = 2 (sigmoid only) is what
    a stack whose backward can recover tanh asks for; a stack with bias rows cannot, so the library refuses that call with
    WN_EARG before any device work -- per frame as per clip -- and no <2, kCondFrame> kernel exists."""
    st, x, block = _case(seed=1)
    n, rs = block.shape[1], block.shape[2]
    rc, got = _fwd_save(st, x, block, _ex("fp16x2", PER_CLIP, n * rs, 1), save)
    if save == 2:
        st.frames = None
        rc2, _ = _fwd_save(st, x, block, _ex("fp16x2", PER_CLIP, n * rs, 1), save)
        assert rc == rc2 == _lib.WN_EARG and float(got[0].abs().max()) == 0.0
        return
    assert rc == 0, _lib.lib().wn_last_error()
    layers, skip, _ = LR.stack_forward(st.p, st.w, x, block, LR.HOP, LR.PHASE)
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL)
        np.testing.assert_allclose(to_np(_split_z(st, got[1], B, T)[l]), btc(layers[l][1]), atol=ATOL)
        if save == 1:
            np.testing.assert_allclose(to_np(_split_z(st, got[2], B, T)[l]), btc(layers[l][2]), atol=ATOL)
            np.testing.assert_allclose(to_np(_split_z(st, got[3], B, T)[l]), btc(layers[l][3]), atol=ATOL)
    np.testing.assert_allclose(to_np(got[4]), btc(skip), atol=ATOL)


@pytest.mark.parametrize("prec,t1", [("bf16x3", 1), ("fp16x2", 1)])
def test_per_frame_rows_with_window_only_and_a_ragged_window_offset(prec, t1):
    """The training form of the call: window_only and t_off = 37 (no multiple of 32).  t counts inside the call's T columns
    whatever t_off says, and a stack with bias rows computes every column."""
    st, x, block = _case(seed=2)
    got = _run(st, x, block, prec, 0, t1, t_off=37, window_only=1)
    assert got[4].shape == (B, T - 37, st.Cs)
    _against_reference(st, x, block, LR.HOP, LR.PHASE, got, t_off=37)


@pytest.mark.parametrize("prec,flags,t1", [("fp32", 0, 1), ("fp32", GENERIC, 0), ("fp16x2", 0, 1)])
@pytest.mark.parametrize("hop", [1, 12, 32, 33])
@pytest.mark.parametrize("last_phase", [False, True])
def test_hops_and_phases(prec, flags, t1, hop, last_phase):
    """hop in {1, 12, 32, 33} (a frame per position; borders inside tiles; a frame per tile when phase = 0; frames that drift
    against the tiles) with phase in {0, hop - 1}, and a frame stride with 4 floats of padding behind the rows."""
    phase = hop - 1 if last_phase else 0
    st, x, block = _case(seed=3 + hop, hop=hop, phase=phase, pad=4)
    got = _run(st, x, block, prec, flags, t1)
    _against_reference(st, x, block, hop, phase, got)


@pytest.mark.parametrize("Cr,cd", [(64, 32), (128, 128)])
def test_per_frame_rows_on_the_wide_path(Cr, cd):
    """Widths the fused 32/32/2 kernels do not cover (wide_layer.hip): the gate GEMMs run without a bias and k_wide_gate adds
    the row of (clip, frame of t).  Forward against the reference within ATOL; gradient rows against the float64 reference
    gradient within 2e-4 of the block's largest entry (the bound the parity tests put on a gradient tensor)."""
    over = dict(quantization_steps=256, causal_conv_channels=[Cr], residual_conv_channels=[cd] * 3, residual_num_blocks=1,
                softmax_conv_channels=[64, 256])
    assert _lib.lib().wn_layer_fast_path(Cr, cd, 2) == 0
    st, x, block = _case(over, seed=6)
    got = _run(st, x, block, "bf16x3", 0, 0)
    _against_reference(st, x, block, LR.HOP, LR.PHASE, got)
    _grad_rows_against_reference(st, x, block, "bf16x3", 0)


# ---- bitwise anchors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,flags,t1", PATHS)
def test_a_frame_that_covers_the_clip_is_the_per_clip_call_bit_for_bit(prec, flags, t1):
    """hop >= T + phase: one frame per clip.  Forward (every output) and backward (dx, the bias-gradient rows and, on the fused
    paths, every weight gradient) equal the per-clip call on the same rows bit for bit, on every path."""
    st, x, block = _case(seed=4, hop=T + 7, phase=6)
    assert block.shape[1] == 1
    rs = np.random.RandomState(40)
    t_off = 21
    dout = dev(rs.standard_normal((B, T, st.Cr)).astype(np.float32))
    dskip = dev(rs.standard_normal((B, T - t_off, st.Cs)).astype(np.float32))
    xd, bd = dev(btc(x)), dev(block)
    res = []
    for frames in (st.frames, None):
        st.frames = frames
        ex = lambda: _ex(prec, flags | PER_CLIP, st.R, t1)
        rc, acts = st.fwd(xd, bd, ex(), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        grad = torch.full((B, 1, st.R), 0.25, device="cuda")
        rc, dx, gW = st.bwd(xd, acts, dout, dskip, grad, ex(), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        res.append((acts, dx, gW, grad))
    (a0, dx0, g0, r0), (a1, dx1, g1, r1) = res
    for k in range(5):
        assert torch.equal(a0[k], a1[k]), k
    assert torch.equal(dx0, dx1) and torch.equal(r0, r1) and float((r0 - 0.25).abs().max()) > 1e-2
    if not flags & GENERIC:         # (the any-shape weight-gradient kernels leave through float atomics, with or without bias rows)
        for k in g0:
            for l in range(st.L):
                assert torch.equal(g0[k][l], g1[k][l]), (k, l)


def test_zero_rows_and_zero_fields_change_no_bit():
    """(a) fp16 x 2: a table of zero rows per frame equals the per-clip call with zero rows bit for bit.  (b) A call with the
    three new fields zero is the call it was: a descriptor built without them and one with them set to 0 explicitly, with and
    without the flag."""
    st, x, block = _case(seed=5)
    zero = np.zeros_like(block)
    a = _run(st, x, zero, "fp16x2", 0, 1)
    frames, st.frames = st.frames, None
    rc, b = st.fwd(dev(btc(x)), dev(zero[:, 0]), _ex("fp16x2", PER_CLIP, st.R, 1))
    assert rc == 0
    for k in range(5):
        assert torch.equal(a[k], b[k]), k
    for prec, flags, stride, rows in (("fp16x2", PER_CLIP, st.R, block[:, 0]), ("fp16x2", 0, 0, None), ("fp32", PER_CLIP, st.R, block[:, 0])):
        outs = []
        for fr in (None, (0, 0, 0), (0, 3, 1)):                # hop == 0: the other two fields are not read
            st.frames = fr
            rc, o = st.fwd(dev(btc(x)), None if rows is None else dev(rows), _ex(prec, flags, stride, 1))
            assert rc == 0, _lib.lib().wn_last_error()
            outs.append(o)
        for o in outs[1:]:
            for k in range(5):
                assert torch.equal(outs[0][k], o[k]), (prec, flags, k)
    st.frames = frames


# ---- bias-gradient rows ----------------------------------------------------------------------------------------------------
def _grad_rows(st, x, block, prec, flags, t_off=21, seed=100, start=0.25):
    Bn, Tn = x.shape[0], x.shape[3]
    rs = np.random.RandomState(seed)
    dout = rs.standard_normal((Bn, st.Cr, 1, Tn)).astype(np.float32)
    dskip = rs.standard_normal((Bn, st.Cs, 1, Tn - t_off)).astype(np.float32)
    n, rw = block.shape[1], block.shape[2]
    xd, bd = dev(btc(x)), dev(block)
    ex = lambda: _ex(prec, flags | PER_CLIP, n * rw, 1)
    rc, acts = st.fwd(xd, bd, ex(), t_off)
    assert rc == 0, _lib.lib().wn_last_error()
    grad = torch.full((Bn, n, rw), start, device="cuda")        # gradients ACCUMULATE: the rows start from a value
    rc, dx, gW, ws = st.bwd_ws(xd, acts, dev(btc(dout)), dev(btc(dskip)), grad, ex(), t_off)
    assert rc == 0, _lib.lib().wn_last_error()
    return grad, ws, dout, dskip, dx, gW


def _grad_rows_against_reference(st, x, block, prec, flags, hop=LR.HOP, phase=LR.PHASE):
    grad, ws, dout, dskip, _, _ = _grad_rows(st, x, block, prec, flags)
    want = LR.stack_row_grads(st.p, st.w, x, block[:, :, :st.R], hop, phase, dout, dskip, 21)
    got = to_np(grad)[:, :, :st.R] - 0.25
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("per-frame bias gradient rows (%s, flags %d): max |row - float64 reference| = %.3g of %.3g" % (prec, flags, err, scale))
    assert scale > 1e-2 and np.abs(want[0] - want[1]).max() > 1e-3 and np.abs(want[:, 0] - want[:, 1]).max() > 1e-3
    assert err <= 2e-4 * scale, (err, scale)
    return grad, ws


def _segments(Tn, hop, phase, Z):
    """[(frame, first row, end row)] of the frames that hold a row >= Z."""
    out = []
    for f in range(LR.frames_needed(Tn, hop, phase)):
        ta, tb = max(Z, f * hop - phase), min(Tn, (f + 1) * hop - phase)
        if tb > ta:
            out.append((f, ta, tb))
    return out


@pytest.mark.parametrize("flags", [GENERIC, 0])
def test_bias_gradient_rows_in_the_documented_order(flags):
    """wn_stack_bwd with per-frame rows at TINY.  Every layer's rows against the float64 reference gradient (2e-4 of the
    block's largest entry).  Layer 0 -- whose (da | dg) scratch is what the workspace still holds when the call returns --
    against sums of that scratch over each frame's rows: under WN_EXEC_FORCE_GENERIC bit-equal to float32 sums formed on the
    host in the documented order; on the fused path within the running-sum bound of
    test_per_clip_bias_gradient_rows_on_the_fused_path with n the segment length, 2 n^2 u max|x|.  The padding behind a row
    stays untouched, and two runs give identical bits."""
    st, x, block = _case(seed=7, pad=4)
    grad, ws = _grad_rows_against_reference(st, x, block, "fp32", flags)
    grad2, _, _, _, _, _ = _grad_rows(st, x, block, "fp32", flags)
    assert torch.equal(grad, grad2)
    assert float((grad[:, :, st.R:] - 0.25).abs().max()) == 0.0
    zoff = B * T * st.ncd
    dab = to_np(ws[zoff:zoff + B * T * 64]).reshape(B, T, 64)
    got = to_np(grad)
    of, og, cd = st.rows[0]
    for b in range(B):
        for f, ta, tb in _segments(T, LR.HOP, LR.PHASE, 0):
            row = np.concatenate([got[b, f, of:of + cd], got[b, f, og:og + cd]])
            if flags == GENERIC:
                want = np.float32(0.25) + LR.colsum_in_kernel_order(dab[b], ta, tb)
                assert np.array_equal(row, want), (b, f)
            else:
                want = 0.25 + dab[b, ta:tb].astype(np.float64).sum(0)
                n = tb - ta
                assert np.abs(row - want).max() <= 2 * n * n * U32 * np.abs(dab[b, ta:tb]).max() + U32, (b, f)


def test_rows_of_frames_wholly_below_the_zero_prefix_stay_untouched():
    """hop = 1: frames 0 and 1 of the d = 4 layers (Z = 2) hold no row that counts; their gradient rows keep the value they
    had, on the generic and on the fused path, and every other row moves."""
    st, x, block = _case(seed=8, hop=1, phase=0)
    for flags in (GENERIC, 0):
        grad, _, _, _, _, _ = _grad_rows(st, x, block, "fp32", flags, start=0.5)
        g = to_np(grad)
        for l, (of, og, cd) in enumerate(st.rows):
            Z = R.conv_pad_and_prefix(T, st.dil[l], 2)[1]
            lay = np.concatenate([g[:, :, of:of + cd], g[:, :, og:og + cd]], axis=2)
            assert np.all(lay[:, :Z] == 0.5), (flags, l)
            assert np.all(np.abs(lay[:, Z:] - 0.5).max(axis=2) > 0), (flags, l)


def test_a_segment_longer_than_one_chunk():
    """hop = 600, T = 1,300, B = 2, one layer: segments of 600 rows are three chunks of 256 (the last ragged) on three
    reduction lanes, the last segment (100 rows) a single ragged chunk.  Generic path, bit-equal to the host order."""
    over = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[24], residual_num_blocks=1,
                softmax_conv_channels=[64, 256])
    Bn, Tn, hop = 2, 1300, 600
    st, x, block = _case(over, seed=9, hop=hop, phase=0, pad=2, Bn=Bn, Tn=Tn)
    assert block.shape[1] == 3 and st.frames[2] == 50
    grad, ws, _, _, _, _ = _grad_rows(st, x, block, "fp32", 0)
    grad2, _, _, _, _, _ = _grad_rows(st, x, block, "fp32", 0)
    assert torch.equal(grad, grad2)
    zoff = Bn * Tn * st.ncd
    dab = to_np(ws[zoff:zoff + Bn * Tn * 48]).reshape(Bn, Tn, 48)
    got = to_np(grad)
    for b in range(Bn):
        for f, ta, tb in _segments(Tn, hop, 0, 0):
            want = np.float32(0.25) + LR.colsum_in_kernel_order(dab[b], ta, tb)
            assert np.abs(want - 0.25).max() > 1.0
            assert np.array_equal(got[b, f, :48], want), (b, f)
    assert float((grad[:, :, 48:] - 0.25).abs().max()) == 0.0


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_bad_frame_geometry_is_refused_before_any_device_work():
    st, x, block = _case(seed=10)
    n, rw = block.shape[1], block.shape[2]
    xd, bd = dev(btc(x)), dev(block)
    lib = _lib.lib()

    def refused(frames, prec, flags, stride, word, bias=bd):
        st.frames = frames
        rc, out = st.fwd(xd, bias, _ex(prec, flags, stride, 1))
        msg = lib.wn_last_error()
        assert rc == _lib.WN_EARG and word in msg, (frames, msg)
        assert all(float(o.abs().max()) == 0.0 for o in out), frames
        grad = torch.full_like(bias, 0.5)
        acts = tuple(torch.ones_like(o) for o in out)
        rc, dx, gW = st.bwd(xd, acts, torch.ones_like(xd), None, grad, _ex(prec, flags, stride, 1))
        assert rc == _lib.WN_EARG and word in lib.wn_last_error(), frames
        assert float(dx.abs().max()) == 0.0 and float((grad - 0.5).abs().max()) == 0.0

    refused((-1, 0, rw), "fp32", PER_CLIP, n * rw, b"bias_hop")
    refused((12, 12, rw), "fp32", PER_CLIP, n * rw, b"bias_phase")
    refused((12, -1, rw), "fp32", PER_CLIP, n * rw, b"bias_phase")
    refused((12, 5, 31), "fp32", PER_CLIP, n * rw, b"bias_frame_stride")
    refused((12, 5, rw), "fp32", PER_CLIP, n * rw - 1, b"reserved")
    refused((12, 5, rw), "fp32", 0, n * rw, b"without WN_EXEC_BIAS_PER_CLIP")
    # the fp16 x 2 kernels load a lane's values as float4: a frame stride of R + 2 floats is refused, not sent down another path
    wide = torch.zeros((B, n, rw + 2), device="cuda")
    st.frames = (12, 5, rw + 2)
    rc, out = st.fwd(xd, wide, _ex("fp16x2", PER_CLIP, n * (rw + 2), 1))
    assert rc == _lib.WN_EARG and b"multiple of 4" in lib.wn_last_error() and float(out[0].abs().max()) == 0.0
    rc, out = st.fwd(xd, wide, _ex("fp32", PER_CLIP, n * (rw + 2), 1))          # the exact-fp32 kernels take any stride
    assert rc == 0


# ---- the locally conditioned model ------------------------------------------------------------------------------------------
def _model(cls=WaveNet, seed=1234, glob=False, local_seed=77, hop=LR.HOP):
    p = R.make_params(**LR.TINY)
    w = R.init_weights(p, seed)
    V, h = LR.init_local(p, seed=local_seed)
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    net = cls(Params(p), seed=0, local_channels=LR.FEATS, local_hop=hop, **kw)
    net.load_state_dict(LR.state_dict(w, V, E, Vg))
    net.to_gpu()
    return p, w, V, h, E, Vg, net


_BATCH = {}


def _batch(glob=False):
    """The tiny batch and its CPU reference, computed once and shared (read-only)."""
    if glob not in _BATCH:
        p = R.make_params(**LR.TINY)
        w = R.init_weights(p, 1234)
        V, h = LR.init_local(p)
        E, Vg = cond_ref.init_condition(p) if glob else (None, None)
        rs = np.random.RandomState(8)
        tw = 40
        idx = rs.randint(0, 256, (B, T)).astype(np.int32)
        tgt = rs.randint(0, 256, (B, tw)).astype(np.int32)
        ref = LR.train_step_grads(p, w, V, h, LR.HOP, LR.PHASE, idx, tgt, E=E, Vg=Vg, ids=cond_ref.IDS if glob else None)
        _BATCH[glob] = dict(idx=idx, tgt=tgt, tw=tw, ref=ref, h=h)
    return _BATCH[glob]


@pytest.mark.parametrize("prec,t1,glob", [("fp32", None, False), ("fp16x2", 1, False), ("fp16x2", None, False),
                                          ("fp32", None, True), ("fp16x2", 1, True)])
def test_locally_conditioned_loss_logits_and_every_gradient_against_the_reference(prec, t1, glob):
    """Loss, logits and the gradient of every weight -- ``local_condition_projection/W`` included -- and of the features,
    which require grad here, against tests/local_cond_ref.py: exact fp32 and the default arithmetic (with the per-frame
    kernels, fwd_t1_min_blocks = 1, and as the library dispatches this size by itself), at the tolerances of
    test_conditioned_loss_logits_and_every_gradient_against_the_reference (1e-4 on loss and logits, 2e-4 of a tensor's
    largest entry on gradients).  Once more with global conditioning also on: the clip's row joins every frame row."""
    p, w, V, h, E, Vg, net = _model(glob=glob)
    net.gemm_precision = prec
    net.fwd_t1_min_blocks = t1
    bt = _batch(glob)
    loss_ref, logits_ref, g = bt["ref"]
    tw = bt["tw"]
    feats = dev(h).requires_grad_(True)
    kw = dict(local=feats, local_phase=LR.PHASE)
    if glob:
        kw["condition"] = cond_ref.IDS
    c = net.forward_causal_block(bt["idx"])
    _, s = net.forward_residual_block(c, t_off=T - tw, **kw)
    lg = net.forward_softmax_block(s, apply_softmax=False)
    loss = net.cross_entropy(lg, bt["tgt"])
    net.zero_grads()
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - loss_ref) < 1e-4
    np.testing.assert_allclose(to_np(lg), logits_ref, atol=ATOL)
    names = {"global_condition_embed": "E", "global_condition_projection": "Vg", "local_condition_projection": "V"}
    seen = set()
    for ln, kind, off, n, shape in net._spans:
        name = names.get(ln.name, "%s/%s" % (ln.name, kind))
        seen.add(name)
        want = g[name].reshape(shape)
        got = to_np(net._grad_arena[off:off + n].view(shape))
        scale = max(np.abs(want).max(), 1e-6)
        assert np.abs(got - want).max() <= 2e-4 * scale + 1e-7, (ln.name, kind, np.abs(got - want).max(), scale)
    assert "V" in seen and np.abs(g["V"]).max() > 1e-4
    gh = to_np(feats.grad)
    scale = np.abs(g["h"]).max()
    assert scale > 1e-5 and np.abs(gh - g["h"]).max() <= 2e-4 * scale + 1e-7, (np.abs(gh - g["h"]).max(), scale)
    l2 = default_loss(net, dev(bt["idx"]), dev(bt["tgt"]), **dict(kw, local=dev(h)))
    assert abs(float(l2.detach()) - float(loss.detach())) < 1e-5 * max(1.0, abs(loss_ref)) + 2e-6


def test_a_locally_conditioned_model_needs_features_and_another_refuses_them():
    p, w, V, h, _, _, net = _model()
    bt = _batch()
    x = dev(bt["idx"])
    with pytest.raises(Exception, match="pass local="):
        net.forward_one_step(x)
    with pytest.raises(Exception, match="pass local="):
        net.token_nll(x, dev(bt["tgt"]))
    with pytest.raises(Exception, match="feature columns"):
        net.forward_one_step(x, local=h[:, :, :6], local_phase=LR.PHASE)
    with pytest.raises(Exception, match="forward_residual_block"):
        net.residual_blocks[0][0](net.forward_causal_block(x))
    net.forward_one_step(x, local=np.concatenate([h, h], axis=2), local_phase=LR.PHASE)      # surplus columns are ignored
    plain = WaveNet(Params(p), seed=0)
    plain.to_gpu()
    with pytest.raises(Exception, match="no local conditioning"):
        plain.forward_one_step(x, local=h)
    with pytest.raises(Exception, match="no local conditioning"):
        TrainStepGraph(plain, x, dev(bt["tgt"]), local=h)


def test_train_step_graph_replays_a_locally_conditioned_step_and_follows_the_feature_buffer():
    """Three replayed locally conditioned steps land on the weights of three op-by-op steps (2e-5, Adam's eps raised, as in
    the conditioned-graph test), the features changing between replays; the step runs WITH the step plan; the same batch under
    other features gives another loss and under the first ones the first loss again; two captures give identical bits."""
    _, _, _, _, _, _, eager = _model()
    nets = [_model()[-1] for _ in range(2)]
    for n in [eager] + nets:
        n.update_laerning_rate(0.01)
        n.optimizer.eps = 1e-3
    iw = eager.input_width
    rs = np.random.RandomState(0)
    nf = LR.frames_needed(T, LR.HOP, LR.PHASE)
    batches = [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, T - iw)).astype(np.int32)),
                dev(rs.standard_normal((B, LR.FEATS, nf)).astype(np.float32))) for _ in range(3)]
    w0 = to_np(nets[0]._arena).copy()
    graphs = [TrainStepGraph(n, batches[0][0], batches[0][1], local=batches[0][2], local_phase=LR.PHASE) for n in nets]
    np.testing.assert_array_equal(to_np(nets[0]._arena), w0)          # capture + warm-up did not train
    if nets[0].use_step_plan:
        assert nets[0].plan_stats()["state"] == 2                     # a locally conditioned step runs WITH the step plan
    for x, tg, ft in batches:
        eager.backprop(default_loss(eager, x, tg, local=ft, local_phase=LR.PHASE))
        losses = [float(g.step(x, tg, local=ft)) for g in graphs]
        assert np.isfinite(losses[0]) and losses[0] == losses[1]
    a, b = to_np(eager._arena), to_np(nets[0]._arena)
    assert np.abs(a - w0).max() > 1e-3
    np.testing.assert_allclose(b, a, atol=2e-5)
    assert torch.equal(nets[0]._arena, nets[1]._arena)                 # two captures: identical bits
    g, net = graphs[0], nets[0]
    x, tg, ft = batches[0]
    la = float(g.step(x, tg, local=ft))
    with torch.no_grad():
        net._arena.copy_(torch.as_tensor(b).cuda())                   # the loss of a step is that of the weights it starts from
    lb = float(g.step(x, tg, local=batches[1][2]))
    with torch.no_grad():
        net._arena.copy_(torch.as_tensor(b).cuda())
    lc = float(g.step(x, tg, local=ft))
    assert la == lc and abs(la - lb) > 1e-4, (la, lb, lc)
    with pytest.raises(_lib.WaveNetHipError, match="captured with phase"):
        g.step(x, tg, local=ft, local_phase=0)


def test_checkpoints_and_the_weight_average_carry_the_local_projection(tmp_path):
    """save / load and wavenet.ema.npz round-trip the new tensor, and ema_weights() swaps it like every weight."""
    _, _, _, h, _, _, net = _model()
    net.enable_ema(0.5, warmup=False)
    net.update_laerning_rate(0.01)
    bt = _batch()
    x, tgt, ft = dev(bt["idx"]), dev(bt["tgt"]), dev(h)
    kw = dict(local=ft, local_phase=LR.PHASE)
    for _ in range(2):
        net.backprop(default_loss(net, x, tgt, **kw))
    sd, ema = net.state_dict(), net.ema_state_dict()
    k = "local_condition_projection/W"
    assert np.abs(sd[k] - ema[k]).max() > 0                           # the average lags the iterate
    with net.ema_weights():
        inside = net.state_dict()
        loss_avg = float(default_loss(net, x, tgt, **kw).detach())
    assert np.array_equal(inside[k], ema[k]) and np.array_equal(net.state_dict()[k], sd[k])
    net.save(str(tmp_path))
    other = _model(seed=5, local_seed=6)[-1]
    other.enable_ema(0.5, warmup=False)
    other.load(str(tmp_path))
    assert np.array_equal(other.state_dict()[k], sd[k]) and np.array_equal(other.ema_state_dict()[k], ema[k])
    avg = _model(seed=5, local_seed=6)[-1]
    avg.load(str(tmp_path), weights="ema")
    assert abs(float(default_loss(avg, x, tgt, **kw).detach()) - loss_avg) <= 1e-6 * max(1.0, abs(loss_avg))


# ---- the decoder -----------------------------------------------------------------------------------------------------------
from test_gpu_condition import _biased_twin as _twin_with       # noqa: E402  (an ordinary biased FasterWaveNet from [(bf, bg)])
from wavenet_amd import FasterWaveNet                           # noqa: E402
from wavenet_amd._lib import check, ptr_array                   # noqa: E402

DHOP = 5


class _Dec(object):
    """Decoder handles of a locally conditioned FasterWaveNet and of its biased twin, all seeded from ONE prefill state."""

    def __init__(self):
        self.p, self.w, self.V, _, _, _, self.net = _model(cls=FasterWaveNet, hop=DHOP)
        rs = np.random.RandomState(21)
        self.h = rs.standard_normal((LR.FEATS, 6)).astype(np.float32)
        self.rows = self.net.local_biases(self.h)                               # (6, R) on the device
        self.R = int(self.rows.shape[1])
        self.Q = 256
        self.tok = dev(rs.randint(0, 256, (1, self.net.input_width)).astype(np.int32))
        self.handles = []

    def twin(self, row):
        """A biased FasterWaveNet whose static gate biases are ``row`` (R,)."""
        net = self.net
        net.condition_biases = lambda c: [(row[of:of + lay.cd].clone(), row[og:og + lay.cd].clone())
                                          for lay, (of, og) in zip(net._flat_layers, net._cond_offsets)]
        try:
            return _twin_with(self.p, self.w, net, 0)
        finally:
            del net.condition_biases

    def seed(self, model, handle, state_from):
        """Load the rings of ``handle`` from the prefill ``state_from`` (a biased twin) ran over self.tok."""
        check(_lib.lib().wn_decoder_load_state(handle, ptr(self.tok), int(self.tok.shape[1]),
                                               ptr_array([t.contiguous() for t in state_from._last_causal_outputs]),
                                               ptr_array(state_from._last_layer_inputs), None), "wn_decoder_load_state")

    def handle(self, model, state_from, table=None):
        d, keep = model._desc(None, table)
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        self.seed(model, h, state_from)
        return h

    def run(self, h, n, u, first=7):
        out = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        probs = torch.zeros((n, self.Q), device="cuda")
        rc = _lib.lib().wn_decoder_run(h, first, ptr(u), n, ptr(out), ptr(probs), None)
        torch.cuda.synchronize()
        return rc, out, probs

    def close(self):
        for h in self.handles:
            _lib.lib().wn_decoder_destroy(h)


def test_decoder_frame_table_through_the_c_abi():
    """(a) A table whose rows all equal r decodes -- tokens and probability trace -- bit for bit as the biased model with
    static biases r (rows 4 floats of padding apart).  (b) Two distinct rows, hop 5, phase 2, 12 steps: steps 0 .. 2 read row
    0 and equal the biased model with row 0 bit for bit; step 3 reads row 1 and differs.  (d) wn_decoder_step fed the run's
    tokens gives the run's probability rows bit for bit.  (f) A run past the last row is refused before any device work and
    leaves the handle as it was: the 13 steps the table does cover then equal those of a fresh handle."""
    D = _Dec()
    try:
        lib = _lib.lib()
        u = dev(np.random.RandomState(5).random_sample(16))
        r0, r1 = D.rows[0].contiguous(), D.rows[1].contiguous()
        assert float((r0 - r1).abs().max()) > 0.1
        tw0 = D.twin(r0)
        with torch.no_grad():
            tw0.forward_one_step(D.tok)                                          # the one prefill every handle is seeded from
        rc, t_ref, p_ref = D.run(D.handle(tw0, tw0), 12, u)
        assert rc == 0
        # (a)
        same = torch.zeros((4, D.R + 4), device="cuda")
        same[:, :D.R] = r0
        rc, t_a, p_a = D.run(D.handle(D.net, tw0, (same, DHOP, 2)), 12, u)
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(t_a, t_ref) and torch.equal(p_a, p_ref)
        # (b)
        two = torch.stack([r0, r1, r1]).contiguous()
        hb = D.handle(D.net, tw0, (two, DHOP, 2))
        rc, t_b, p_b = D.run(hb, 12, u)
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(p_b[:3], p_ref[:3]) and torch.equal(t_b[:3], t_ref[:3])
        assert not torch.equal(p_b[3], p_ref[3])
        # (d) the same table, one wn_decoder_step per token
        hd = D.handle(D.net, tw0, (two, DHOP, 2))
        feed = [7] + [int(t) for t in t_b[:-1].cpu()]
        row = torch.zeros((D.Q,), device="cuda")
        for k, tk in enumerate(feed):
            check(lib.wn_decoder_step(hd, tk, ptr(row), 1, None), "wn_decoder_step")
            torch.cuda.synchronize()
            assert torch.equal(row, p_b[k]), k
        # (f) 3 rows at hop 5 from phase 2 cover 13 steps; hb has run 12 of them
        rc, t_f, p_f = D.run(hb, 2, u)
        assert rc == _lib.WN_EARG and b"frame table of 3 rows" in lib.wn_last_error()
        assert int(t_f.min()) == -1 and float(p_f.abs().max()) == 0.0            # nothing ran
        rc = lib.wn_decoder_step(hd, 3, ptr(row), 1, None)
        assert rc == 0
        rc = lib.wn_decoder_step(hd, 3, ptr(row), 1, None)
        assert rc == _lib.WN_EARG and b"frame table" in lib.wn_last_error()
        fresh = D.handle(D.net, tw0, (two, DHOP, 2))
        rc, t_13, p_13 = D.run(fresh, 13, u)
        assert rc == 0
        rc, t_last, p_last = D.run(hb, 1, u[12:], first=int(t_b[11]))
        assert rc == 0 and torch.equal(p_last[0], p_13[12]) and torch.equal(t_13[:12], t_b)
        # a table is refused where its geometry is wrong, and an update without one drops it
        for tab, word in (((two, 0, 0), b"frame_hop"), ((two, DHOP, DHOP), b"frame_phase")):
            d, keep = D.net._desc(None, tab)
            assert lib.wn_decoder_update_weights(fresh, C.byref(d), None) == _lib.WN_EARG and word in lib.wn_last_error()
        d, keep = D.net._desc(None, (two, DHOP, 2))
        d.frame_stride = D.R - 1
        assert lib.wn_decoder_update_weights(fresh, C.byref(d), None) == _lib.WN_EARG and b"frame_stride" in lib.wn_last_error()
    finally:
        D.close()


def test_decoded_trace_agrees_with_the_teacher_forced_forward():
    """(c) hop 5, 40 decoded steps behind the prefill: row i of generate()'s probability trace agrees within ATOL with the
    model's own forward -- the ELU head the decoder uses -- over the window and the emitted tokens with the same features.
    (The window is 16 positions and the whole sequence 56: both multiples of every dilation, so the two forwards share one
    zero-prefix pattern.)  Generating past the features raises before anything runs."""
    p, w, V, _, _, _, net = _model(cls=FasterWaveNet, hop=DHOP)
    n = 41
    W = net.input_width
    assert W == 16
    rs = np.random.RandomState(31)
    h = rs.standard_normal((LR.FEATS, LR.frames_needed(W + n - 1, DHOP, 3))).astype(np.float32)
    u = rs.random_sample(n)
    prompt = rs.randint(0, 256, (W,)).astype(np.int32)
    toks, probs = net.generate(n, u, initial_tokens=prompt, return_probs=True, local=h, local_phase=3)
    full = np.concatenate([prompt, to_np(toks)[:-1]])[None]
    with torch.no_grad():
        c = net.forward_causal_block(dev(full))
        _, s = WaveNet.forward_residual_block(net, c, local=dev(h[None]), local_phase=3)
        ref = net.forward_softmax_block(s, apply_softmax=True, activation="elu")
    ref = to_np(ref)[0, :, 0, :].T                                   # (W + n - 1, Q); column W - 1 + i predicts token i
    np.testing.assert_allclose(to_np(probs)[1:], ref[W:], atol=ATOL)
    other = net.generate(n, u, initial_tokens=prompt, local=h[:, ::-1].copy(), local_phase=3)
    assert not torch.equal(other, toks)                               # the features steer the samples
    with pytest.raises(Exception, match="cover fewer samples"):
        net.generate(n + 5, np.concatenate([u, u]), initial_tokens=prompt, local=h, local_phase=3)
    with pytest.raises(Exception, match="pass local="):
        net.generate(4, u)


def test_generate_batch_with_a_table_and_a_phase_per_utterance_equals_the_single_runs():
    """(e) Three utterances with different features and phases: row u of generate_batch is generate() with utterance u's
    features and phase, bit for bit; one array for all utterances likewise."""
    p, w, V, _, _, _, net = _model(cls=FasterWaveNet, hop=DHOP)
    n = 24
    W = net.input_width
    rs = np.random.RandomState(41)
    u = rs.random_sample((3, n))
    phases = [0, 3, 4]
    hs = [rs.standard_normal((LR.FEATS, LR.frames_needed(W + n - 1, DHOP, ph) + k)).astype(np.float32) for k, ph in enumerate(phases)]
    singles = [net.generate(n, u[i], local=hs[i], local_phase=phases[i]) for i in range(3)]
    assert len({tuple(to_np(t)) for t in singles}) == 3
    rows = net.generate_batch(n, u, local=hs, local_phase=phases)
    for i in range(3):
        assert torch.equal(rows[i], singles[i]), i
    shared = net.generate_batch(n, u, local=hs[1], local_phase=3)
    assert torch.equal(shared[1], singles[1])
    with pytest.raises(Exception, match="2 feature arrays for 3 utterances"):
        net.generate_batch(n, u, local=hs[:2])
    with pytest.raises(Exception, match="cover fewer samples"):
        net.generate_batch(n, u, local=[hs[0], hs[1], hs[2][:, :3]], local_phase=phases)


# ---- scoring ---------------------------------------------------------------------------------------------------------------
def test_locally_conditioned_scoring():
    """The mean of token_nll(local=) is the training loss of the same window (1e-5 relative, the agreement the conditioned
    scoring test uses); score() does not change with batch_size or with a chunk_width of another multiple of the hop beyond
    the arithmetic of the default precision's tile scales (tests/test_gpu_scoring.py's bound for the same comparison is
    used), changes with the features, and refuses a chunk_width that is no multiple of the hop."""
    _, _, _, h, _, _, net = _model()
    bt = _batch()
    x, tgt, ft = dev(bt["idx"]), dev(bt["tgt"]), dev(h)
    want = float(default_loss(net, x, tgt, local=ft, local_phase=LR.PHASE).detach())
    rows = net.token_nll(x, tgt, local=ft, local_phase=LR.PHASE)
    assert rows.shape == tuple(bt["tgt"].shape) and not rows.requires_grad
    mean = float(to_np(rows).astype(np.float64).mean())
    assert abs(mean - want) <= 1e-5 * abs(want), (mean, want)
    rs = np.random.RandomState(51)
    toks = rs.randint(0, 256, (200,)).astype(np.int32)
    f = rs.standard_normal((LR.FEATS, LR.frames_needed(200, LR.HOP))).astype(np.float32)
    net.gemm_precision = "fp32"                                        # exact arithmetic: the cut may not move a value beyond rounding
    a = net.score(toks, chunk_width=48, batch_size=2, local=f)
    b = net.score(toks, chunk_width=96, batch_size=8, local=f)
    c = net.score(toks, chunk_width=48, batch_size=1, local=f)
    assert a.shape == (200,)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) and float((a - c).abs().max()) <= 1e-5 * float(a.abs().max())
    other = net.score(toks, chunk_width=48, batch_size=2, local=-f)
    assert float((a - other).abs().max()) > 1e-3
    with pytest.raises(Exception, match="chunk_width % local_hop == 0"):
        net.score(toks, chunk_width=50, local=f)
    with pytest.raises(Exception, match="pass local="):
        net.score(toks, chunk_width=48)
    with pytest.raises(Exception, match="feature columns"):
        net.score(toks, chunk_width=48, local=f[:, :5])


# ---- the command line end to end: wavs -> features -> locally conditioned training -> generation from features -> scores ----
def test_cli_features_train_generate_evaluate(tmp_path):
    import json
    from scipy.io import wavfile
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import features as cli_features
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import local as cli_local
    from wavenet_amd.train_audio import train as cli_train
    wav, feat, model = tmp_path / "wav", tmp_path / "feat", tmp_path / "model"
    wav.mkdir()
    model.mkdir()
    sr = 8000
    t = np.arange(sr) / sr
    for name, hz in (("a.wav", 220), ("b.wav", 330), ("p225_c.wav", 440)):          # three short synthetic wavs
        wavfile.write(str(wav / name), sr, (0.5 * np.sin(2 * np.pi * hz * t) * 32767).astype(np.int16))
    written = cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "64", "--mels", "12", "--win", "256"])
    assert [os.path.basename(f) for f in written] == ["a.npy", "b.npy", "p225_c.npy"]
    fa = np.load(str(feat / "a.npy"))
    assert fa.shape[0] == 12 and fa.dtype == np.float32 and abs(fa.shape[1] - sr // 64) <= 1
    cfg = {"quantization_steps": 256, "sampling_rate": sr, "causal_conv_channels": [32], "residual_conv_channels": [32] * 4,
           "residual_num_blocks": 2, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
    (model / "wavenet.json").write_text(json.dumps(cfg))
    common = ["-w", str(wav), "-m", str(model), "--seed", "1"]
    loop = ["--lr", "0.003", "--batch-size", "4", "--train-width", "256", "--repeat", "30", "--max-epoch", "2"]
    l1 = cli_train.main(common + loop + ["--local-dir", str(feat), "--local-hop", "64"])
    assert cli_local.load_config(str(model)) == (12, 64)
    assert json.loads((model / "wavenet.json").read_text()) == cfg           # wavenet.json is unchanged
    with np.load(str(model / "wavenet.model.npz")) as z:
        assert z["local_condition_projection/W"].shape == (512, 12, 1, 1)
    l2 = cli_train.main(common + loop + ["--local-dir", str(feat), "--no-graph"])    # resumed: the hop comes from local.json
    assert np.isfinite(l1) and np.isfinite(l2) and l2 < l1, (l1, l2)
    with pytest.raises(SystemExit, match="give --local-dir"):
        cli_train.main(common + loop)
    out = str(tmp_path / "gen")
    short = str(tmp_path / "short.npy")
    np.save(short, fa[:, :4])                                               # 256 samples of features: the 32-sample window + 224 steps
    fn, one = cli_generate.main(["-m", str(model), "-o", out, "--fast", "--seed", "2", "--local", short])
    assert one.shape == (4 * 64 - 32 + 1,) and one.min() >= 0 and one.max() < 256   # the length the features cover
    fns, tokens = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.02", "--fast", "--seed", "2", "--utterances", "2",
                                     "--local", short, "--local", str(feat / "b.npy")])
    assert len(fns) == 2 and tokens.shape == (2, int(sr * 0.02) - 1) and tokens.min() >= 0 and tokens.max() < 256
    fn2, slow = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.003", "--seed", "2", "--local", short])
    assert slow.shape == (int(sr * 0.003) - 1,) and slow[0] == one[0]       # the slow path draws the same first sample
    with pytest.raises(SystemExit, match="the features cover"):
        cli_generate.main(["-m", str(model), "-o", out, "-s", "0.5", "--fast", "--local", short])
    with pytest.raises(SystemExit, match="the features cover"):           # an explicit -s is a length like any other, 1.0 included
        cli_generate.main(["-m", str(model), "-o", out, "-s", "1.0", "--fast", "--local", short])
    with pytest.raises(SystemExit, match="give --local FILE.npy"):
        cli_generate.main(["-m", str(model), "-o", out, "--fast"])
    table = cli_evaluate.main(["-w", str(wav), "-m", str(model), "--local-dir", str(feat)])
    assert [r["file"] for r in table["files"]] == ["a.wav", "b.wav", "p225_c.wav"]
    assert all(np.isfinite(r["nats_per_sample"]) and r["samples"] > 0 for r in table["files"])
    with pytest.raises(SystemExit, match="give --local-dir"):
        cli_evaluate.main(["-w", str(wav), "-m", str(model)])
    os.remove(str(feat / "b.npy"))
    with pytest.raises(SystemExit, match=r"b\.npy is missing"):
        cli_evaluate.main(["-w", str(wav), "-m", str(model), "--local-dir", str(feat)])
