"""Linear interpolation between feature frames on the GPU (WnStackDesc.bias_interp / WnDecoderDesc.frame_interp = 1,
``local_interp="linear"``) against the float64 reference of tests/local_interp_ref.py and, bit for bit, against the per-clip
and repeat forms where the rule makes them equal: rows that are equal within a clip, and hop 1 (alpha = 0 everywhere).

The base case is local_cond_ref's: cond_ref.TINY, B = 3, T = 70, hop 12, phase 5 -- 7 frames, so 8 rows per clip, frame
borders inside 32-column tiles.  Every tolerance is the one tests/test_gpu_local_condition.py (or, for bf16x3 / bf16 on the
whole model, tests/test_gpu_condition.py) uses for the same path and precision."""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
import local_interp_ref as LI
from gpu_util import btc, dev, to_np
from oracle import wavenet_ref as R
from test_gpu_condition import _biased_twin, _ex, _split_z
from test_gpu_local_condition import ATOL, PATHS, _FrameStack, _grad_rows
from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, WaveNet, _lib
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.graph import default_loss

pytestmark = pytest.mark.gpu

PER_CLIP = _lib.WN_EXEC_BIAS_PER_CLIP
GENERIC = _lib.WN_EXEC_FORCE_GENERIC
B, T = LI.B, LI.T
WIDE = [(64, 32), (128, 128)]               # test_per_frame_rows_on_the_wide_path's shapes: wn_layer_fast_path is 0


def _wide(Cr, cd):
    return dict(quantization_steps=256, causal_conv_channels=[Cr], residual_conv_channels=[cd] * 3, residual_num_blocks=1,
                softmax_conv_channels=[64, 256])


# ---- the residual stack through the C ABI ---------------------------------------------------------------------------------
class _LerpStack(_FrameStack):
    """_FrameStack with the mode field; ``interp`` is written whenever ``frames`` is."""
    interp = 1

    def desc(self, bias=None):
        d, keep = super().desc(bias)
        if self.frames is not None:
            d.bias_interp = self.interp
        return d, keep


def _case(over=LI.TINY, seed=0, hop=LI.HOP, phase=LI.PHASE, bias_scale=0.5, pad=0, Bn=B, Tn=T):
    """Stack, input (B, Cr, 1, T) and a (B, frames + 1, R + pad) block of random rows that differ by clip and frame."""
    st = _LerpStack(over)
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((Bn, st.Cr, 1, Tn)).astype(np.float32)
    n = LI.frames_needed(Tn, hop, phase)
    block = (rs.standard_normal((Bn, n, st.R + pad)) * bias_scale).astype(np.float32)
    st.frames = (hop, phase, st.R + pad)
    return st, x, block


def _run(st, x, block, prec, flags, t1, t_off=0, window_only=0):
    n, rw = block.shape[1], block.shape[2]
    rc, got = st.fwd(dev(btc(x)), dev(block), _ex(prec, flags | PER_CLIP, n * rw, t1), t_off, window_only)
    assert rc == 0, _lib.lib().wn_last_error()
    return got


def _against_reference(st, x, block, hop, phase, got, t_off=0):
    Bn, Tn = x.shape[0], x.shape[3]
    layers, skip, _ = LI.stack_forward(st.p, st.w, x, block[:, :, :st.R], hop, phase)
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL, err_msg="out %d" % l)
        for k in (1, 2, 3):
            np.testing.assert_allclose(to_np(_split_z(st, got[k], Bn, Tn)[l]), btc(layers[l][k]), atol=ATOL,
                                       err_msg="%s %d" % (("z", "tanh", "sigmoid")[k - 1], l))
    np.testing.assert_allclose(to_np(got[4]), btc(skip)[:, t_off:], atol=ATOL)


def _grad_rows_against_reference(st, x, block, prec, flags, hop=LI.HOP, phase=LI.PHASE):
    """dbf / dbg blocks of wn_stack_bwd against the float64 reference gradient within 2e-4 of the block's largest entry (the
    bound test_gpu_local_condition.py puts on the same rows), and two runs give identical bits."""
    grad, _, dout, dskip, _, _ = _grad_rows(st, x, block, prec, flags)
    grad2 = _grad_rows(st, x, block, prec, flags)[0]
    assert torch.equal(grad, grad2)
    want = LI.stack_row_grads(st.p, st.w, x, block[:, :, :st.R], hop, phase, dout, dskip, 21)
    got = to_np(grad)[:, :, :st.R] - 0.25
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("interpolated bias gradient rows (%s, flags %d, hop %d): max |row - float64 reference| = %.3g of %.3g"
          % (prec, flags, hop, err, scale))
    assert scale > 1e-2 and np.abs(want[0] - want[1]).max() > 1e-3 and np.abs(want[:, -1]).max() > 1e-4
    assert err <= 2e-4 * scale, (err, scale)
    if block.shape[2] > st.R:
        assert float((grad[:, :, st.R:] - 0.25).abs().max()) == 0.0          # the padding behind a row stays untouched
    return grad


@pytest.mark.parametrize("prec,flags,t1", PATHS)
def test_interpolated_rows_against_the_reference_on_every_path(prec, flags, t1):
    """wn_stack_fwd with bias_interp = 1 at hop 12, phase 5 against the float64 reference within ATOL: every layer's out, z,
    tanh, sigmoid and the skip sum, on every entry of test_gpu_local_condition.PATHS (fp16 x 2 runs
    k_layer_fwd_h2_t1<1, kCondLinear>)."""
    st, x, block = _case()
    assert block.shape[1] == 8
    got = _run(st, x, block, prec, flags, t1)
    _against_reference(st, x, block, LI.HOP, LI.PHASE, got)
    z2 = _split_z(st, got[1], B, T)[2]                       # the d = 4 layer: zero prefix, neither convolution nor bias
    assert float(z2[:, :2].abs().max()) == 0.0 and float(z2[:, 2].abs().max()) > 0.0
    rep = LR.stack_forward(st.p, st.w, x, block[:, :7], LI.HOP, LI.PHASE)[1]
    assert np.abs(to_np(got[4]) - btc(rep)).max() > 100 * ATOL          # ... and it is not the staircase


@pytest.mark.parametrize("prec,flags,t1", PATHS)
def test_interpolated_rows_with_window_only_and_a_ragged_window_offset(prec, flags, t1):
    """The training form of the call, window_only and t_off = 37, on every path."""
    st, x, block = _case(seed=2)
    got = _run(st, x, block, prec, flags, t1, t_off=37, window_only=1)
    assert got[4].shape == (B, T - 37, st.Cs)
    _against_reference(st, x, block, LI.HOP, LI.PHASE, got, t_off=37)


@pytest.mark.parametrize("Cr,cd", WIDE)
def test_interpolated_rows_on_the_wide_path(Cr, cd):
    """Widths the fused kernels do not cover: k_wide_gate<true> adds the interpolated row.  Forward against the reference;
    the gradient rows against the reference gradient, identical from run to run."""
    assert _lib.lib().wn_layer_fast_path(Cr, cd, 2) == 0
    st, x, block = _case(_wide(Cr, cd), seed=6)
    got = _run(st, x, block, "bf16x3", 0, 0)
    _against_reference(st, x, block, LI.HOP, LI.PHASE, got)
    _grad_rows_against_reference(st, x, block, "bf16x3", 0)


@pytest.mark.parametrize("flags", [0, GENERIC])
def test_interpolated_gradient_rows_on_the_fused_and_generic_paths(flags):
    """wn_stack_bwd's dbf / dbg blocks (k_colsum_per_frame_lerp) at the base case with 4 floats of padding behind a row."""
    st, x, block = _case(seed=7, pad=4)
    _grad_rows_against_reference(st, x, block, "fp32", flags)


def test_segments_longer_than_eight_chunks():
    """hop = 600, T = 1,300, B = 2, one 16 / 24-channel layer (test_a_segment_longer_than_one_chunk's shape): a segment of 600
    rows is 19 chunks of 32 (the last ragged), so every reduction lane of a half adds two or three chunks; the last frame
    holds 100 rows.  Gradient rows against the reference, identical from run to run, the padding behind a row untouched."""
    over = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[24], residual_num_blocks=1,
                softmax_conv_channels=[64, 256])
    st, x, block = _case(over, seed=9, hop=600, phase=0, pad=2, Bn=2, Tn=1300)
    assert block.shape[1] == 4 and st.frames[2] == 50
    _grad_rows_against_reference(st, x, block, "fp32", 0, hop=600, phase=0)


def test_interpolated_gradient_rows_in_the_documented_order():
    """test_segments_longer_than_eight_chunks's shape (B = 2, T = 1,300, hop 600, one 16 / 24-channel layer, generic path): a
    reduction lane adds more than one chunk and the last frame is ragged.  Layer 0's rows -- the (da | dg) scratch the
    workspace still holds when the call returns -- are bit-equal to the float32 sums formed on the host in the documented
    order of k_colsum_per_frame_lerp (LI.colsum_lerp_in_kernel_order: halves of 8 lanes, chunks of 32 rows, weights 1 - alpha /
    alpha, one fused multiply-add per row, the 16 partials in index order), added to the value the rows started from."""
    over = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[24], residual_num_blocks=1,
                softmax_conv_channels=[64, 256])
    Bn, Tn, hop = 2, 1300, 600
    st, x, block = _case(over, seed=9, hop=hop, phase=0, pad=2, Bn=Bn, Tn=Tn)
    assert block.shape[1] == 4 and st.frames[2] == 50
    grad, ws, _, _, _, _ = _grad_rows(st, x, block, "fp32", 0)
    zoff = Bn * Tn * st.ncd
    dab = to_np(ws[zoff:zoff + Bn * Tn * 48]).reshape(Bn, Tn, 48)
    got = to_np(grad)
    for b in range(Bn):
        for f in range(4):
            tot, suspect = LI.colsum_lerp_in_kernel_order(dab[b], f, hop, 0)
            assert suspect == 0, (b, f)                    # (the host emulation vouches for every fused multiply-add)
            want = np.float32(0.25) + tot
            assert np.abs(want - 0.25).max() > 1e-3       # (every row receives something: the last one the ragged frame's alpha part)
            assert np.array_equal(got[b, f, :48], want), (b, f, np.abs(got[b, f, :48] - want).max())
    assert float((grad[:, :, 48:] - 0.25).abs().max()) == 0.0


@pytest.mark.parametrize("prec,t1", [("fp32", 1), ("fp16x2", 1)])
def test_a_hop_longer_than_the_clip(prec, t1):
    """hop 100, phase 40: hop > T, two frames (the border at t = 60) and three rows; the first segment lies partly below the
    d = 4 layers' zero prefix.  Forward and gradient rows against the reference."""
    st, x, block = _case(seed=11, hop=100, phase=40)
    assert block.shape[1] == 3
    got = _run(st, x, block, prec, 0, t1)
    _against_reference(st, x, block, 100, 40, got)
    _grad_rows_against_reference(st, x, block, prec, 0, hop=100, phase=40)


@pytest.mark.parametrize("prec,t1", [("fp32", 1), ("fp16x2", 1)])
def test_hop_one_is_repeat_mode_on_the_first_T_rows(prec, t1):
    """hop 1, phase 0: alpha is 0 at every position, so r[j] + 0 (r[j + 1] - r[j]) is r[j]: every output and every gradient
    row equals (==) the repeat-mode call on the first T rows.  Row T is read (weight 0) and its gradient is 0: the value it
    started from is still there.  Rows below a layer's zero prefix are untouched in both modes."""
    st, x, block = _case(seed=12, hop=1, phase=0)
    assert block.shape[1] == T + 1
    lin = _run(st, x, block, prec, 0, t1)
    g_lin = _grad_rows(st, x, block, prec, 0)[0]
    st.interp = 0
    rep_block = np.ascontiguousarray(block[:, :T])
    rep = _run(st, x, rep_block, prec, 0, t1)
    g_rep = _grad_rows(st, x, rep_block, prec, 0)[0]
    for k in range(5):
        assert torch.equal(lin[k], rep[k]), k
    assert torch.equal(g_lin[:, :T], g_rep) and float((g_rep - 0.25).abs().max()) > 1e-2
    assert float((g_lin[:, T] - 0.25).abs().max()) == 0.0


# ---- bitwise anchor --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,flags,t1", PATHS)
def test_rows_equal_within_a_clip_give_the_per_clip_call_bit_for_bit(prec, flags, t1):
    """A block whose 8 rows are equal within a clip and differ between clips (random, nonzero): a + alpha (b - a) with b == a
    is a, so the linear-mode call gives the bits of the per-clip call with that row -- every forward output, dx and (off the
    generic path, whose any-shape weight-gradient kernels leave through float atomics with or without bias rows) every weight
    gradient.  The gradient rows of a clip, summed over its rows in float64, are the per-clip gradient row up to fp32
    summation order: sum_f [(1 - alpha_t) + alpha_t] d_t against sum_t d_t -- within 2e-4 of the per-clip block's largest
    entry, the bound the gradient-row comparisons of test_gpu_local_condition.py use."""
    st, x, block = _case(seed=4)
    rs = np.random.RandomState(40)
    row = (rs.standard_normal((B, 1, st.R)) * 0.5).astype(np.float32)
    assert np.abs(row).min() > 0 and np.abs(row[0] - row[1]).max() > 0.1
    block = np.ascontiguousarray(np.repeat(row, block.shape[1], axis=1))
    t_off = 21
    dout = dev(rs.standard_normal((B, T, st.Cr)).astype(np.float32))
    dskip = dev(rs.standard_normal((B, T - t_off, st.Cs)).astype(np.float32))
    xd = dev(btc(x))
    res = []
    for frames, bias in ((st.frames, block), (None, block[:, :1])):
        st.frames = frames
        bd = dev(np.ascontiguousarray(bias))
        n = bias.shape[1]
        ex = lambda: _ex(prec, flags | PER_CLIP, n * st.R, t1)
        rc, acts = st.fwd(xd, bd, ex(), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        grad = torch.zeros((B, n, st.R), device="cuda")
        rc, dx, gW = st.bwd(xd, acts, dout, dskip, grad, ex(), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        res.append((acts, dx, gW, grad))
    (a0, dx0, g0, r0), (a1, dx1, g1, r1) = res
    for k in range(5):
        assert torch.equal(a0[k], a1[k]), k
    assert torch.equal(dx0, dx1)
    if not flags & GENERIC:
        for k in g0:
            for l in range(st.L):
                assert torch.equal(g0[k][l], g1[k][l]), (k, l)
    summed, clip = to_np(r0).astype(np.float64).sum(1), to_np(r1)[:, 0].astype(np.float64)
    scale = np.abs(clip).max()
    assert scale > 1e-2 and np.abs(summed - clip).max() <= 2e-4 * scale, (np.abs(summed - clip).max(), scale)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_bad_interpolation_fields_are_refused_before_any_device_work():
    st, x, block = _case(seed=10)
    n, rw = block.shape[1], block.shape[2]
    xd, bd = dev(btc(x)), dev(block)
    lib = _lib.lib()

    def refused(frames, interp, stride, word, bias=bd):
        st.frames, st.interp = frames, interp
        rc, out = st.fwd(xd, bias, _ex("fp32", PER_CLIP, stride, 1))
        msg = lib.wn_last_error()
        assert rc == _lib.WN_EARG and word in msg, (frames, interp, msg)
        assert all(float(o.abs().max()) == 0.0 for o in out)
        grad = torch.full_like(bias, 0.5)
        acts = tuple(torch.ones_like(o) for o in out)
        rc, dx, gW = st.bwd(xd, acts, torch.ones_like(xd), None, grad, _ex("fp32", PER_CLIP, stride, 1))
        assert rc == _lib.WN_EARG and word in lib.wn_last_error(), (frames, interp)
        assert float(dx.abs().max()) == 0.0 and float((grad - 0.5).abs().max()) == 0.0

    refused((12, 5, rw), 2, n * rw, b"bias_interp")
    refused((12, 5, rw), -1, n * rw, b"bias_interp")
    refused((0, 0, 0), 1, n * rw, b"without frames")
    refused((12, 5, rw), 1, (n - 1) * rw, b"frames + 1")             # 7 rows: what repeat mode needs, one short here
    st.frames, st.interp = (12, 5, rw), 0
    rc, _ = st.fwd(xd, bd, _ex("fp32", PER_CLIP, (n - 1) * rw, 1))
    assert rc == 0


# ---- the locally conditioned model ------------------------------------------------------------------------------------------
def _model(cls=WaveNet, seed=1234, glob=False, local_seed=77, hop=LI.HOP):
    p = R.make_params(**LI.TINY)
    w = R.init_weights(p, seed)
    V, h = LI.init_local(p, seed=local_seed)
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    net = cls(Params(p), seed=0, local_channels=LI.FEATS, local_hop=hop, local_interp="linear", **kw)
    net.load_state_dict(LI.state_dict(w, V, E, Vg))
    net.to_gpu()
    return p, w, V, h, E, Vg, net


_BATCH = {}


def _batch(glob=False):
    """The tiny batch and its CPU reference, computed once and shared (read-only)."""
    if glob not in _BATCH:
        p = R.make_params(**LI.TINY)
        w = R.init_weights(p, 1234)
        V, h = LI.init_local(p)
        E, Vg = cond_ref.init_condition(p) if glob else (None, None)
        rs = np.random.RandomState(8)
        tw = 40
        idx = rs.randint(0, 256, (B, T)).astype(np.int32)
        tgt = rs.randint(0, 256, (B, tw)).astype(np.int32)
        ref = LI.train_step_grads(p, w, V, h, LI.HOP, LI.PHASE, idx, tgt, E=E, Vg=Vg, ids=cond_ref.IDS if glob else None)
        _BATCH[glob] = dict(idx=idx, tgt=tgt, tw=tw, ref=ref, h=h)
    return _BATCH[glob]


@pytest.mark.parametrize("prec,t1,glob", [("fp32", None, False), ("bf16x3", None, False), ("fp16x2", 1, False),
                                          ("fp16x2", None, False), ("bf16", None, False), ("fp32", None, True),
                                          ("fp16x2", 1, True)])
def test_interpolating_model_loss_logits_and_every_gradient_against_the_reference(prec, t1, glob):
    """Loss, logits and the gradient of every weight -- V included -- and of the features against tests/local_interp_ref.py
    in every GEMM precision, at the tolerances of the conditioned whole-model tests: 1e-4 on loss and logits, 2e-4 of a
    tensor's largest entry on gradients; bf16: 2e-2 on the loss and 15 % in the 2-norm.  fp16x2 runs with the COND kernels
    forced (fwd_t1_min_blocks = 1) and as the library dispatches this size.  Twice more with global conditioning also on."""
    p, w, V, h, E, Vg, net = _model(glob=glob)
    assert net.local_interp == "linear" and (net.local_channels, net.local_hop) == (LI.FEATS, LI.HOP)
    net.gemm_precision = prec
    net.fwd_t1_min_blocks = t1
    bt = _batch(glob)
    loss_ref, logits_ref, g = bt["ref"]
    tw = bt["tw"]
    feats = dev(h).requires_grad_(True)
    kw = dict(local=feats, local_phase=LI.PHASE)
    if glob:
        kw["condition"] = cond_ref.IDS
    c = net.forward_causal_block(bt["idx"])
    _, s = net.forward_residual_block(c, t_off=T - tw, **kw)
    lg = net.forward_softmax_block(s, apply_softmax=False)
    loss = net.cross_entropy(lg, bt["tgt"])
    net.zero_grads()
    loss.backward()
    torch.cuda.synchronize()
    loose = prec == "bf16"
    assert abs(float(loss.detach()) - loss_ref) < (2e-2 * max(1.0, abs(loss_ref)) if loose else 1e-4)
    if not loose:
        np.testing.assert_allclose(to_np(lg), logits_ref, atol=ATOL)
    names = {"global_condition_embed": "E", "global_condition_projection": "Vg", "local_condition_projection": "V"}

    def close(got, want, what):
        if loose:
            rel = np.linalg.norm((got - want).astype(np.float64)) / (np.linalg.norm(want.astype(np.float64)) + 1e-30)
            assert rel < 0.15, (what, rel)
        else:
            scale = max(np.abs(want).max(), 1e-6)
            assert np.abs(got - want).max() <= 2e-4 * scale + 1e-7, (what, np.abs(got - want).max(), scale)
    seen = set()
    for ln, kind, off, n, shape in net._spans:
        name = names.get(ln.name, "%s/%s" % (ln.name, kind))
        seen.add(name)
        close(to_np(net._grad_arena[off:off + n].view(shape)), g[name].reshape(shape), name)
    assert "V" in seen and np.abs(g["V"]).max() > 1e-4 and np.abs(g["h"][:, :, -1]).max() > 1e-6
    close(to_np(feats.grad), g["h"], "h")
    # seven columns are one short, and say so
    with pytest.raises(Exception, match="linear interpolation"):
        net.forward_residual_block(c, t_off=T - tw, **dict(kw, local=dev(h[:, :, :7])))


def test_train_step_graph_replays_an_interpolating_step():
    """Three replayed steps land on the weights of three op-by-op steps (2e-5, Adam's eps raised, as the repeat-mode graph
    test demands), the features changing between replays; two captures give identical bits."""
    eager = _model()[-1]
    nets = [_model()[-1] for _ in range(2)]
    for n in [eager] + nets:
        n.update_laerning_rate(0.01)
        n.optimizer.eps = 1e-3
    iw = eager.input_width
    rs = np.random.RandomState(0)
    nf = LI.frames_needed(T, LI.HOP, LI.PHASE)
    batches = [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, T - iw)).astype(np.int32)),
                dev(rs.standard_normal((B, LI.FEATS, nf)).astype(np.float32))) for _ in range(3)]
    w0 = to_np(nets[0]._arena).copy()
    graphs = [TrainStepGraph(n, batches[0][0], batches[0][1], local=batches[0][2], local_phase=LI.PHASE) for n in nets]
    np.testing.assert_array_equal(to_np(nets[0]._arena), w0)
    for x, tg, ft in batches:
        eager.backprop(default_loss(eager, x, tg, local=ft, local_phase=LI.PHASE))
        losses = [float(g.step(x, tg, local=ft)) for g in graphs]
        assert np.isfinite(losses[0]) and losses[0] == losses[1]
    a, b = to_np(eager._arena), to_np(nets[0]._arena)
    assert np.abs(a - w0).max() > 1e-3
    np.testing.assert_allclose(b, a, atol=2e-5)
    assert torch.equal(nets[0]._arena, nets[1]._arena)
    with pytest.raises(Exception, match="feature columns"):
        TrainStepGraph(eager, batches[0][0], batches[0][1], local=batches[0][2][:, :, :nf - 1], local_phase=LI.PHASE)


def test_the_weight_average_swap_keeps_the_mode(tmp_path):
    """The EMA swap and a checkpoint round trip in linear mode: the averaged weights give the same loss before and after."""
    _, _, _, h, _, _, net = _model()
    net.enable_ema(0.5, warmup=False)
    net.update_laerning_rate(0.01)
    bt = _batch()
    x, tgt = dev(bt["idx"]), dev(bt["tgt"])
    kw = dict(local=dev(h), local_phase=LI.PHASE)
    for _ in range(2):
        net.backprop(default_loss(net, x, tgt, **kw))
    with net.ema_weights():
        assert net.local_interp == "linear"
        loss_avg = float(default_loss(net, x, tgt, **kw).detach())
    net.save(str(tmp_path))
    avg = _model(seed=5, local_seed=6)[-1]
    avg.load(str(tmp_path), weights="ema")
    assert abs(float(default_loss(avg, x, tgt, **kw).detach()) - loss_avg) <= 1e-6 * max(1.0, abs(loss_avg))


# ---- the decoder -----------------------------------------------------------------------------------------------------------
DHOP = 5


class _Dec(object):
    """Decoder handles of an interpolating FasterWaveNet and of its biased twin, all seeded from ONE prefill state."""

    def __init__(self):
        self.p, self.w, self.V, _, _, _, self.net = _model(cls=FasterWaveNet, hop=DHOP)
        rs = np.random.RandomState(21)
        self.h = rs.standard_normal((LI.FEATS, 6)).astype(np.float32)
        self.rows = self.net.local_biases(self.h)                               # (6, R): one row per given column
        self.R = int(self.rows.shape[1])
        self.Q = 256
        self.tok = dev(rs.randint(0, 256, (1, self.net.input_width)).astype(np.int32))
        self.handles = []

    def twin(self, row):
        net = self.net
        net.condition_biases = lambda c: [(row[of:of + lay.cd].clone(), row[og:og + lay.cd].clone())
                                          for lay, (of, og) in zip(net._flat_layers, net._cond_offsets)]
        try:
            return _biased_twin(self.p, self.w, net, 0)
        finally:
            del net.condition_biases

    def handle(self, model, state_from, table=None, interp=None):
        d, keep = model._desc(None, table)
        if interp is not None:
            d.frame_interp = interp
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        check(_lib.lib().wn_decoder_load_state(h, ptr(self.tok), int(self.tok.shape[1]),
                                               ptr_array([t.contiguous() for t in state_from._last_causal_outputs]),
                                               ptr_array(state_from._last_layer_inputs), None), "wn_decoder_load_state")
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


def test_decoder_interpolated_table_through_the_c_abi():
    """(a) A table of zeros decodes bit for bit as the biased model with zero biases, and a table whose rows all equal r as
    the biased model with static biases r (tokens and probability trace).  (b) Rows r0, r1, r1, r0 at hop 5 from phase 2: step 0
    already differs from the static-r0 model (alpha = 2/5), and the repeat-mode handle on the same table decodes something
    else.  (c) 12 steps in one launch equal 5 + 7 in two, bit for bit.  (d) A run one
    row short is refused before any device work and leaves the handle's state alone: 4 rows cover 13 steps in linear mode
    where repeat mode covers 18.  (e) A batch that mixes modes is refused; a mode outside {0, 1} is refused at create."""
    D = _Dec()
    try:
        lib = _lib.lib()
        u = dev(np.random.RandomState(5).random_sample(20))
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
        twz = D.twin(torch.zeros_like(r0))
        rc, t_z, p_z = D.run(D.handle(twz, tw0), 12, u)
        rc2, t_0, p_0 = D.run(D.handle(D.net, tw0, (torch.zeros((4, D.R), device="cuda"), DHOP, 2)), 12, u)
        assert rc == 0 and rc2 == 0 and torch.equal(t_z, t_0) and torch.equal(p_z, p_0)
        # (b) + (c)
        tab = torch.stack([r0, r1, r1, r0]).contiguous()
        hb = D.handle(D.net, tw0, (tab, DHOP, 2))
        rc, t_b, p_b = D.run(hb, 12, u)
        assert rc == 0, lib.wn_last_error()
        assert not torch.equal(p_b[0], p_ref[0])
        hc = D.handle(D.net, tw0, (tab, DHOP, 2))
        rc, t_c1, p_c1 = D.run(hc, 5, u)
        rc2, t_c2, p_c2 = D.run(hc, 7, u[5:], first=int(t_c1[4]))
        assert rc == 0 and rc2 == 0
        assert torch.equal(torch.cat([t_c1, t_c2]), t_b) and torch.equal(torch.cat([p_c1, p_c2]), p_b)
        rep = D.handle(D.net, tw0, (tab, DHOP, 2), interp=0)
        rc, t_r, p_r = D.run(rep, 12, u)
        assert rc == 0 and not torch.equal(p_r, p_b)                             # the staircase is another function
        # (d) phase 2 + 13 steps: the last step sits at p = 14, j = 2, and reads row 3 -- the last one.  One more is refused.
        rc, t_f, p_f = D.run(hb, 2, u)
        assert rc == _lib.WN_EARG and b"frame table of 4 rows" in lib.wn_last_error() and b"linear" in lib.wn_last_error()
        assert int(t_f.min()) == -1 and float(p_f.abs().max()) == 0.0            # nothing ran
        fresh = D.handle(D.net, tw0, (tab, DHOP, 2))
        rc, t_13, p_13 = D.run(fresh, 13, u)
        assert rc == 0
        rc, t_last, p_last = D.run(hb, 1, u[12:], first=int(t_b[11]))
        assert rc == 0 and torch.equal(p_last[0], p_13[12]) and torch.equal(t_13[:12], t_b)
        rc, _, _ = D.run(rep, 6, u)                                              # repeat mode covers 18 steps with the 4 rows
        assert rc == 0
        # (e)
        h1, h2 = D.handle(D.net, tw0, (tab, DHOP, 2)), D.handle(D.net, tw0, (tab, DHOP, 2), interp=0)
        outs = [torch.full((3,), -1, device="cuda", dtype=torch.int32) for _ in range(2)]
        us = [u[:3].contiguous(), u[3:6].contiguous()]
        for same_w in (0, 1):
            rc = lib.wn_decoder_run_batch((C.c_void_p * 2)(h1.value, h2.value), 2, (C.c_int32 * 2)(7, 7), ptr_array(us), 3,
                                          ptr_array(outs), None, same_w, None)
            assert rc == _lib.WN_EARG and b"frame_interp" in lib.wn_last_error()
        torch.cuda.synchronize()
        assert int(outs[0].min()) == -1 and int(outs[1].min()) == -1
        d, keep = D.net._desc(None, (tab, DHOP, 2))
        d.frame_interp = 2
        hx = C.c_void_p()
        assert lib.wn_decoder_create(C.byref(hx), C.byref(d), None) == _lib.WN_EARG and b"frame_interp" in lib.wn_last_error()
        assert lib.wn_decoder_update_weights(fresh, C.byref(d), None) == _lib.WN_EARG
    finally:
        D.close()


def test_decoded_trace_agrees_with_the_teacher_forced_forward_in_linear_mode():
    """hop 5, phase 3, 40 decoded steps behind the prefill: row i of generate()'s probability trace agrees within ATOL with
    the model's own forward (ELU head) over the window and the emitted tokens with the same features.  The features hold the
    one column more that linear mode reads; without it generate() raises before anything runs."""
    p, w, V, _, _, _, net = _model(cls=FasterWaveNet, hop=DHOP)
    n = 41
    W = net.input_width
    assert W == 16
    rs = np.random.RandomState(31)
    cols = LI.frames_needed(W + n - 1, DHOP, 3)
    h = rs.standard_normal((LI.FEATS, cols)).astype(np.float32)
    u = rs.random_sample(n)
    prompt = rs.randint(0, 256, (W,)).astype(np.int32)
    toks, probs = net.generate(n, u, initial_tokens=prompt, return_probs=True, local=h, local_phase=3)
    full = np.concatenate([prompt, to_np(toks)[:-1]])[None]
    with torch.no_grad():
        c = net.forward_causal_block(dev(full))
        _, s = WaveNet.forward_residual_block(net, c, local=dev(h[None]), local_phase=3)
        ref = net.forward_softmax_block(s, apply_softmax=True, activation="elu")
    ref = to_np(ref)[0, :, 0, :].T
    np.testing.assert_allclose(to_np(probs)[1:], ref[W:], atol=ATOL)
    assert tuple(net.local_biases(h).shape) == (cols, 384)                    # one row per given column, as in repeat mode
    with pytest.raises(Exception, match="cover fewer samples"):
        net.generate(n, u, initial_tokens=prompt, local=h[:, :cols - 1], local_phase=3)


def test_generate_batch_equals_the_single_runs_in_linear_mode():
    """Three utterances with different features and phases: row u of generate_batch is generate() with utterance u's features
    and phase, bit for bit."""
    p, w, V, _, _, _, net = _model(cls=FasterWaveNet, hop=DHOP)
    n = 24
    W = net.input_width
    rs = np.random.RandomState(41)
    u = rs.random_sample((3, n))
    phases = [0, 3, 4]
    hs = [rs.standard_normal((LI.FEATS, LI.frames_needed(W + n - 1, DHOP, ph) + k)).astype(np.float32) for k, ph in enumerate(phases)]
    singles = [net.generate(n, u[i], local=hs[i], local_phase=phases[i]) for i in range(3)]
    assert len({tuple(to_np(t)) for t in singles}) == 3
    rows = net.generate_batch(n, u, local=hs, local_phase=phases)
    for i in range(3):
        assert torch.equal(rows[i], singles[i]), i
    with pytest.raises(Exception, match="cover fewer samples"):
        net.generate_batch(n, u, local=[hs[0], hs[1], hs[2][:, :-3]], local_phase=phases)


# ---- scoring ---------------------------------------------------------------------------------------------------------------
def test_scoring_in_linear_mode_does_not_depend_on_the_cut():
    """The mean of token_nll is the training loss of the same window (1e-5 relative); score() in exact arithmetic does not
    change with batch_size or chunk_width (1e-5 of the largest value, test_locally_conditioned_scoring's bound) -- the pieces
    overlap by one column --, changes with the features, and needs ceil(n / H) + 1 columns."""
    _, _, _, h, _, _, net = _model()
    bt = _batch()
    x, tgt, ft = dev(bt["idx"]), dev(bt["tgt"]), dev(h)
    want = float(default_loss(net, x, tgt, local=ft, local_phase=LI.PHASE).detach())
    rows = net.token_nll(x, tgt, local=ft, local_phase=LI.PHASE)
    mean = float(to_np(rows).astype(np.float64).mean())
    assert abs(mean - want) <= 1e-5 * abs(want), (mean, want)
    rs = np.random.RandomState(51)
    toks = rs.randint(0, 256, (200,)).astype(np.int32)
    cols = LI.frames_needed(200, LI.HOP)
    f = rs.standard_normal((LI.FEATS, cols)).astype(np.float32)
    net.gemm_precision = "fp32"
    a = net.score(toks, chunk_width=48, batch_size=2, local=f)
    b = net.score(toks, chunk_width=96, batch_size=8, local=f)
    c = net.score(toks, chunk_width=48, batch_size=1, local=f)
    assert a.shape == (200,)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) and float((a - c).abs().max()) <= 1e-5 * float(a.abs().max())
    other = net.score(toks, chunk_width=48, batch_size=2, local=-f)
    assert float((a - other).abs().max()) > 1e-3
    with pytest.raises(Exception, match="feature columns"):
        net.score(toks, chunk_width=48, local=f[:, :cols - 1])


# ---- the command line: train --local-interp linear -> generate -> evaluate -----------------------------------------------------
def test_cli_train_generate_evaluate_in_linear_mode(tmp_path):
    """A few updates with --local-interp linear write ``"interp": "linear"`` into local.json; generate and evaluate take the
    mode from the checkpoint and supply the column behind the file's last one themselves: n columns still give n * hop
    samples, and a file of ceil(samples / hop) columns still scores.  A resumed run with the other mode stops."""
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
    t = np.arange(sr // 4) / sr
    wavfile.write(str(wav / "a.wav"), sr, (0.5 * np.sin(2 * np.pi * 220 * t) * 32767).astype(np.int16))
    cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "64", "--mels", "12", "--win", "256"])
    fa = np.load(str(feat / "a.npy"))
    cfg = {"quantization_steps": 256, "sampling_rate": sr, "causal_conv_channels": [32], "residual_conv_channels": [32] * 4,
           "residual_num_blocks": 2, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
    (model / "wavenet.json").write_text(json.dumps(cfg))
    common = ["-w", str(wav), "-m", str(model), "--seed", "1"]
    loop = ["--lr", "0.003", "--batch-size", "4", "--train-width", "256", "--repeat", "4", "--max-epoch", "2"]
    l1 = cli_train.main(common + loop + ["--local-dir", str(feat), "--local-hop", "64", "--local-interp", "linear"])
    assert np.isfinite(l1)
    assert json.loads((model / "local.json").read_text()) == {"channels": 12, "hop": 64, "interp": "linear"}
    assert cli_local.load_config(str(model)) == (12, 64) and cli_local.load_interp(str(model)) == "linear"
    l2 = cli_train.main(common + loop + ["--local-dir", str(feat), "--no-graph"])      # resumed: the mode comes from local.json
    assert np.isfinite(l2)
    with pytest.raises(SystemExit, match="same mode"):
        cli_train.main(common + loop + ["--local-dir", str(feat), "--local-interp", "repeat"])
    out = str(tmp_path / "gen")
    short = str(tmp_path / "short.npy")
    np.save(short, fa[:, :4])
    fn, one = cli_generate.main(["-m", str(model), "-o", out, "--fast", "--seed", "2", "--local", short])
    assert one.shape == (4 * 64 - 32 + 1,) and one.min() >= 0 and one.max() < 256     # n columns: n * hop samples, as in repeat mode
    fn2, slow = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.003", "--seed", "2", "--local", short])
    assert slow.shape == (int(sr * 0.003) - 1,) and slow[0] == one[0]
    table = cli_evaluate.main(["-w", str(wav), "-m", str(model), "--local-dir", str(feat)])
    assert np.isfinite(table["files"][0]["nats_per_sample"]) and table["files"][0]["samples"] > 0
