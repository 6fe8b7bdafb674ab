"""Global conditioning on the GPU: per-clip bias rows through the C ABI (WN_EXEC_BIAS_PER_CLIP) against the shared-bias form
clip by clip and against the float64 reference of tests/cond_ref.py, then the conditioned model -- loss and every gradient,
the replayed training step, generation, scoring, checkpoints and the weight average.

The tiny case (cond_ref.TINY, B = 3, T = 70, ids [2, 0, 2]): three 32-column tiles per clip, the last one partial, so one
four-wave workgroup holds tiles of two clips -- the case a wrong clip index gets wrong -- with a repeated id, an unused class
and the compatibility zero prefix on."""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_ref
from gpu_util import EX, btc, dev, to_np
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, WaveNet, _lib
from wavenet_amd._lib import check, int_array, ptr
from wavenet_amd.graph import default_loss

pytestmark = pytest.mark.gpu

PER_CLIP = _lib.WN_EXEC_BIAS_PER_CLIP
GENERIC = _lib.WN_EXEC_FORCE_GENERIC
ATOL = 1e-4                      # tests/test_gpu_parity.py: fp32 activations and logits within 1e-4 absolute
U32 = 2.0 ** -24                 # unit round-off of float32


# ---- the residual stack through the C ABI ---------------------------------------------------------------------------------
class _Stack(object):
    """Device weights of a model's residual stack and descriptors over them; bias tables are given per call."""

    def __init__(self, over, seed=1234):
        self.p = R.make_params(**over)
        self.w = R.init_weights(self.p, seed)
        p = self.p
        self.cds = list(p["residual_conv_channels"]) * p["residual_num_blocks"]
        self.dil = [p["residual_conv_filter_width"] ** li for _ in range(p["residual_num_blocks"])
                    for li in range(len(p["residual_conv_channels"]))]
        self.L = len(self.cds)
        self.Cr, self.Cs, self.fw = p["causal_conv_channels"][-1], p["softmax_conv_channels"][0], p["residual_conv_filter_width"]
        pres = ["residual_%d_block_%d_" % (b, li) for b in range(p["residual_num_blocks"])
                for li in range(len(p["residual_conv_channels"]))]
        self.W = {k: [dev(self.w[pre + name + "/W"]) for pre in pres]
                  for k, name in (("Wf", "wf"), ("Wg", "wg"), ("Wp", "projection_block"), ("Ws", "projection_softmax"))}
        self.rows, self.R = cond_ref.cond_rows(p)
        self.ncd = sum(self.cds)

    def _tab(self, ptrs):
        arr = (C.c_void_p * self.L)(*ptrs)
        return arr, C.cast(arr, C.POINTER(C.c_void_p))

    def desc(self, bias=None):
        """bias: a device tensor whose FIRST row's layer slices the bf / bg tables point at (None: no biases)."""
        d = _lib.WnStackDesc()
        keep = [int_array(self.cds), int_array(self.dil)]
        d.n_layers, d.Cr, d.Cs, d.fw = self.L, self.Cr, self.Cs, self.fw
        d.cd, d.dilation = keep[0], keep[1]
        for k in ("Wf", "Wg", "Wp", "Ws"):
            arr, cast = self._tab([t.data_ptr() for t in self.W[k]])
            keep.append(arr)
            setattr(d, k, cast)
        if bias is not None:
            p0 = bias.data_ptr()
            for k, col in (("bf", 0), ("bg", 1)):
                arr, cast = self._tab([p0 + 4 * r[col] for r in self.rows])
                keep.append(arr)
                setattr(d, k, cast)
        return d, keep

    def fwd(self, x, bias, ex, t_off=0, window_only=0, desc_bias=True):
        """x (B, T, Cr) device; bias (B, R) device block or None.  Returns xs, z, f, g, skip."""
        B, T, _ = x.shape
        d, keep = self.desc(bias if desc_bias else None)
        xs = torch.zeros((self.L, B, T, self.Cr), device="cuda")
        z = torch.zeros((B * T * self.ncd,), device="cuda")
        f, g = torch.zeros_like(z), torch.zeros_like(z)
        skip = torch.zeros((B, T - t_off, self.Cs), device="cuda")
        rc = _lib.lib().wn_stack_fwd(C.byref(d), ptr(x), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(skip), B, T, t_off, 1,
                                     window_only, ex, None)
        torch.cuda.synchronize()
        return rc, (xs, z, f, g, skip)

    def bwd(self, x, acts, dout, dskip, dblock, ex, t_off=0):
        """Weight gradients go to fresh zero tensors (returned), bias gradients to dblock's rows (accumulated)."""
        B, T, _ = x.shape
        xs, z, f, g, _ = acts
        bias = torch.zeros_like(dblock)                    # the backward reads no bias value: only the tables' presence
        d, keep = self.desc(bias)
        lib = _lib.lib()
        gW = {k: [torch.zeros_like(t) for t in self.W[k]] for k in self.W}
        tabs = {k: self._tab([t.data_ptr() for t in gW[k]]) for k in gW}
        p0 = dblock.data_ptr()
        dbf = self._tab([p0 + 4 * r[0] for r in self.rows])
        dbg = self._tab([p0 + 4 * r[1] for r in self.rows])
        nbytes = lib.wn_stack_bwd_workspace_bytes(C.byref(d), B, T)
        ws = torch.empty((nbytes // 4,), device="cuda")
        dx = torch.zeros_like(x)
        rc = lib.wn_stack_bwd(C.byref(d), ptr(x), ptr(xs), ptr(z), ptr(f), ptr(g), ptr(dout), ptr(dskip), ptr(dx),
                              tabs["Wf"][1], dbf[1], tabs["Wg"][1], dbg[1], tabs["Wp"][1], None, tabs["Ws"][1], None,
                              ptr(ws), nbytes, B, T, t_off, 1, ex, None)
        torch.cuda.synchronize()
        return rc, dx, gW


def _ex(prec, flags, stride, t1=None):
    """WnExec of a direct call; ``stride`` travels in the field the flag gives a meaning to."""
    ref = EX(prec, flags=flags, t1_min_blocks=t1)
    ref._obj.reserved = int(stride)
    return ref


def _case(over=cond_ref.TINY, seed=0, bias_scale=0.5):
    st = _Stack(over)
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((cond_ref.B, st.Cr, 1, cond_ref.T)).astype(np.float32)
    bias = (rs.standard_normal((cond_ref.B, st.R)) * bias_scale).astype(np.float32)
    return st, x, bias


def _per_clip_and_clip_by_clip(st, x, bias, prec, flags, t1, t_off=0, window_only=0):
    """One B = 3 call with the flag, and three B = 1 calls of the shared-bias form with that clip's row."""
    xd, bd = dev(btc(x)), dev(bias)
    rc, got = st.fwd(xd, bd, _ex(prec, flags | PER_CLIP, st.R, t1), t_off, window_only)
    assert rc == 0, _lib.lib().wn_last_error()
    want = []
    for b in range(x.shape[0]):
        rc, one = st.fwd(xd[b:b + 1].contiguous(), bd[b:b + 1].contiguous(), _ex(prec, flags, 0, t1), t_off, window_only)
        assert rc == 0, _lib.lib().wn_last_error()
        want.append(one)
    return got, want


def _split_z(st, t, B, T):
    """Layer-major (sum_l B T cd_l) activations -> list of (B, T, cd_l)."""
    out, off = [], 0
    for cd in st.cds:
        out.append(t[off:off + B * T * cd].view(B, T, cd))
        off += B * T * cd
    return out


@pytest.mark.parametrize("prec,flags,t1", [("fp32", 0, 1), ("fp32", 0, -1), ("bf16x3", 0, 1), ("bf16x3", 0, -1),
                                           ("fp32", GENERIC, 0)])
def test_per_clip_bias_rows_are_the_shared_bias_form_clip_by_clip_bit_for_bit(prec, flags, t1):
    """wn_stack_fwd with WN_EXEC_BIAS_PER_CLIP and random bias rows against three B = 1 calls of the shared-bias form, each
    with that clip's row: layer outputs, z, tanh, sigmoid and the skip sum are IDENTICAL -- the same kernels (the exact-fp32
    fused ones in their one-tile-per-wave and looping forms, or the generic ones), the same columns, and a tile never spans
    clips.  A library that ignores the flag gives every clip the first clip's row and fails here."""
    st, x, bias = _case()
    B, T = cond_ref.B, cond_ref.T
    got, want = _per_clip_and_clip_by_clip(st, x, bias, prec, flags, t1)
    assert np.abs(to_np(got[1])).max() > 0.05
    assert not torch.equal(got[0][:, 1], got[0][:, 0])
    for b in range(B):
        assert torch.equal(got[0][:, b], want[b][0][:, 0]), ("layer outputs", b)
        for k, what in ((1, "z"), (2, "tanh"), (3, "sigmoid")):
            for l, (a, c) in enumerate(zip(_split_z(st, got[k], B, T), _split_z(st, want[b][k], 1, T))):
                assert torch.equal(a[b], c[0]), (what, b, l)
        assert torch.equal(got[4][b], want[b][4][0]), ("skip", b)
    # and it is the right answer: the float64 reference, at the bar of the parity tests
    layers, skip, _ = cond_ref.stack_forward(st.p, st.w, x, bias)
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL)
        np.testing.assert_allclose(to_np(_split_z(st, got[1], B, T)[l]), btc(layers[l][1]), atol=ATOL)
    np.testing.assert_allclose(to_np(got[4]), btc(skip), atol=ATOL)


def test_per_clip_bias_rows_with_window_only_and_a_ragged_window_offset():
    """The training form of the call: window_only and t_off = 37 (no multiple of 32).  A biased stack computes every column
    (its backward is the per-layer one), so the comparison is again bit for bit, skip window included."""
    st, x, bias = _case(seed=1)
    B, T, t_off = cond_ref.B, cond_ref.T, 37
    got, want = _per_clip_and_clip_by_clip(st, x, bias, "bf16x3", 0, 1, t_off=t_off, window_only=1)
    assert got[4].shape == (B, T - t_off, st.Cs)
    for b in range(B):
        assert torch.equal(got[0][:, b], want[b][0][:, 0]) and torch.equal(got[4][b], want[b][4][0]), b
    _, skip, _ = cond_ref.stack_forward(st.p, st.w, x, bias)
    np.testing.assert_allclose(to_np(got[4]), btc(skip)[:, t_off:], atol=ATOL)


def test_fp16x2_cond_kernels_against_the_reference_and_the_exact_fp32_kernels():
    """The default arithmetic: k_layer_fwd_h2_t1<SAVE = 1, COND> (fwd_t1_min_blocks = 1 selects it at this size), tanh saved.

    (a) Against the float64 reference at 1e-4 absolute, the bar tests/test_gpu_parity.py holds the unbiased fp16x2 layer
    outputs to.
    (b) Against the exact-fp32 kernels on the same rows.  The bias is added in fp32 BEHIND the rescale, so it must not cost
    the split products anything: the distance with random rows may exceed the distance the same two paths show with all rows
    ZERO (measured here, not assumed) by no more than the float32 rounding of the added term -- one rounding of a
    pre-activation per layer on either path, 2 x 2^-24 x the largest |pre-activation| (taken from the float64 reference) x
    the number of layers it can pass through.  A bias that went through the power-of-two tile scale or an fp16 split would
    add ~2^-11 of its size instead."""
    st, x, bias = _case(seed=2)
    B, T = cond_ref.B, cond_ref.T
    xd = dev(btc(x))
    dist = {}
    for name, rows in (("random", bias), ("zero", np.zeros_like(bias))):
        bd = dev(rows)
        rc, h2 = st.fwd(xd, bd, _ex("fp16x2", PER_CLIP, st.R, 1))
        assert rc == 0, _lib.lib().wn_last_error()
        rc, f32 = st.fwd(xd, bd, _ex("fp32", PER_CLIP, st.R, 1))
        assert rc == 0, _lib.lib().wn_last_error()
        dist[name] = max(float((a - c).abs().max()) for a, c in zip(h2, f32))
        if name == "random":
            layers, skip, amax = cond_ref.stack_forward(st.p, st.w, x, rows)
            for l in range(st.L):
                np.testing.assert_allclose(to_np(h2[0][l]), btc(layers[l][0]), atol=ATOL)
                for k in (1, 2, 3):
                    np.testing.assert_allclose(to_np(_split_z(st, h2[k], B, T)[l]), btc(layers[l][k]), atol=ATOL)
            np.testing.assert_allclose(to_np(h2[4]), btc(skip), atol=ATOL)
            # the zero prefix: neither the convolution nor the bias contributes
            Z = R.conv_pad_and_prefix(T, 4, 2)[1]
            assert Z > 0 and float(_split_z(st, h2[1], B, T)[2][:, :Z].abs().max()) == 0.0
    allowance = 2 * U32 * amax * st.L
    print("fp16x2 COND vs exact fp32: %.3g with random rows, %.3g with zero rows, allowance %.3g (max |pre-activation| %.3g)"
          % (dist["random"], dist["zero"], allowance, amax))
    assert dist["zero"] > 0.0                              # the two arithmetics do differ: the comparison measures something
    assert dist["random"] <= dist["zero"] + allowance, (dist, allowance)


def _bwd_case(over, prec, flags, seed=3):
    st, x, bias = _case(over, seed=seed)
    B, T, t_off = cond_ref.B, cond_ref.T, 21
    rs = np.random.RandomState(seed + 100)
    dout = dev(rs.standard_normal((B, T, st.Cr)).astype(np.float32))
    dskip = dev(rs.standard_normal((B, T - t_off, st.Cs)).astype(np.float32))
    xd, bd = dev(btc(x)), dev(bias)
    rc, acts = st.fwd(xd, bd, _ex(prec, flags | PER_CLIP, st.R, 1), t_off)
    assert rc == 0, _lib.lib().wn_last_error()
    block = torch.full((B, st.R), 0.25, device="cuda")     # gradients ACCUMULATE: the rows start from a value
    rc, dx, gW = st.bwd(xd, acts, dout, dskip, block, _ex(prec, flags | PER_CLIP, st.R, 1), t_off)
    assert rc == 0, _lib.lib().wn_last_error()
    rows, dxs = [], []
    for b in range(B):
        one = xd[b:b + 1].contiguous()
        rc, a1 = st.fwd(one, bd[b:b + 1].contiguous(), _ex(prec, flags, 0, 1), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        r1 = torch.full((1, st.R), 0.25, device="cuda")
        rc, dx1, _ = st.bwd(one, a1, dout[b:b + 1].contiguous(), dskip[b:b + 1].contiguous(), r1, _ex(prec, flags, 0, 1), t_off)
        assert rc == 0, _lib.lib().wn_last_error()
        rows.append(r1[0])
        dxs.append(dx1[0])
    return st, block, torch.stack(rows), dx, torch.stack(dxs)


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_per_clip_bias_gradient_rows_on_the_fused_path(prec):
    """wn_stack_bwd with the flag: row b of dbf / dbg is what a B = 1 call of the shared-bias form accumulates into its
    dbf / dbg for clip b -- the sums over t >= Z of that clip only.  Both sum the same (da, dg) scratch; the per-clip kernel
    follows the shared form's summation tree, so the difference is bounded by float32 summation order: at most
    2 (n - 1) u sum_t |x_t| <= 2 n^2 u max|x| for the n = 70 terms of a row (u = 2^-24), taken relative to the block's
    largest entry."""
    st, block, rows, dx, dxs = _bwd_case(cond_ref.TINY, prec, 0)
    got, want = to_np(block) - 0.25, to_np(rows) - 0.25
    assert np.abs(want).max() > 1e-2 and np.abs(want[0] - want[1]).max() > 1e-3          # rows differ from clip to clip
    n = cond_ref.T
    err = np.abs(got - want).max()
    print("per-clip bias gradient rows (%s): max |row - B=1 row| = %.3g of %.3g" % (prec, err, np.abs(want).max()))
    assert err <= 2 * n * n * U32 * np.abs(want).max(), err
    np.testing.assert_allclose(to_np(dx), to_np(dxs), atol=2 * n * U32 * float(dxs.abs().max()))


@pytest.mark.parametrize("over", [cond_ref.TINY,
                                  dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[24] * 3,
                                       residual_num_blocks=2, softmax_conv_channels=[64, 256])])
def test_per_clip_bias_gradient_rows_on_the_generic_path_are_bit_equal(over):
    """The same comparison under WN_EXEC_FORCE_GENERIC, and on a shape only the generic kernels take (Cr = 16, cd = 24;
    the row stride 288 is then no multiple of the width): bit for bit, forward included."""
    flags = GENERIC if over is cond_ref.TINY else 0
    if flags == 0:
        assert _lib.lib().wn_layer_fast_path(16, 24, 2) == 0
    st, block, rows, dx, dxs = _bwd_case(over, "fp32", flags, seed=4)
    assert float((rows - 0.25).abs().max()) > 1e-2
    assert torch.equal(block, rows)
    assert torch.equal(dx, dxs)


def test_per_clip_column_sums_over_many_chunks_keep_the_shared_forms_order():
    """k_colsum_per_clip where a clip is many chunks: T - Z = 67 x 256 + 37 rows that count make 68 chunks of 256 rows -- every
    reduction lane adds several, the last chunk is ragged -- through wn_layer_bwd on a
    generic shape (Cr = 16, cd = 24, stride 50: no multiple of the width or of 4).  Row b of dbf / dbg is bit for bit what a
    B = 1 call of the shared-bias form (per-chunk partials, then its fixed tree) adds for clip b."""
    B, Cr, Cd, fw, d, Z, stride = 2, 16, 24, 2, 4, 2, 50
    T = 67 * 256 + 37 + Z
    rs = np.random.RandomState(12)
    x = dev(rs.standard_normal((B, T, Cr)).astype(np.float32))
    f = dev(np.tanh(rs.standard_normal((B, T, Cd))).astype(np.float32))
    g = dev((1 / (1 + np.exp(-rs.standard_normal((B, T, Cd))))).astype(np.float32))
    Wf, Wg = (dev((rs.standard_normal((Cd, Cr, fw)) / 6).astype(np.float32)) for _ in range(2))
    Wp = dev((rs.standard_normal((Cr, Cd)) / 5).astype(np.float32))
    dout = dev(rs.standard_normal((B, T, Cr)).astype(np.float32))
    lib = _lib.lib()
    assert lib.wn_layer_fast_path(Cr, Cd, fw) == 0

    def run(sl, rows, flags, st):
        nb = sl.stop - sl.start
        ws = torch.empty((lib.wn_layer_bwd_workspace_floats(nb, T, Cr, Cd, fw),), device="cuda")
        dx = torch.empty((nb, T, Cr), device="cuda")
        gW = [torch.zeros_like(Wf), torch.zeros_like(Wg), torch.zeros_like(Wp)]
        check(lib.wn_layer_bwd(ptr(x[sl].contiguous()), ptr(f[sl].contiguous()), ptr(g[sl].contiguous()), ptr(Wf), ptr(Wg), ptr(Wp),
                               ptr(dout[sl].contiguous()), None, ptr(dx), ptr(gW[0]), rows.data_ptr(), ptr(gW[1]),
                               rows.data_ptr() + 4 * Cd, ptr(gW[2]), None, ptr(ws), nb, T, Cr, Cd, fw, d, Z,
                               _ex("fp32", flags, st), None), "wn_layer_bwd")
        torch.cuda.synchronize()

    block = torch.full((B, stride), 0.5, device="cuda")
    run(slice(0, B), block, PER_CLIP, stride)
    for b in range(B):
        row = torch.full((stride,), 0.5, device="cuda")
        run(slice(b, b + 1), row, 0, 0)
        assert float((row[:2 * Cd] - 0.5).abs().max()) > 1.0
        assert torch.equal(block[b], row), b                       # the two untouched floats behind the gates included


@pytest.mark.parametrize("Cr,cd", [(64, 32), (128, 128)])
def test_per_clip_bias_rows_on_the_wide_path(Cr, cd):
    """Widths the fused 32/32/2 kernels do not cover (wide_layer.hip; 128/128 takes its one-array (da | dg) backward): the
    gate GEMMs run without a bias and k_wide_gate adds the clip's row, so against the shared-bias form -- whose GEMM epilogue
    adds it -- the forward agrees to arithmetic, not to the bit: both are held to the float64 reference at the parity bar, and
    the per-clip gradient rows to the B = 1 rows within float32 summation order of n = 70 terms plus the two forwards'
    distance (1e-5 of the block's largest entry covers both by two orders of magnitude less than a wrong clip would show)."""
    over = dict(quantization_steps=256, causal_conv_channels=[Cr], residual_conv_channels=[cd] * 3, residual_num_blocks=1,
                softmax_conv_channels=[64, 256])
    assert _lib.lib().wn_layer_fast_path(Cr, cd, 2) == 0
    st, x, bias = _case(over, seed=6)
    B, T = cond_ref.B, cond_ref.T
    rc, got = st.fwd(dev(btc(x)), dev(bias), _ex("bf16x3", PER_CLIP, st.R, 0))
    assert rc == 0, _lib.lib().wn_last_error()
    layers, skip, _ = cond_ref.stack_forward(st.p, st.w, x, bias)
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL)
        for k in (1, 2, 3):
            np.testing.assert_allclose(to_np(_split_z(st, got[k], B, T)[l]), btc(layers[l][k]), atol=ATOL)
    np.testing.assert_allclose(to_np(got[4]), btc(skip), atol=ATOL)
    st, block, rows, dx, dxs = _bwd_case(over, "bf16x3", 0, seed=6)
    want = to_np(rows) - 0.25
    assert np.abs(want).max() > 1e-2 and np.abs(want[0] - want[1]).max() > 1e-3
    assert np.abs(to_np(block) - 0.25 - want).max() <= 1e-5 * np.abs(want).max()


def test_the_flag_is_refused_before_any_device_work():
    st, x, bias = _case()
    xd, bd = dev(btc(x)), dev(bias)
    lib = _lib.lib()
    rc, out = st.fwd(xd, bd, _ex("fp32", PER_CLIP, 31, 1))                      # stride below cd
    assert rc == _lib.WN_EARG and b"stride" in lib.wn_last_error() and float(out[0].abs().max()) == 0.0
    rc, out = st.fwd(xd, bd, _ex("fp32", PER_CLIP, st.R, 1), desc_bias=False)   # the flag without bias tables
    assert rc == _lib.WN_EARG and float(out[0].abs().max()) == 0.0
    # the fp16 x 2 kernels load a lane's biases as float4: a stride of 386 floats is refused, not sent down another path
    wide = torch.zeros((cond_ref.B, st.R + 2), device="cuda")
    rc, out = st.fwd(xd, wide, _ex("fp16x2", PER_CLIP, st.R + 2, 1))
    assert rc == _lib.WN_EARG and b"multiple of 4" in lib.wn_last_error() and float(out[0].abs().max()) == 0.0
    rc, out = st.fwd(xd, wide, _ex("fp32", PER_CLIP, st.R + 2, 1))              # the exact-fp32 kernels take any stride
    assert rc == 0
    # without the flag the field is ignored, as ever
    rc, a = st.fwd(xd[:1].contiguous(), bd[:1].contiguous(), _ex("fp32", 0, 12345, 1))
    rc2, b = st.fwd(xd[:1].contiguous(), bd[:1].contiguous(), _ex("fp32", 0, 0, 1))
    assert rc == 0 and rc2 == 0 and torch.equal(a[0], b[0])


# ---- the conditioned model -------------------------------------------------------------------------------------------------
def _model(cls=WaveNet, seed=1234, cond_seed=99):
    p = R.make_params(**cond_ref.TINY)
    w = R.init_weights(p, seed)
    E, V = cond_ref.init_condition(p, seed=cond_seed)
    net = cls(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    net.load_state_dict(cond_ref.state_dict(w, E, V))
    net.to_gpu()
    return p, w, E, V, net


_BATCH = {}


def _batch():
    """The tiny batch and its CPU reference, computed once and shared (read-only)."""
    if not _BATCH:
        p = R.make_params(**cond_ref.TINY)
        w = R.init_weights(p, 1234)
        E, V = cond_ref.init_condition(p)
        rs = np.random.RandomState(8)
        tw = 40
        idx = rs.randint(0, 256, (cond_ref.B, cond_ref.T)).astype(np.int32)
        tgt = rs.randint(0, 256, (cond_ref.B, tw)).astype(np.int32)
        _BATCH.update(idx=idx, tgt=tgt, tw=tw, ref=cond_ref.train_step_grads(p, w, E, V, cond_ref.IDS, idx, tgt))
    return _BATCH


@pytest.mark.parametrize("prec,t1", [("fp32", None), ("bf16x3", None), ("fp16x2", 1), ("fp16x2", None), ("bf16", None)])
def test_conditioned_loss_logits_and_every_gradient_against_the_reference(prec, t1):
    """Loss, logits and the gradient of every weight -- the embedding E and the projection V included -- against
    tests/cond_ref.py, in each GEMM precision at the tolerance the parity tests use for it (1e-4 on loss and logits, 2e-4 of a
    tensor's largest entry on gradients; bf16: 2e-2 and 15 % in the 2-norm).  fp16x2 runs twice: with the COND kernels
    (fwd_t1_min_blocks = 1) and as the library dispatches this size by itself.  The unused class's embedding gradient is
    exactly 0.  (Two runs from the same state: the two tests below.)"""
    p, w, E, V, net = _model()
    net.gemm_precision = prec
    net.fwd_t1_min_blocks = t1
    bt = _batch()
    loss_ref, logits_ref, g = bt["ref"]
    T, tw = cond_ref.T, bt["tw"]
    c = net.forward_causal_block(bt["idx"])
    _, s = net.forward_residual_block(c, t_off=T - tw, condition=cond_ref.IDS)
    lg = net.forward_softmax_block(s, apply_softmax=False)
    loss = net.cross_entropy(lg, bt["tgt"])
    net.zero_grads()
    loss.backward()
    torch.cuda.synchronize()
    gE = to_np(net.global_condition_embed.W.grad).reshape(E.shape)
    assert not gE[1].any() and gE[0].any() and gE[2].any()
    loose = prec == "bf16"
    assert abs(float(loss.detach()) - loss_ref) < (2e-2 * max(1.0, abs(loss_ref)) if loose else 1e-4)
    if not loose:
        np.testing.assert_allclose(to_np(lg), logits_ref, atol=ATOL)
    for ln, kind, off, n, shape in net._spans:
        name = {"global_condition_embed": "E", "global_condition_projection": "V"}.get(ln.name, "%s/%s" % (ln.name, kind))
        want = g[name].reshape(shape)
        got = to_np(net._grad_arena[off:off + n].view(shape))
        if loose:
            rel = np.linalg.norm((got - want).astype(np.float64)) / (np.linalg.norm(want.astype(np.float64)) + 1e-30)
            assert rel < 0.15, (ln.name, rel)
        else:
            scale = max(np.abs(want).max(), 1e-6)
            assert np.abs(got - want).max() <= 2e-4 * scale + 1e-7, (ln.name, kind, np.abs(got - want).max(), scale)
    # the one-call loss of the training step is the same number
    l2 = default_loss(net, dev(bt["idx"]), dev(bt["tgt"]), condition=cond_ref.IDS)
    assert abs(float(l2.detach()) - float(loss.detach())) < (2e-2 if loose else 1e-5 * max(1.0, abs(loss_ref)) + 2e-6)


def _two_runs(net, idx, tgt, ids, tw):
    """Gradient arenas of two forward + backward passes from the same state, and the tensors in which they differ."""
    arenas = []
    for run in range(2):
        c = net.forward_causal_block(idx)
        _, s = net.forward_residual_block(c, t_off=idx.shape[1] - tw, **({} if ids is None else {"condition": ids}))
        loss = net.cross_entropy(net.forward_softmax_block(s, apply_softmax=False), tgt)
        net.zero_grads()
        loss.backward()
        torch.cuda.synchronize()
        arenas.append(net._grad_arena.clone())
    differ = {"%s/%s" % (ln.name, kind): float((arenas[0][off:off + n] - arenas[1][off:off + n]).abs().max())
              for ln, kind, off, n, shape in net._spans if not torch.equal(arenas[0][off:off + n], arenas[1][off:off + n])}
    return arenas, differ


@pytest.mark.parametrize("t1", [1, None])
def test_two_conditioned_runs_give_identical_bits_where_the_unconditioned_step_does(t1):
    """Default arithmetic (fp16x2), a model of the shape whose UNCONDITIONED step is bit-reproducible (tests/test_gpu_parity.py
    test_training_steps_of_the_fast_path_are_bit_reproducible: 256 skip channels and at least 8 layers, so that the skip
    weight gradient takes the fixed-order wide kernel): 2 x 4 layers of 32 channels, head [256, 256], B = 3, T = 70.  What
    conditioning adds to the step -- the COND forward, the per-layer backward with its weight-gradient tiles summed in a fixed
    order (k_layer_bwd_reduce_fixed), the per-clip column sums, the conditioning node's embedding gradient -- uses no float
    atomic: every gradient of two runs from the same state is identical."""
    over = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 4, residual_num_blocks=2,
                softmax_conv_channels=[256, 256])
    p = R.make_params(**over)
    w = R.init_weights(p, 1234)
    E, V = cond_ref.init_condition(p)
    net = WaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    net.load_state_dict(cond_ref.state_dict(w, E, V))
    net.to_gpu()
    net.gemm_precision = "fp16x2"
    net.fwd_t1_min_blocks = t1
    bt = _batch()
    arenas, differ = _two_runs(net, bt["idx"], bt["tgt"], cond_ref.IDS, bt["tw"])
    assert float(arenas[0].abs().max()) > 0 and not differ, differ


@pytest.mark.parametrize("prec", ["fp16x2", "bf16x3", "fp32"])
def test_two_conditioned_runs_give_identical_bits_on_the_tiny_model(prec):
    """The tiny model (64 skip channels, 6 layers): two runs from the same state give identical bits in every gradient.
    At this skip width the skip weight gradient does not take the 256-channel kernel with its fixed-order reduction but
    k_wgrad_b3 (k_wgrad_mfma under fp32 arithmetic), which leaves with one float atomic per workgroup and address -- an UNCONDITIONED tiny model's six
    ``projection_softmax/W`` gradients differ in the last bit between runs (9e-10 to 2e-9 on values of order 1e-2).  A call with
    per-clip bias rows asks that kernel for plain stores of per-workgroup tiles instead, added in workgroup order by
    k_wgrad_fixed_reduce (WGArgs.fixed_part), so the conditioned step is reproducible at every width."""
    _, _, _, _, net = _model()
    net.gemm_precision = prec
    bt = _batch()
    arenas, differ = _two_runs(net, bt["idx"], bt["tgt"], cond_ref.IDS, bt["tw"])
    for _ in range(3):                                                  # an order-dependent sum shows within a few repeats
        more, d2 = _two_runs(net, bt["idx"], bt["tgt"], cond_ref.IDS, bt["tw"])
        differ.update(d2)
        assert torch.equal(more[0], arenas[0])
    print("tiny model, repeated runs: tensors that differ and by how much:", differ)
    assert float(arenas[0].abs().max()) > 0 and not differ, differ


def test_a_conditioned_model_needs_ids_and_an_unconditioned_one_refuses_them():
    p, w, E, V, net = _model()
    bt = _batch()
    x = dev(bt["idx"])
    with pytest.raises(Exception, match="pass condition="):
        net.forward_one_step(x)
    with pytest.raises(Exception, match="pass condition="):
        net.token_nll(x, dev(bt["tgt"]))
    with pytest.raises(Exception, match="forward_residual_block"):
        net.residual_blocks[0][0](net.forward_causal_block(x))
    plain = WaveNet(Params(p), seed=0)
    plain.to_gpu()
    with pytest.raises(Exception, match="no global conditioning"):
        plain.forward_one_step(x, condition=cond_ref.IDS)
    with pytest.raises(Exception, match="no global conditioning"):
        TrainStepGraph(plain, x, dev(bt["tgt"]), condition=cond_ref.IDS)


def test_train_step_graph_replays_a_conditioned_step_and_follows_the_id_buffer():
    """Three replayed conditioned steps land on the weights of three op-by-op steps, to the agreement
    test_train_step_graph_replay_equals_eager_steps demands (2e-5; Adam's eps raised as there).  The ids change between the
    replays: a graph that kept the captured ids would train other embedding rows than the eager model."""
    _, _, _, _, eager = _model()
    _, _, _, _, graphed = _model()
    for n in (eager, graphed):
        n.update_laerning_rate(0.01)
        n.optimizer.eps = 1e-3
    B, T = cond_ref.B, cond_ref.T
    iw = eager.input_width
    rs = np.random.RandomState(0)
    batches = [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, T - iw)).astype(np.int32)), ids)
               for ids in ([2, 0, 2], [1, 1, 0], [0, 2, 1])]
    w0 = to_np(graphed._arena).copy()
    g = TrainStepGraph(graphed, batches[0][0], batches[0][1], condition=batches[0][2])
    np.testing.assert_array_equal(to_np(graphed._arena), w0)          # capture + warm-up did not train
    if graphed.use_step_plan:
        assert graphed.plan_stats()["state"] == 2                     # a conditioned step runs WITH the step plan
    e0 = to_np(eager.global_condition_embed.W).copy()
    for x, tg, ids in batches:
        eager.backprop(default_loss(eager, x, tg, condition=ids))
        assert np.isfinite(float(g.step(x, tg, condition=ids)))
        if ids == [2, 0, 2]:
            moved = np.abs(to_np(eager.global_condition_embed.W) - e0).reshape(3, -1).max(1)
            assert moved[1] == 0.0 and moved[0] > 0 and moved[2] > 0  # class 1 was absent from the first batch
    a, b = to_np(eager._arena), to_np(graphed._arena)
    assert np.abs(a - w0).max() > 1e-3
    np.testing.assert_allclose(b, a, atol=2e-5)
    # the same batch under other ids gives another loss: the replay reads the buffer, not the captured values
    x, tg, _ = batches[0]
    la = float(g.step(x, tg, condition=[0, 0, 0]))
    with torch.no_grad():
        graphed._arena.copy_(torch.as_tensor(b).cuda())               # the loss of a step is that of the weights it starts from
    lb = float(g.step(x, tg, condition=[1, 1, 1]))
    with torch.no_grad():
        graphed._arena.copy_(torch.as_tensor(b).cuda())
    lc = float(g.step(x, tg, condition=[0, 0, 0]))
    assert la == lc and abs(la - lb) > 1e-4, (la, lb, lc)


def _biased_twin(p, w, net, c):
    """An ordinary biased FasterWaveNet holding condition_biases(c) as wf/b and wg/b."""
    pb = dict(p, residual_conv_dilation_no_bias=False)
    sd = dict(w)
    pres = ["residual_%d_block_%d_" % (b, li) for b in range(p["residual_num_blocks"])
            for li in range(len(p["residual_conv_channels"]))]
    for pre, (bf, bg) in zip(pres, net.condition_biases(c)):
        sd[pre + "wf/b"], sd[pre + "wg/b"] = to_np(bf), to_np(bg)
    twin = FasterWaveNet(Params(pb), seed=0)
    twin.load_state_dict(sd)
    twin.to_gpu()
    return twin


def test_conditioned_generation_is_the_biased_models_generation_bit_for_bit():
    """generate(condition=c): tokens and probability trace are those of an ordinary biased model loaded with
    condition_biases(c); generate_batch with ids [0, 2, 1]: row u is the single run with c_u; condition_biases against numpy
    within the float32 rounding of a ``channels``-term dot product."""
    p, w, E, V, net = _model(cls=FasterWaveNet)
    n = 24
    u = np.random.RandomState(7).random_sample((3, n))
    singles = {}
    for c in (0, 2, 1):
        biases = net.condition_biases(c)
        want = V.astype(np.float64) @ E[c].astype(np.float64)
        bound = (cond_ref.CHANNELS + 1) * U32 * (np.abs(V).astype(np.float64) @ np.abs(E[c]).astype(np.float64))
        for (of, og, cd), (bf, bg) in zip(cond_ref.cond_rows(p)[0], biases):
            assert np.all(np.abs(to_np(bf) - want[of:of + cd]) <= bound[of:of + cd] + 1e-30)
            assert np.all(np.abs(to_np(bg) - want[og:og + cd]) <= bound[og:og + cd] + 1e-30)
        toks, probs = net.generate(n, u[(0, 2, 1).index(c)], return_probs=True, condition=c)
        twin = _biased_twin(p, w, net, c)
        t2, p2 = twin.generate(n, u[(0, 2, 1).index(c)], return_probs=True)
        assert torch.equal(toks, t2) and torch.equal(probs, p2), c
        singles[c] = toks
    assert len({tuple(to_np(t)) for t in singles.values()}) > 1       # the voices differ
    rows = net.generate_batch(n, u, condition=[0, 2, 1])
    for i, c in enumerate((0, 2, 1)):
        assert torch.equal(rows[i], singles[c]), (i, c)
    with pytest.raises(Exception, match="pass condition="):
        net.generate(4, u[0])
    with pytest.raises(Exception):
        net.generate_batch(4, u, condition=[0, 1])


def test_conditioned_scoring_is_the_conditioned_training_loss_and_depends_on_the_id():
    """The mean of token_nll(condition=ids) is the conditioned training loss (1e-5 relative, the agreement
    tests/test_gpu_scoring.py uses), and scoring one clip under two ids gives different values."""
    _, _, _, _, net = _model()
    bt = _batch()
    x, tgt = dev(bt["idx"]), dev(bt["tgt"])
    want = float(default_loss(net, x, tgt, condition=cond_ref.IDS).detach())
    rows = net.token_nll(x, tgt, condition=cond_ref.IDS)
    assert rows.shape == tuple(bt["tgt"].shape) and not rows.requires_grad
    mean = float(to_np(rows).astype(np.float64).mean())
    assert abs(mean - want) <= 1e-5 * abs(want), (mean, want)
    other = net.token_nll(x, tgt, condition=[0, 0, 2])
    assert not torch.equal(rows[0], other[0]) and torch.equal(rows[1], other[1]) and torch.equal(rows[2], other[2])
    toks = bt["idx"][0]
    a, b = net.score(toks, condition=0), net.score(toks, condition=2)
    assert a.shape == (toks.size,) and float((a - b).abs().max()) > 1e-4
    with pytest.raises(Exception, match="pass condition="):
        net.score(toks)


def test_checkpoints_and_the_weight_average_carry_the_conditioning_tensors(tmp_path):
    """save / load and wavenet.ema.npz round-trip the two new tensors, and ema_weights() swaps them like every weight."""
    _, _, _, _, net = _model()
    net.enable_ema(0.5, warmup=False)
    net.update_laerning_rate(0.01)
    bt = _batch()
    x, tgt = dev(bt["idx"]), dev(bt["tgt"])
    for _ in range(2):
        net.backprop(default_loss(net, x, tgt, condition=cond_ref.IDS))
    sd, ema = net.state_dict(), net.ema_state_dict()
    keys = ("global_condition_embed/W", "global_condition_projection/W")
    for k in keys:
        assert np.abs(sd[k] - ema[k]).max() > 0                       # the average lags the iterate: they are different tensors
    with net.ema_weights():
        inside = net.state_dict()
        loss_avg = float(default_loss(net, x, tgt, condition=cond_ref.IDS).detach())
    for k in keys:
        assert np.array_equal(inside[k], ema[k])
        assert np.array_equal(net.state_dict()[k], sd[k])             # ... and back again
    net.save(str(tmp_path))
    _, _, _, _, other = _model(seed=5, cond_seed=6)
    other.enable_ema(0.5, warmup=False)
    other.load(str(tmp_path))
    for k in keys:
        assert np.array_equal(other.state_dict()[k], sd[k]) and np.array_equal(other.ema_state_dict()[k], ema[k])
    _, _, _, _, avg = _model(seed=5, cond_seed=6)
    avg.load(str(tmp_path), weights="ema")
    assert abs(float(default_loss(avg, x, tgt, condition=cond_ref.IDS).detach()) - loss_avg) <= 1e-6 * max(1.0, abs(loss_avg))


# ---- the command line end to end: two speakers' files -> conditioned training -> checkpoint -> a voice per utterance -> scores
def test_cli_trains_on_speaker_labels_then_generates_and_evaluates(tmp_path):
    import json
    import os
    from scipy.io import wavfile
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import speakers
    from wavenet_amd.train_audio import train as cli_train
    wav = tmp_path / "wav"
    wav.mkdir()
    model = tmp_path / "model"
    model.mkdir()
    sr = 8000
    t = np.arange(2 * sr) / sr
    for name, hz in (("p225_001.wav", 220), ("p300_001.wav", 330)):          # two "speakers": two tones
        wavfile.write(str(wav / name), sr, (0.5 * np.sin(2 * np.pi * hz * t) * 32767).astype(np.int16))
    cfg = {"quantization_steps": 256, "sampling_rate": sr, "causal_conv_channels": [32], "residual_conv_channels": [32] * 4,
           "residual_num_blocks": 2, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
    (model / "wavenet.json").write_text(json.dumps(cfg))
    common = ["-w", str(wav), "-m", str(model), "--seed", "1"]
    loop = ["--lr", "0.003", "--batch-size", "4", "--train-width", "256", "--repeat", "30", "--max-epoch", "2"]
    l1 = cli_train.main(common + loop + ["--speaker-prefix", "--condition-channels", "8"])
    assert speakers.load_table(str(model)) == (["p225", "p300"], 8)
    assert json.loads((model / "wavenet.json").read_text()) == cfg           # wavenet.json is unchanged
    with np.load(str(model / "wavenet.model.npz")) as z:
        assert z["global_condition_embed/W"].shape == (2, 8, 1, 1) and z["global_condition_projection/W"].shape == (512, 8, 1, 1)
    # a resumed run finds the same table and keeps improving; the op-by-op form trains the same model
    l2 = cli_train.main(common + loop + ["--speaker-prefix", "--condition-channels", "8", "--no-graph"])
    assert np.isfinite(l1) and np.isfinite(l2) and l2 < l1, (l1, l2)
    out = str(tmp_path / "gen")
    fns, tokens = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.02", "--fast", "--seed", "2", "--utterances", "2",
                                     "--speaker", "p225", "--speaker", "p300"])
    assert len(fns) == 2 and tokens.shape == (2, int(sr * 0.02) - 1) and tokens.min() >= 0 and tokens.max() < 256
    fn, one = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.02", "--fast", "--seed", "2", "--speaker", "p300"])
    assert one.shape == (int(sr * 0.02) - 1,)
    # the slow path (full window per sample) draws the same first sample from the same seed, weights and speaker
    fn2, slow = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.003", "--seed", "2", "--speaker", "p300"])
    assert slow[0] == one[0]
    with pytest.raises(SystemExit, match="unknown speaker"):
        cli_generate.main(["-m", str(model), "-o", out, "--fast", "--speaker", "p999"])
    with pytest.raises(SystemExit, match="name one"):
        cli_generate.main(["-m", str(model), "-o", out, "--fast"])
    table = cli_evaluate.main(["-w", str(wav), "-m", str(model)])
    assert [r["file"] for r in table["files"]] == ["p225_001.wav", "p300_001.wav"]
    assert all(np.isfinite(r["nats_per_sample"]) and r["samples"] > 0 for r in table["files"])
    os.rename(str(wav / "p300_001.wav"), str(wav / "p999_001.wav"))
    with pytest.raises(SystemExit, match="unknown speaker"):
        cli_evaluate.main(["-w", str(wav), "-m", str(model)])
