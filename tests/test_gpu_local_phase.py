"""A feature phase per clip on the GPU (WnStackDesc.bias_phase_tab; ``local_phase=`` a sequence) against the float64
reference of tests/local_phase_ref.py and, bit for bit, against the scalar-phase call wherever the rule makes the two equal:
a table whose entries all equal p, and, clip by clip, a table of distinct phases against the scalar call with that clip's.

The base case is local_cond_ref's: cond_ref.TINY, B = 3, T = 70, hop 12 -- with the phases (0, 5, 11): a clip on a column
border, one inside a column, one on a column's last position.  A block holds the rows of the worst phase, 11: 7, and 8 in
linear mode.  Every tolerance is the one tests/test_gpu_local_condition.py / tests/test_gpu_local_interp.py use for the same
quantity."""
import json
import os

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
import local_phase_ref as LP
from gpu_util import btc, dev, to_np
from oracle import wavenet_ref as R
from test_gpu_condition import _ex, _split_z
from test_gpu_local_condition import ATOL, PATHS, _grad_rows
from test_gpu_local_interp import WIDE, _LerpStack, _wide
from wavenet_amd import Params, TrainStepGraph, WaveNet, _lib
from wavenet_amd.graph import default_loss
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

PER_CLIP = _lib.WN_EXEC_BIAS_PER_CLIP
GENERIC = _lib.WN_EXEC_FORCE_GENERIC
B, T, HOP = LP.B, LP.T, LP.HOP
PHASES = LP.PHASES
INTERP = [0, 1]
# the five paths of test_gpu_local_condition.PATHS plus the wide shapes (which run bf16x3 there): (over, prec, flags, t1)
ALL_PATHS = [(LP.TINY,) + p for p in PATHS] + [(_wide(Cr, cd), "bf16x3", 0, 0) for Cr, cd in WIDE]
PATH_IDS = ["%s-%d-%d" % p for p in PATHS] + ["wide%dx%d" % s for s in WIDE]


# ---- the residual stack through the C ABI ---------------------------------------------------------------------------------
class _TabStack(_LerpStack):
    """_LerpStack with the table field: ``tab`` is an int32 device tensor (or None: the scalar ``frames[1]`` holds)."""
    tab = None

    def desc(self, bias=None):
        d, keep = super().desc(bias)
        if self.tab is not None:
            d.bias_phase_tab = self.tab.data_ptr()
        return d, keep

    def phases(self, ph):
        """A sequence: a table (and bias_phase = 0).  An int: the scalar field, no table."""
        hop, _, stride = self.frames
        if isinstance(ph, int):
            self.tab, self.frames = None, (hop, ph, stride)
        else:
            self.tab, self.frames = torch.tensor(list(ph), dtype=torch.int32, device="cuda"), (hop, 0, stride)
        return self


def _case(over=LP.TINY, seed=0, hop=HOP, interp=0, pad=0, Bn=B, Tn=T):
    """Stack, input (B, Cr, 1, T) and a (B, n_max, R + pad) block of random rows that differ by clip and frame."""
    st = _TabStack(over)
    st.interp = interp
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((Bn, st.Cr, 1, Tn)).astype(np.float32)
    block = (rs.standard_normal((Bn, LP.rows_needed(Tn, hop, interp), st.R + pad)) * 0.5).astype(np.float32)
    st.frames = (hop, 0, st.R + pad)
    return st, x, block


def _run(st, x, block, prec, flags, t1, t_off=0, window_only=0):
    n, rw = block.shape[1], block.shape[2]
    rc, got = st.fwd(dev(btc(x)), dev(block), _ex(prec, flags | PER_CLIP, n * rw, t1), t_off, window_only)
    assert rc == 0, _lib.lib().wn_last_error()
    return got


_REF = {}


def _reference(key, fn):
    """A float64 reference, computed once and shared (read-only)."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _against_reference(st, x, block, hop, phases, got, key, t_off=0):
    Bn, Tn = x.shape[0], x.shape[3]
    layers, skip, _ = _reference(("fwd",) + key, lambda: LP.stack_forward(st.p, st.w, x, block[:, :, :st.R], hop, phases, st.interp))
    for l in range(st.L):
        np.testing.assert_allclose(to_np(got[0][l]), btc(layers[l][0]), atol=ATOL, err_msg="out %d" % l)
        for k in (1, 2, 3):
            np.testing.assert_allclose(to_np(_split_z(st, got[k], Bn, Tn)[l]), btc(layers[l][k]), atol=ATOL,
                                       err_msg="%s %d" % (("z", "tanh", "sigmoid")[k - 1], l))
    np.testing.assert_allclose(to_np(got[4]), btc(skip)[:, t_off:], atol=ATOL)


def _grad_rows_against_reference(st, x, block, prec, flags, hop, phases, key):
    """dbf / dbg blocks of wn_stack_bwd (started from 0.25) against the float64 reference gradient within 2e-4 of the block's
    largest entry -- the bound test_gpu_local_condition.py and test_gpu_local_interp.py put on the same rows.  The reference
    gives the rows a clip's phase does not reach exactly 0: there the block must still hold the value it started from, and
    so must the padding behind a row."""
    grad, _, dout, dskip, _, _ = _grad_rows(st, x, block, prec, flags)
    want = _reference(("rows",) + key, lambda: LP.stack_row_grads(st.p, st.w, x, block[:, :, :st.R], hop, phases, st.interp,
                                                                    dout, dskip, 21))
    got = to_np(grad)[:, :, :st.R] - 0.25
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("per-clip-phase bias gradient rows (%s, flags %d, hop %d, interp %d): max |row - float64 reference| = %.3g of %.3g"
          % (prec, flags, hop, st.interp, err, scale))
    assert scale > 1e-2 and err <= 2e-4 * scale, (err, scale)
    for b, ph in enumerate(phases):
        n = LP.rows_read(x.shape[3], hop, ph, st.interp)
        assert np.all(want[b, n:] == 0.0) and float((grad[b, n:] - 0.25).abs().max() if n < grad.shape[1] else 0.0) == 0.0, b
    if block.shape[2] > st.R:
        assert float((grad[:, :, st.R:] - 0.25).abs().max()) == 0.0
    return grad


# ---- 1. distinct phases against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("over,prec,flags,t1", ALL_PATHS, ids=PATH_IDS)
def test_a_phase_per_clip_against_the_reference_on_every_path(over, prec, flags, t1, interp):
    """Phases (0, 5, 11): every layer's out, z, tanh, sigmoid and the skip sum against the float64 reference within ATOL, on
    the five paths of test_gpu_local_condition.PATHS and the two wide shapes, in both modes.  Clips hold different rows and
    different phases, so a wrong clip index or a phase taken from another clip shows -- and the scalar call with any ONE of
    the three phases is far from the reference."""
    st, x, block = _case(over, seed=1, interp=interp)
    assert block.shape[1] == (8 if interp else 7)
    got = _run(st.phases(PHASES), x, block, prec, flags, t1)
    _against_reference(st, x, block, HOP, PHASES, got, (str(sorted(over.items())), interp, 1))
    one = _run(st.phases(5), x, block, prec, flags, t1)
    assert float((one[4][1] - got[4][1]).abs().max()) < 5 * ATOL < float((one[4][2] - got[4][2]).abs().max())


# ---- 2. a table of equal phases is the scalar call -------------------------------------------------------------------------
def _fwd_bwd(st, x, block, prec, flags):
    """Forward outputs (t_off = 21) and, through wn_stack_bwd, dx, every weight gradient and the row-gradient block started
    from 0.25 (test_gpu_local_condition._grad_rows: fwd_t1_min_blocks = 1)."""
    n, rw = block.shape[1], block.shape[2]
    rc, acts = st.fwd(dev(btc(x)), dev(block), _ex(prec, flags | PER_CLIP, n * rw, 1), 21)
    assert rc == 0, _lib.lib().wn_last_error()
    grad, _, _, _, dx, gW = _grad_rows(st, x, block, prec, flags)
    return acts, dx, gW, grad


@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("p", [0, 5, 11])
@pytest.mark.parametrize("over,prec,flags,t1", ALL_PATHS, ids=PATH_IDS)
def test_a_table_of_equal_phases_is_the_scalar_call_bit_for_bit(over, prec, flags, t1, p, interp):
    """Table [p, p, p] against bias_phase = p on the same block (sized for the worst phase): every forward output, dx, the
    whole row-gradient block and every weight gradient, bit for bit; the rows a scalar call with p does not have still hold
    the value they started from.  (Weight gradients are compared off WN_EXEC_FORCE_GENERIC only: the any-shape weight-gradient
    kernels leave through float atomics, with or without bias rows -- test_gpu_local_condition.py makes the same exception.)"""
    st, x, block = _case(over, seed=2, interp=interp)
    fwd_t = _run(st.phases([p] * B), x, block, prec, flags, t1)
    a_t, dx_t, g_t, r_t = _fwd_bwd(st, x, block, prec, flags)
    fwd_s = _run(st.phases(p), x, block, prec, flags, t1)
    a_s, dx_s, g_s, r_s = _fwd_bwd(st, x, block, prec, flags)
    for k in range(5):
        assert torch.equal(fwd_t[k], fwd_s[k]) and torch.equal(a_t[k], a_s[k]), k
    assert torch.equal(dx_t, dx_s) and torch.equal(r_t, r_s)
    n = LP.rows_read(T, HOP, p, interp)
    assert float((r_s[:, :n] - 0.25).abs().max()) > 1e-2
    assert n == block.shape[1] or float((r_t[:, n:] - 0.25).abs().max()) == 0.0
    if not flags & GENERIC:
        for k in g_t:
            for l in range(st.L):
                assert torch.equal(g_t[k][l], g_s[k][l]), (k, l)


# ---- 3. distinct phases, clip by clip --------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("over,prec,flags,t1", ALL_PATHS, ids=PATH_IDS)
def test_distinct_phases_are_the_scalar_calls_clip_by_clip_bit_for_bit(over, prec, flags, t1, interp):
    """One batch, one block, the table (0, 5, 11): clip b's outputs, dx and row gradients equal those of the scalar call with
    p_b on the same batch, bit for bit -- on the exact-fp32 and generic paths and on the split-product paths as well.  No
    quantity shared across clips stands in the way: the fp16 x 2 layer kernels scale per tile, z is contracted at its known
    range, and the only batch-wide range words of a stack call are taken over dskip and the weights, which the compared calls
    share."""
    st, x, block = _case(over, seed=3, interp=interp)
    a_t, dx_t, _, r_t = _fwd_bwd(st.phases(PHASES), x, block, prec, flags)
    for b, p in enumerate(PHASES):
        a_s, dx_s, _, r_s = _fwd_bwd(st.phases(p), x, block, prec, flags)
        assert torch.equal(a_t[0][:, b], a_s[0][:, b]) and torch.equal(a_t[4][b], a_s[4][b]), b
        for k in (1, 2, 3):
            for zt, zs in zip(_split_z(st, a_t[k], B, T), _split_z(st, a_s[k], B, T)):
                assert torch.equal(zt[b], zs[b]), (b, k)
        assert torch.equal(dx_t[b], dx_s[b]) and torch.equal(r_t[b], r_s[b]), b
        assert float((r_t[b] - 0.25).abs().max()) > 1e-2
    assert not torch.equal(a_t[4][2], _fwd_bwd(st.phases(0), x, block, prec, flags)[0][4][2])      # ... and the phase matters


# ---- 4. the model: loss, logits and every gradient -------------------------------------------------------------------------
def _model(interp, glob=False, seed=1234):
    p = R.make_params(**LP.TINY)
    w = R.init_weights(p, seed)
    V, h = LR.init_local(p, frames=LP.rows_needed(T, HOP, interp))
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    net = WaveNet(Params(p), seed=0, local_channels=LP.FEATS, local_hop=HOP, local_interp="linear" if interp else "repeat", **kw)
    net.load_state_dict(LR.state_dict(w, V, E, Vg))
    net.to_gpu()
    return p, w, V, h, E, Vg, net


def _batch(interp, glob):
    def make():
        p = R.make_params(**LP.TINY)
        w = R.init_weights(p, 1234)
        V, h = LR.init_local(p, frames=LP.rows_needed(T, HOP, interp))
        E, Vg = cond_ref.init_condition(p) if glob else (None, None)
        rs = np.random.RandomState(8)
        idx = rs.randint(0, 256, (B, T)).astype(np.int32)
        tgt = rs.randint(0, 256, (B, 40)).astype(np.int32)
        ref = LP.train_step_grads(p, w, V, h, HOP, PHASES, interp, idx, tgt, E=E, Vg=Vg, ids=cond_ref.IDS if glob else None)
        return dict(idx=idx, tgt=tgt, tw=40, ref=ref, h=h)
    return _reference(("model", interp, glob), make)


@pytest.mark.parametrize("interp,prec,t1,glob", [
    (0, "fp32", None, False), (0, "fp16x2", 1, False), (0, "fp16x2", None, False), (0, "fp32", None, True), (0, "fp16x2", 1, True),
    (1, "fp32", None, False), (1, "bf16x3", None, False), (1, "fp16x2", 1, False), (1, "fp16x2", None, False),
    (1, "bf16", None, False), (1, "fp32", None, True), (1, "fp16x2", 1, True)])
def test_model_loss_logits_and_every_gradient_with_a_phase_per_clip(interp, prec, t1, glob):
    """``local_phase=[0, 5, 11]``: loss, logits and the gradient of every weight -- ``local_condition_projection/W`` included
    -- and of the features against tests/local_phase_ref.py, with the cases and at the bars of
    test_locally_conditioned_loss_logits_and_every_gradient_against_the_reference (repeat mode) and
    test_interpolating_model_loss_logits_and_every_gradient_against_the_reference (linear mode): 1e-4 on loss and logits,
    2e-4 of a tensor's largest entry on gradients; bf16: 2e-2 on the loss and 15 % in the 2-norm.  With and without global
    conditioning."""
    p, w, V, h, E, Vg, net = _model(interp, glob)
    net.gemm_precision = prec
    net.fwd_t1_min_blocks = t1
    bt = _batch(interp, glob)
    loss_ref, logits_ref, g = bt["ref"]
    tw = bt["tw"]
    feats = dev(h).requires_grad_(True)
    kw = dict(local=feats, local_phase=list(PHASES))
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
    print("loss %.6f against %.6f" % (float(loss.detach()), loss_ref))
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
    assert "V" in seen and np.abs(g["V"]).max() > 1e-4
    close(to_np(feats.grad), g["h"], "h")
    # the same call through token_nll / default_loss, a numpy array of phases and an integer tensor
    l2 = default_loss(net, dev(bt["idx"]), dev(bt["tgt"]), **dict(kw, local=dev(h), local_phase=np.array(PHASES)))
    assert abs(float(l2.detach()) - float(loss.detach())) < 1e-5 * max(1.0, abs(loss_ref)) + 2e-6
    rows = net.token_nll(dev(bt["idx"]), dev(bt["tgt"]), **dict(kw, local=dev(h), local_phase=torch.tensor(PHASES)))
    assert abs(float(rows.double().mean()) - float(l2.detach())) <= (2e-2 if loose else 1e-5) * abs(loss_ref)
    # checked before any device work, naming the clip; and one column short of the worst phase's raises whatever the phases
    with pytest.raises(Exception, match="got 12 for clip 1"):
        net.forward_residual_block(c, **dict(kw, local_phase=[0, 12, 3]))
    with pytest.raises(Exception, match="feature columns"):
        net.forward_residual_block(c, **dict(kw, local=dev(h[:, :, :-1]), local_phase=[0, 0, 0]))


# ---- 5. edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("hop", [1, 32, 33])
@pytest.mark.parametrize("prec,flags,t1", [("fp32", 0, 1), ("fp32", GENERIC, 0), ("fp16x2", 0, 1)])
def test_hops_with_their_first_last_and_middle_phase(prec, flags, t1, hop, interp):
    """hop in {1, 32, 33} (a frame per position; a frame per tile at phase 0; frames that drift against the tiles) with the
    phases (0, hop - 1, hop // 2), and a frame stride with 4 floats of padding behind the rows: forward and gradient rows
    against the reference; the padding stays untouched."""
    phases = (0, hop - 1, hop // 2)
    st, x, block = _case(seed=4 + hop, hop=hop, interp=interp, pad=4)
    key = ("hops", hop, interp)
    got = _run(st.phases(phases), x, block, prec, flags, t1)
    _against_reference(st, x, block, hop, phases, got, key)
    _grad_rows_against_reference(st, x, block, prec, flags, hop, phases, key)


@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("prec,t1", [("bf16x3", 1), ("fp16x2", 1)])
def test_a_phase_per_clip_with_window_only_and_a_ragged_window_offset(prec, t1, interp):
    """The training form of the call: window_only and t_off = 37 (no multiple of 32)."""
    st, x, block = _case(seed=5, interp=interp)
    got = _run(st.phases(PHASES), x, block, prec, 0, t1, t_off=37, window_only=1)
    assert got[4].shape == (B, T - 37, st.Cs)
    _against_reference(st, x, block, HOP, PHASES, got, ("window", interp), t_off=37)


@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("prec,t1", [("fp32", 1), ("fp16x2", 1)])
def test_a_hop_longer_than_the_clip(prec, t1, interp):
    """hop 100 > T = 70 with the phases (0, 13, 30): every clip lies inside frame 0, so in repeat mode the phases change
    nothing, and in linear mode they move every position's weight (alpha = (t + p) / 100): the clips' outputs differ from
    the scalar-phase call's.  Two rows (three in linear mode), of which a clip reads one (two)."""
    phases = (0, 13, 30)
    st, x, block = _case(seed=6, hop=100, interp=interp)
    assert block.shape[1] == 2 + interp
    key = ("long", interp)
    got = _run(st.phases(phases), x, block, prec, 0, t1)
    _against_reference(st, x, block, 100, phases, got, key)
    _grad_rows_against_reference(st, x, block, prec, 0, 100, phases, key)
    zero = _run(st.phases(0), x, block, prec, 0, t1)
    assert torch.equal(zero[4][0], got[4][0])
    assert torch.equal(zero[4][2], got[4][2]) == (interp == 0)


@pytest.mark.parametrize("interp", INTERP)
def test_rows_wholly_below_the_zero_prefix_stay_untouched(interp):
    """hop 2 with the phases (0, 1, 0): at the d = 4 layers (Z = 2) frame 0 of clips 0 and 2 holds t = 0, 1 and frame 0 of clip
    1 holds t = 0 only -- no row that counts.  A gradient row is touched exactly when a position t >= Z reads it (in linear
    mode: as its own frame's row or, with a weight alpha > 0, as the next row of the frame before), on the generic and on the
    fused path."""
    phases = (0, 1, 0)
    st, x, block = _case(seed=7, hop=2, interp=interp)
    st.phases(phases)
    for flags in (GENERIC, 0):
        g = to_np(_grad_rows(st, x, block, "fp32", flags, start=0.5)[0])
        for l, (of, og, cd) in enumerate(st.rows):
            Z = R.conv_pad_and_prefix(T, st.dil[l], 2)[1]
            lay = np.concatenate([g[:, :, of:of + cd], g[:, :, og:og + cd]], axis=2)
            for b, p in enumerate(phases):
                read = {(t + p) // 2 for t in range(Z, T)}
                if interp:                # (a position with alpha = 0 adds 0 * d to the next row: nothing that shows)
                    read |= {(t + p) // 2 + 1 for t in range(Z, T) if (t + p) % 2}
                for f in range(block.shape[1]):
                    moved = float(np.abs(lay[b, f] - 0.5).max()) > 0
                    assert moved == (f in read), (flags, l, b, f)
        Z = R.conv_pad_and_prefix(T, 4, 2)[1]
        assert Z == 2


# ---- 6. the fence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERP)
@pytest.mark.parametrize("over,prec,flags,t1", ALL_PATHS, ids=PATH_IDS)
def test_values_outside_the_hop_are_reduced_into_it(over, prec, flags, t1, interp):
    """A table holding hop + 5, -1 and 3, uploaded through the C ABI past the Python check, runs to completion and equals --
    forward outputs, dx and the row-gradient block, bit for bit -- the call with those values reduced modulo the hop as the
    kernels reduce them, (unsigned) v % hop: 5, 3 (2^32 - 1 = 12 * 357,913,941 + 3) and 3.  The reduction is a fence: with
    every phase inside [0, hop) no access leaves a block sized for phase hop - 1."""
    st, x, block = _case(over, seed=8, interp=interp)
    wild = [HOP + 5, -1, 3]
    want = [(v % 2 ** 32) % HOP for v in wild]
    assert want == [5, 3, 3]
    a_w, dx_w, _, r_w = _fwd_bwd(st.phases(wild), x, block, prec, flags)
    assert st.tab.tolist() == wild
    a_r, dx_r, _, r_r = _fwd_bwd(st.phases(want), x, block, prec, flags)
    for k in range(5):
        assert torch.equal(a_w[k], a_r[k]), k
    assert torch.equal(dx_w, dx_r) and torch.equal(r_w, r_r) and float((r_w - 0.25).abs().max()) > 1e-2


# ---- 7. the replayed step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERP)
def test_train_step_graph_follows_the_phase_buffer(interp):
    """Built with the phases A, step(local_phase=B) lands on the weights of the op-by-op update with B, and the next step with
    A on those of the update with A -- 2e-5 with Adam's eps raised, the bar of
    test_train_step_graph_replays_a_locally_conditioned_step_and_follows_the_feature_buffer.  The step captured with a table
    holds exactly the kernel nodes of the step captured with an int phase: the table adds no launch.  A graph built with an
    int keeps refusing another int, and refuses a sequence; a bad sequence leaves features and phases as they were."""
    eager, net, other = (_model(interp)[-1] for _ in range(3))
    for n in (eager, net, other):
        n.update_laerning_rate(0.01)
        n.optimizer.eps = 1e-3
    iw = eager.input_width
    rs = np.random.RandomState(0)
    nf = LP.rows_needed(T, HOP, interp)
    batches = [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, T - iw)).astype(np.int32)),
                dev(rs.standard_normal((B, LP.FEATS, nf)).astype(np.float32))) for _ in range(3)]
    A, Bp = [0, 5, 11], np.array([7, 0, 3])
    w0 = to_np(net._arena).copy()
    g = TrainStepGraph(net, batches[0][0], batches[0][1], local=batches[0][2], local_phase=A, keep_graph=True)
    np.testing.assert_array_equal(to_np(net._arena), w0)                # capture + warm-up did not train
    if net.use_step_plan:
        assert net.plan_stats()["state"] == 2                           # ... and the step runs WITH the step plan
    for (x, tg, ft), ph in zip(batches, (Bp, A, 4)):                    # (an int is broadcast)
        eager.backprop(default_loss(eager, x, tg, local=ft, local_phase=[4] * B if isinstance(ph, int) else ph))
        loss = float(g.step(x, tg, local=ft, local_phase=ph))
        assert np.isfinite(loss)
        np.testing.assert_allclose(to_np(net._arena), to_np(eager._arena), atol=2e-5)
    assert np.abs(to_np(net._arena) - w0).max() > 1e-3
    # the phases matter: the same batch and weights under A and under B give different losses, under A again the first one
    x, tg, ft = batches[0]
    keep = net._arena.clone()
    losses = []
    for ph in (A, Bp, A):
        with torch.no_grad():
            net._arena.copy_(keep)
        losses.append(float(g.step(x, tg, local=ft, local_phase=ph)))
    assert losses[0] == losses[2] and abs(losses[0] - losses[1]) > 1e-4, losses
    # refused before anything is refilled
    before = (g.local.clone(), g.local_phase.tab.clone())
    with pytest.raises(Exception, match="got 12 for clip 2"):
        g.step(x, tg, local=batches[1][2], local_phase=[0, 0, 12])
    with pytest.raises(Exception, match="holds 2 phases for 3 clips"):
        g.step(x, tg, local=batches[1][2], local_phase=[0, 0])
    assert torch.equal(g.local, before[0]) and torch.equal(g.local_phase.tab, before[1])
    # an int-phase capture: the same kernel nodes, and the raises it always had
    gi = TrainStepGraph(other, x, tg, local=ft, local_phase=5, keep_graph=True)
    assert gi.node_counts()["kernel"] == g.node_counts()["kernel"] > 0
    with pytest.raises(_lib.WaveNetHipError, match="captured with phase 5"):
        gi.step(x, tg, local=ft, local_phase=0)
    with pytest.raises(_lib.WaveNetHipError, match="capture a step with a sequence"):
        gi.step(x, tg, local=ft, local_phase=[5, 5, 5])


# ---- 8. the driver ---------------------------------------------------------------------------------------------------------
def test_cli_trains_on_sample_aligned_crops(tmp_path, monkeypatch):
    """train --local-dir --local-crop sample on a tiny wav: two updates replayed and, resumed from the checkpoint they wrote,
    two op by op; both report a finite loss.  The first batch's tokens are those of the same command without features under
    the same seed, and its phases are not all 0."""
    from scipy.io import wavfile
    from wavenet_amd.train_audio import features as cli_features
    from wavenet_amd.train_audio import train as cli_train
    wav, feat, model, plain = tmp_path / "wav", tmp_path / "feat", tmp_path / "model", tmp_path / "plain"
    for d in (wav, model, plain):
        d.mkdir()
    sr = 8000
    t = np.arange(sr // 2) / sr
    wavfile.write(str(wav / "a.wav"), sr, (0.5 * np.sin(2 * np.pi * 220 * t) * 32767).astype(np.int16))
    cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "64", "--mels", "12", "--win", "256"])
    cfg = {"quantization_steps": 256, "sampling_rate": sr, "causal_conv_channels": [32], "residual_conv_channels": [32] * 4,
           "residual_num_blocks": 2, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
    for d in (model, plain):
        (d / "wavenet.json").write_text(json.dumps(cfg))
    loop = ["-w", str(wav), "--seed", "1", "--lr", "0.003", "--batch-size", "4", "--train-width", "256", "--repeat", "2",
            "--max-epoch", "2"]
    first = []
    draw = cli_train._Crops.draw

    def spy(self, n):
        out = draw(self, n)
        first.append(out)
        return out
    monkeypatch.setattr(cli_train._Crops, "draw", spy)
    local = ["-m", str(model), "--local-dir", str(feat), "--local-hop", "64", "--local-crop", "sample"]
    l1 = cli_train.main(loop + local)
    assert os.path.isfile(str(model / "wavenet.model.npz")) and json.loads((model / "local.json").read_text()) == {"channels": 12, "hop": 64}
    l2 = cli_train.main(loop + local + ["--no-graph"])                       # resumed from the checkpoint, op by op
    assert np.isfinite(l1) and np.isfinite(l2)
    sampled = first[0]
    assert len(first) == 4 and len(sampled) == 4 and len(set(sampled[3].tolist())) > 1
    assert tuple(sampled[2].shape) == (4, 12, frames_needed(int(sampled[0].shape[1]), 64, 63))
    del first[:]
    cli_train.main(loop + ["-m", str(plain)])
    assert len(first[0]) == 2 and torch.equal(first[0][0], sampled[0]) and torch.equal(first[0][1], sampled[1])
