"""GPU: conditioned decoding on the specialised 32/256-channel decoder (WN_DECODER_GATE_ROWS).

The model is config 4's shape at 2 x 5 layers (tests/test_gpu_ragged_generation.py's NINE), locally conditioned at hop 5 with
the random order-1 rows V h -- distinct in every layer and in both halves, so a swapped half, a wrong layer offset or a wrong
row shows at the first step --, with three classes of global conditioning on top where stated.

What is equality is bit for bit: a table of zeros against the unconditioned handle, equal rows against static biases, a batched
row against the utterance's own generate() call.  What is arithmetic is within ATOL = 1e-4 of the model's own teacher-forced
forward, the bar of tests/test_gpu_local_condition.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from gpu_util import dev, to_np
from oracle import wavenet_ref as R
from test_gpu_condition import _biased_twin
from test_gpu_ragged_generation import NINE, _one, _run_batch, _untouched, _utterances, spy
from wavenet_amd import FasterWaveNet, Params, WaveNet, _lib
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

ATOL = 1e-4                      # tests/test_gpu_local_condition.py: fp32 probabilities within 1e-4 absolute
HOP = 5
GATE = _lib.WN_DECODER_GATE_ROWS
Q = 256
INTERP = {"repeat": 0, "linear": 1}


def _model(interp="repeat", glob=False, local=True):
    p = R.make_params(**NINE)
    w = R.init_weights(p, 1234)
    V, _ = LR.init_local(p)
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    if local:
        kw.update(local_channels=LR.FEATS, local_hop=HOP, local_interp=interp)
    net = FasterWaveNet(Params(p), seed=0, **kw)
    net.load_state_dict(LR.state_dict(w, V, E, Vg) if local else (cond_ref.state_dict(w, E, Vg) if glob else w))
    net.to_gpu()
    return p, w, net


class _Dec(object):
    """Decoder handles of the locally conditioned model, of its unconditioned twin (the same weights) and of biased twins, all
    seeded from ONE prefill over one prompt."""

    def __init__(self):
        self.p, self.w, self.net = _model()
        self.plain = _model(local=False)[2]
        assert self.net._nine_workgroup_shape(_lib.default_exec_flags()) and self.plain._nine_workgroup_shape(_lib.default_exec_flags())
        rs = np.random.RandomState(21)
        self.rows = self.net.local_biases(rs.standard_normal((LR.FEATS, 6)).astype(np.float32))       # (6, R) on the device
        self.R, self.Q = int(self.rows.shape[1]), Q
        assert self.R == 64 * 10
        self.tok = dev(rs.randint(0, Q, (1, self.net.input_width)).astype(np.int32))
        self.u = dev(rs.random_sample(16))
        self.handles = []

    def twin(self, row):
        """An ordinary biased FasterWaveNet whose static gate biases are ``row`` (R,)."""
        net = self.net
        net.condition_biases = lambda c: [(row[of:of + lay.cd].clone(), row[og:og + lay.cd].clone())
                                          for lay, (of, og) in zip(net._flat_layers, net._cond_offsets)]
        try:
            return _biased_twin(self.p, self.w, net, 0)
        finally:
            del net.condition_biases

    def desc(self, model, table=None, interp=0, step_limit=0, flag=None):
        """``flag``: None = what the model sets itself; True / False = WN_DECODER_GATE_ROWS forced on / off."""
        d, keep = model._desc(None, table, step_limit)
        if table is not None:
            d.frame_interp = interp
        if flag is not None:
            d.flags = (d.flags | GATE) if flag else (d.flags & ~GATE)
        return d, keep

    def seed(self, handle, state_from):
        check(_lib.lib().wn_decoder_load_state(handle, ptr(self.tok), int(self.tok.shape[1]),
                                               ptr_array([t.contiguous() for t in state_from._last_causal_outputs]),
                                               ptr_array(state_from._last_layer_inputs), None), "wn_decoder_load_state")

    def handle(self, model, state_from, table=None, interp=0, step_limit=0, flag=None):
        d, keep = self.desc(model, table, interp, step_limit, flag)
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        self.seed(h, state_from)
        return h

    def run(self, h, n, u=None, first=7):
        out = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        probs = torch.zeros((n, Q), device="cuda")
        rc = _lib.lib().wn_decoder_run(h, first, ptr(self.u if u is None else u), n, ptr(out), ptr(probs), None)
        torch.cuda.synchronize()
        return rc, out, probs

    def steps(self, h, feed):
        """One wn_decoder_step per token of ``feed`` -> (len(feed), Q) probability rows."""
        rows = torch.zeros((len(feed), Q), device="cuda")
        for k, tk in enumerate(feed):
            check(_lib.lib().wn_decoder_step(h, int(tk), ptr(rows[k]), 1, None), "wn_decoder_step")
        torch.cuda.synchronize()
        return rows

    def is_nine(self, h):
        """What a handle IS shows in the limit wn_decoder_run_batch applies to it (nothing runs)."""
        out = torch.zeros((8,), device="cuda", dtype=torch.int32)
        rc = _lib.lib().wn_decoder_run_batch((C.c_void_p * 29)(*[h.value] * 29), 29, (C.c_int32 * 29)(*[1] * 29),
                                             (C.c_void_p * 29)(*[self.u.data_ptr()] * 29), 8,
                                             (C.c_void_p * 29)(*[out.data_ptr()] * 29), None, 0, None)
        msg = _lib.lib().wn_last_error().decode()
        torch.cuda.synchronize()
        assert int(out.abs().sum()) == 0
        assert (rc, "at most 28" in msg) in ((_lib.WN_ESHAPE, True), (_lib.WN_EARG, False)), (rc, msg)
        return rc == _lib.WN_ESHAPE

    def close(self):
        for h in self.handles:
            _lib.lib().wn_decoder_destroy(h)


@pytest.fixture(scope="module")
def D():
    d = _Dec()
    yield d
    d.close()


# ---- 1. form -----------------------------------------------------------------------------------------------------------------
def test_a_flagged_conditioned_handle_is_a_nine_workgroup_handle(D):
    """29 copies of a flagged handle with a table are refused by count ("at most 28", WN_ESHAPE); the same description without
    the flag gives an any-shape handle, refused as a duplicate (WN_EARG).  So does a flagged one under WN_EXEC_FORCE_GENERIC and
    with projection biases: the flag is about gate biases and tables only."""
    with torch.no_grad():
        D.plain.forward_one_step(D.tok)
    two = torch.stack([D.rows[0], D.rows[1], D.rows[1]]).contiguous()
    assert D.is_nine(D.handle(D.net, D.plain, (two, HOP, 2)))
    assert D.is_nine(D.handle(D.net, D.plain))                                  # flagged, no table, no biases
    assert D.is_nine(D.handle(D.twin(D.rows[0]), D.plain, flag=True))           # flagged, static gate biases
    assert not D.is_nine(D.handle(D.net, D.plain, (two, HOP, 2), flag=False))
    assert not D.is_nine(D.handle(D.twin(D.rows[0]), D.plain))                  # bias tensors alone: as ever
    D.net.exec_flags = _lib.WN_EXEC_FORCE_GENERIC
    try:
        assert not D.is_nine(D.handle(D.net, D.plain, (two, HOP, 2)))
    finally:
        D.net.exec_flags = None
    pb = FasterWaveNet(Params(R.make_params(**dict(NINE, residual_conv_projection_no_bias=False))), seed=3)
    pb.to_gpu()
    assert not D.is_nine(D.handle(pb, D.plain, flag=True))


# ---- 2. zero rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_a_table_of_zeros_changes_no_bit(D, interp):
    """Tokens and probability trace of the unconditioned fast handle, bit for bit: 12 steps of wn_decoder_run (nine
    workgroups) and 12 wn_decoder_step calls (one workgroup)."""
    with torch.no_grad():
        D.plain.forward_one_step(D.tok)
    rc, t_ref, p_ref = D.run(D.handle(D.plain, D.plain), 12)
    assert rc == 0
    zeros = torch.zeros((4, D.R), device="cuda")
    rc, t_z, p_z = D.run(D.handle(D.net, D.plain, (zeros, HOP, 2), INTERP[interp]), 12)
    assert rc == 0, _lib.lib().wn_last_error()
    assert torch.equal(t_z, t_ref) and torch.equal(p_z, p_ref)
    feed = [7] + [int(t) for t in t_ref[:-1].cpu()]
    s_ref = D.steps(D.handle(D.plain, D.plain), feed)
    s_z = D.steps(D.handle(D.net, D.plain, (zeros, HOP, 2), INTERP[interp]), feed)
    assert torch.equal(s_z, s_ref)
    assert float((s_ref - p_ref).abs().max()) <= ATOL and len(set(t_ref.cpu().tolist())) > 3


# ---- 3. equal rows are static biases -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_equal_rows_are_static_gate_biases_bit_for_bit(D, interp):
    r0, r1 = D.rows[0].contiguous(), D.rows[1].contiguous()
    assert float((r0 - r1).abs().max()) > 0.1
    for lay in range(10):                         # distinct in every layer and in both halves
        blocks = [r0[64 * lay + 32 * k:64 * lay + 32 * k + 32] for k in (0, 1)]
        assert float((blocks[0] - blocks[1]).abs().max()) > 0.1
        if lay:
            assert float((blocks[0] - r0[64 * lay - 64:64 * lay - 32]).abs().max()) > 0.1
    tw0 = D.twin(r0)
    with torch.no_grad():
        tw0.forward_one_step(D.tok)                                             # the one prefill every handle is seeded from
    ref = D.handle(tw0, tw0, flag=True)                                         # the flagged handle with static biases r0, no table
    assert D.is_nine(ref)
    rc, t_ref, p_ref = D.run(ref, 12)
    assert rc == 0
    same = torch.zeros((4, D.R + 4), device="cuda")                             # rows 4 floats of padding apart
    same[:, :D.R] = r0
    rc, t_a, p_a = D.run(D.handle(D.net, tw0, (same, HOP, 2), INTERP[interp]), 12)
    assert rc == 0, _lib.lib().wn_last_error()
    assert torch.equal(t_a, t_ref) and torch.equal(p_a, p_ref)
    # the biases matter: the unconditioned handle from the same state gives other rows
    rc, t_0, p_0 = D.run(D.handle(D.plain, tw0), 12)
    assert float((p_0[0] - p_ref[0]).abs().max()) > 1e-3
    if interp == "repeat":
        # two distinct rows, phase 2: steps 0 .. 2 read row 0, step 3 reads row 1
        two = torch.stack([r0, r1, r1]).contiguous()
        rc, t_b, p_b = D.run(D.handle(D.net, tw0, (two, HOP, 2)), 12)
        assert rc == 0, _lib.lib().wn_last_error()
        assert torch.equal(p_b[:3], p_ref[:3]) and torch.equal(t_b[:3], t_ref[:3])
        assert not torch.equal(p_b[3], p_ref[3])
    else:
        # rows r0, r0, r1, r1: steps 0 .. 2 lie between equal rows, step 3 (p = 5) has alpha = 0 -- r0 exactly --, step 4
        # is the first that sees r1
        lin = torch.stack([r0, r0, r1, r1]).contiguous()
        rc, t_b, p_b = D.run(D.handle(D.net, tw0, (lin, HOP, 2), 1), 12)
        assert rc == 0, _lib.lib().wn_last_error()
        assert torch.equal(p_b[:4], p_ref[:4]) and torch.equal(t_b[:4], t_ref[:4])
        assert not torch.equal(p_b[4], p_ref[4])


# ---- 4. arithmetic --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glob", [False, True], ids=["local", "local+global"])
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_decoded_trace_agrees_with_the_teacher_forced_forward(interp, glob):
    """41 samples behind the prefill, phase 3: every row of generate()'s probability trace agrees within ATOL with the model's
    own forward -- the ELU head the decoder uses -- over prompt + emitted tokens with the same features (and class).
    The two forwards must share one zero-prefix pattern (columns t < Z of a dilated layer carry neither convolution nor bias,
    and Z depends on the width): here the prompt is the input width + 16 = 80 positions, so the 64 columns a decoded position
    reads lie behind column 16 = the largest Z of any layer at any width, in the prefill as in the teacher-forced forward.
    wn_decoder_step (one workgroup) fed the run's tokens agrees with the run's rows (nine workgroups) within the same ATOL."""
    p, w, net = _model(interp, glob)
    assert net._nine_workgroup_shape(_lib.default_exec_flags())
    n, ph = 41, 3
    W = net.input_width + 16
    assert net.input_width == 64 and W == 80
    rs = np.random.RandomState(31)
    h = rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, HOP, ph, interp))).astype(np.float32)
    u = rs.random_sample(n)
    prompt = rs.randint(0, Q, (W,)).astype(np.int32)
    kw = dict(condition=1) if glob else {}
    toks, probs = net.generate(n, u, initial_tokens=prompt, return_probs=True, local=h, local_phase=ph, **kw)
    assert _lib.lib().wn_decoder_status(net._dec.h, None) == _lib.WN_OK
    full = np.concatenate([prompt, to_np(toks)[:-1]])[None]
    with torch.no_grad():
        c = net.forward_causal_block(dev(full))
        _, s = WaveNet.forward_residual_block(net, c, local=dev(h[None]), local_phase=ph, **({"condition": [1]} if glob else {}))
        ref = net.forward_softmax_block(s, apply_softmax=True, activation="elu")
    ref = to_np(ref)[0, :, 0, :].T                                   # (W + n - 1, Q); column W - 1 + i predicts token i
    err = float(np.abs(to_np(probs)[1:] - ref[W:]).max())
    print("conditioned fast decode (%s, %s): max |trace - teacher-forced forward| = %.3g" % (interp, "local+global" if glob else "local", err))
    np.testing.assert_allclose(to_np(probs)[1:], ref[W:], atol=ATOL)
    other = net.generate(n, u, initial_tokens=prompt, local=h[:, ::-1].copy(), local_phase=ph, **kw)
    assert not torch.equal(other, toks)                               # the features steer the samples
    if glob:
        assert not torch.equal(net.generate(n, u, initial_tokens=prompt, local=h, local_phase=ph, condition=2), toks)
    # step by step on the one-workgroup kernel, fed the run's tokens
    net.keep_window = False
    with torch.no_grad():
        net.prev_causal_outputs = None
        net.forward_one_step(dev(prompt[None]), local=h, local_phase=ph, **kw)
        rows = [net._forward_one_step(int(t), full_window=False)[0, :, 0, 0].clone() for t in to_np(toks)[:-1]]
    step_err = float((torch.stack(rows) - probs[1:]).abs().max())
    print("    wn_decoder_step against the run: max |difference| = %.3g" % step_err)
    assert step_err <= ATOL
    with pytest.raises(Exception, match="cover fewer samples"):
        net.generate(n + 5, np.concatenate([u, u]), initial_tokens=prompt, local=h, local_phase=ph, **kw)


# ---- 5. batch -------------------------------------------------------------------------------------------------------------------
class _same_weights_seen(object):
    """Records the ``same_weights`` argument of every wn_decoder_run_batch call made inside."""

    def __enter__(self):
        lib = _lib.lib()
        inner = lib.wn_decoder_run_batch
        self.seen = []

        def counted(*a):
            self.seen.append(int(a[7]))
            return inner(*a)
        lib.wn_decoder_run_batch = counted
        self.lib, self.inner = lib, inner
        return self

    def __exit__(self, *exc):
        self.lib.wn_decoder_run_batch = self.inner


@pytest.mark.parametrize("own_weights", [False, True], ids=["same_weights", "own_weights"])
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_batched_rows_are_their_own_generate_calls(monkeypatch, interp, own_weights):
    """Decode lengths 2, 3, 17 and 40 (n_samples one more each: the first sample comes from the prefill, and an utterance of
    n_samples = 2 -- ONE decode step -- sends the whole call to the loop over generate(), the nine-workgroup form's rule,
    checked at the end): a prompt, a table, a phase and a class per utterance, sampling controls on the last one.  One
    launch, no generate() call, row u = utterance u's own generate() bit for bit -- reading one copy of the weights
    (same_weights = 1, although classes and tables differ) and with WAVENET_HIP_BATCH_OWN_WEIGHTS=1 a copy each."""
    if own_weights:
        monkeypatch.setenv("WAVENET_HIP_BATCH_OWN_WEIGHTS", "1")
    else:
        monkeypatch.delenv("WAVENET_HIP_BATCH_OWN_WEIGHTS", raising=False)
    p, w, net = _model(interp, True)
    Wd = net.input_width
    lengths = [3, 4, 18, 41]
    N = len(lengths)
    rs, prompts, u, kw = _utterances(net, lengths, 11)
    phases = [0, 3, 4, 1]
    # (every feature array covers the longest utterance at the worst phase: any of them serves any utterance below)
    hs = [rs.standard_normal((LR.FEATS, frames_needed(Wd + max(lengths) - 1, HOP, HOP - 1, interp))).astype(np.float32) for _ in range(N)]
    kw["condition"] = [2, 0, 1, 0]
    singles = [net.generate(lengths[i], u[i], initial_tokens=prompts[i], local=hs[i], local_phase=phases[i], **_one(kw, i))
               for i in range(N)]
    with spy(net) as s, _same_weights_seen() as seen:
        rows = net.generate_batch(lengths, u, initial_tokens=prompts, local=hs, local_phase=phases, **kw)
    assert s.calls == 0 and seen.seen == [0 if own_weights else 1]
    assert isinstance(rows, list) and len(rows) == N
    for i in range(N):
        assert rows[i].shape == (lengths[i],) and rows[i].dtype == torch.int32 and rows[i].is_cuda
        assert torch.equal(rows[i], singles[i]), i
        assert _lib.lib().wn_decoder_status(net._batch_decs[i], None) == _lib.WN_OK
    # the handles were updated, not re-created, by a second call with other classes and tables
    held = [h.value for h in net._batch_decs]
    kw2 = dict(kw, condition=[1, 2, 0, 2])
    with spy(net) as s:
        again = net.generate_batch(lengths, u, initial_tokens=prompts, local=hs[::-1], local_phase=phases[::-1], **kw2)
    assert s.calls == 0 and [h.value for h in net._batch_decs] == held
    i = 2
    assert torch.equal(again[i], net.generate(lengths[i], u[i], initial_tokens=prompts[i], local=hs[N - 1 - i],
                                              local_phase=phases[N - 1 - i], **_one(kw2, i)))
    # two utterances with the same weights, prompt, uniforms and class, and different tables: each its own generate(), and
    # not each other's -- a kernel that read utterance 0's rows would give two equal rows
    n = 18
    pair = [hs[3], hs[2]]
    with spy(net) as s:
        two = net.generate_batch(n, np.stack([u[2], u[2]]), initial_tokens=prompts[2], local=pair, local_phase=1, condition=1)
    assert s.calls == 0
    for k in range(2):
        assert torch.equal(two[k], net.generate(n, u[2], initial_tokens=prompts[2], local=pair[k], local_phase=1, condition=1)), k
    assert not torch.equal(two[0], two[1])
    # n_samples = [2, 3, 17, 40]: the utterance of one decode step sends the call to the loop, rows equal all the same
    short = [2, 3, 17, 40]
    with spy(net) as s:
        rows = net.generate_batch(short, [r[:n] for r, n in zip(u, short)], initial_tokens=prompts, local=hs, local_phase=phases, **kw)
    assert s.calls == N
    for i in range(N):
        assert torch.equal(rows[i], singles[i][:short[i]]), i                     # a chain: a shorter run is a prefix


# ---- 6. counters and refusals ---------------------------------------------------------------------------------------------------
def test_counters_and_refusals_of_a_flagged_handle(D):
    """The any-shape decoder's rules on a flagged fast handle, refusals before any device work.  3 rows at hop 5 from phase 2
    cover 13 steps in repeat mode.  In linear mode step k reads rows j and j + 1, j = (2 + k) / 5, so the same 3 rows cover
    the 8 steps with j <= 1 (and 4 rows 13, the figure of tests/test_gpu_local_interp.py) -- check_frames' rule, which
    stays as it is."""
    lib = _lib.lib()
    r0, r1 = D.rows[0].contiguous(), D.rows[1].contiguous()
    tw0 = D.twin(r0)
    with torch.no_grad():
        tw0.forward_one_step(D.tok)
    two = torch.stack([r0, r1, r1]).contiguous()
    rc, t_13, p_13 = D.run(D.handle(D.net, tw0, (two, HOP, 2)), 13)
    assert rc == 0, lib.wn_last_error()
    rc, t_x, p_x = D.run(D.handle(D.net, tw0, (two, HOP, 2)), 14)
    assert rc == _lib.WN_EARG and b"frame table of 3 rows" in lib.wn_last_error() and int(t_x.min()) == -1 and float(p_x.abs().max()) == 0.0
    lin = D.handle(D.net, tw0, (two, HOP, 2), 1)
    rc, t_x, p_x = D.run(lin, 9)
    assert rc == _lib.WN_EARG and b"linear interpolation" in lib.wn_last_error() and int(t_x.min()) == -1
    rc, t_l, p_l = D.run(lin, 8)                                                # ... and the handle goes on as a fresh one does
    rc2, t_l2, p_l2 = D.run(D.handle(D.net, tw0, (two, HOP, 2), 1), 8)
    assert rc == 0 and rc2 == 0 and torch.equal(t_l, t_l2) and torch.equal(p_l, p_l2)
    four = torch.stack([r0, r1, r1, r0]).contiguous()
    lin4 = D.handle(D.net, tw0, (four, HOP, 2), 1)
    assert D.run(lin4, 14)[0] == _lib.WN_EARG and D.run(lin4, 13)[0] == 0
    # a run or a step past the rows, after 12 steps run
    hb = D.handle(D.net, tw0, (two, HOP, 2))
    rc, t_b, p_b = D.run(hb, 12)
    assert rc == 0 and torch.equal(t_b, t_13[:12]) and torch.equal(p_b, p_13[:12])
    rc, t_f, p_f = D.run(hb, 2)
    assert rc == _lib.WN_EARG and b"frame table of 3 rows" in lib.wn_last_error()
    assert int(t_f.min()) == -1 and float(p_f.abs().max()) == 0.0               # nothing ran
    # (a run of ONE step is on one workgroup: the row of the nine-workgroup run to rounding, not bit for bit)
    rc, t_last, p_last = D.run(hb, 1, D.u[12:], first=int(t_b[11]))
    assert rc == 0 and float((p_last[0] - p_13[12]).abs().max()) <= ATOL
    row = torch.zeros((Q,), device="cuda")
    assert lib.wn_decoder_step(hb, 3, ptr(row), 1, None) == _lib.WN_EARG and b"frame table" in lib.wn_last_error()
    # an update with another table restarts the count (and re-seeded, the handle decodes that table from its start)
    d, keep = D.desc(D.net, (two, HOP, 2))
    check(lib.wn_decoder_update_weights(hb, C.byref(d), None), "wn_decoder_update_weights")
    D.seed(hb, tw0)
    rc, t_u, p_u = D.run(hb, 13)
    assert rc == 0 and torch.equal(t_u, t_13) and torch.equal(p_u, p_13)
    # ... an update without a table drops it, and one with static biases brings those: the twin's rows
    rc, t_ref, p_ref = D.run(D.handle(tw0, tw0, flag=True), 13)
    assert torch.equal(p_ref[:3], p_13[:3]) and not torch.equal(p_ref[3], p_13[3])
    d, keep = D.desc(tw0, flag=True)
    check(lib.wn_decoder_update_weights(hb, C.byref(d), None), "wn_decoder_update_weights")
    D.seed(hb, tw0)
    rc, t_s, p_s = D.run(hb, 13)
    assert rc == 0 and torch.equal(t_s, t_ref) and torch.equal(p_s, p_ref)
    d, keep = D.desc(D.net)                                                       # neither biases nor a table: the unconditioned rows
    check(lib.wn_decoder_update_weights(hb, C.byref(d), None), "wn_decoder_update_weights")
    D.seed(hb, tw0)
    rc, t_n, p_n = D.run(hb, 13)
    rc2, t_p, p_p = D.run(D.handle(D.plain, tw0), 13)
    assert rc == 0 and rc2 == 0 and torch.equal(t_n, t_p) and torch.equal(p_n, p_p)
    # an update whose flag differs from the handle's is refused, and the handle still decodes
    hc = D.handle(D.net, tw0, (two, HOP, 2))
    rc, _, _ = D.run(hc, 12)
    d, keep = D.desc(D.net, (two, HOP, 2), flag=False)
    assert lib.wn_decoder_update_weights(hc, C.byref(d), None) == _lib.WN_EARG and b"WN_DECODER_GATE_ROWS" in lib.wn_last_error()
    rc, t_c, p_c = D.run(hc, 1, D.u[12:], first=int(t_13[11]))
    assert rc == 0 and float((p_c[0] - p_13[12]).abs().max()) <= ATOL
    plain = D.handle(D.plain, tw0)
    d, keep = D.desc(D.plain, flag=True)
    assert lib.wn_decoder_update_weights(plain, C.byref(d), None) == _lib.WN_EARG and b"WN_DECODER_GATE_ROWS" in lib.wn_last_error()
    # an unflagged fast handle keeps refusing a table with the message it always gave
    d, keep = D.desc(D.net, (two, HOP, 2), flag=False)
    assert lib.wn_decoder_update_weights(plain, C.byref(d), None) == _lib.WN_EARG and b"take no frame table" in lib.wn_last_error()
    rc, t_q, p_q = D.run(plain, 13)
    assert rc == 0 and torch.equal(p_q, p_p)
    # step_limit ends a flagged handle after its own steps; the single-utterance entry points never clamp
    h4 = D.handle(D.net, tw0, (two, HOP, 2), step_limit=4)
    rc, t_x, p_x = D.run(h4, 5)
    assert rc == _lib.WN_EARG and b"step_limit = 4" in lib.wn_last_error() and int(t_x.min()) == -1
    rc, t_4, p_4 = D.run(h4, 4)
    assert rc == 0 and torch.equal(t_4, t_13[:4]) and torch.equal(p_4, p_13[:4])
    assert lib.wn_decoder_step(h4, 3, ptr(row), 1, None) == _lib.WN_EARG and b"step_limit" in lib.wn_last_error()
    # a batched launch: a limit of 6 ends that utterance there, nothing behind it is written; n_u < 2 is refused
    short, wide = D.handle(D.net, tw0, (two, HOP, 2), step_limit=6), D.handle(D.net, tw0, (two, HOP, 2))
    rc, toks, probs = _run_batch(D, [short, wide], 13, D.u)
    assert rc == 0, lib.wn_last_error()
    assert torch.equal(toks[0][:6], t_13[:6]) and torch.equal(probs[0][:6], p_13[:6]) and _untouched(toks[0], probs[0], 6)
    assert torch.equal(toks[1], t_13) and torch.equal(probs[1], p_13)
    one = D.handle(D.net, tw0, (two, HOP, 2), step_limit=1)
    rc, toks, probs = _run_batch(D, [D.handle(D.net, tw0, (two, HOP, 2)), one], 10, D.u)
    assert rc == _lib.WN_EARG and b"utterance 1" in lib.wn_last_error() and b"2 at least" in lib.wn_last_error()
    assert _untouched(toks[0], probs[0], 0) and _untouched(toks[1], probs[1], 0)
    # ... as are handles that disagree on having a table or on frame_interp, and a run past an utterance's rows
    rc, toks, probs = _run_batch(D, [D.handle(D.net, tw0, (two, HOP, 2)), D.handle(D.net, tw0)], 10, D.u)
    assert rc == _lib.WN_EARG and b"frame table" in lib.wn_last_error() and _untouched(toks[0], probs[0], 0)
    rc, toks, probs = _run_batch(D, [D.handle(D.net, tw0, (two, HOP, 2)), D.handle(D.net, tw0, (two, HOP, 2), 1)], 10, D.u)
    assert rc == _lib.WN_EARG and b"frame_interp" in lib.wn_last_error() and _untouched(toks[0], probs[0], 0)
    rc, toks, probs = _run_batch(D, [D.handle(D.net, tw0, (two, HOP, 2)), D.handle(D.net, tw0, (two, HOP, 4))], 12, D.u)
    assert rc == _lib.WN_EARG and b"frame table of 3 rows" in lib.wn_last_error() and _untouched(toks[1], probs[1], 0)
