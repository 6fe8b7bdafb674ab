"""GPU: streaming synthesis -- a ring of feature rows the decoders read in place (WN_DECODER_FRAME_RING, ``open_stream``).

Everything decoded here is equality: whatever the chunking of pushes and pulls and whatever the ring's size, the concatenation of
what a stream's pulls return is what ONE ``generate`` / ``generate_batch`` call returns for the same rows, tokens and ``chosen``,
bit for bit.  "The same rows" is a premise, and the tests that rest on it check it (``_same_rows``): the rows the opening call
projects from the window's columns must be the rows the whole utterance's projection gives for those columns; everything behind
them is fed by ``push_rows`` from the whole utterance's table.  What is arithmetic -- rows made by ``push(features)`` from fewer
columns per projection -- is held to ATOL of tests/test_gpu_local_condition.py against the float64 rows."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
import local_upsample_ref as LU
from gpu_util import CFG2, dev, to_np
from oracle import wavenet_ref as R
from test_gpu_local_condition import ATOL
from test_gpu_ragged_generation import _local_model, spy
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.faster_wavenet import stream_frames
from wavenet_amd.wavenet import coarse_frames_needed, frames_needed

pytestmark = pytest.mark.gpu

Q = 256
# config 4's shape for the decoder -- 32 / 32 / 256 channels, Q = 256 -- at one block of three layers
NINE3 = dict(CFG2, residual_conv_channels=[32] * 3, residual_num_blocks=1)


def _nine_model(interp="repeat", glob=False, hop=5):
    p = R.make_params(**NINE3)
    w = R.init_weights(p, 1234)
    V, _ = LR.init_local(p)
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    net = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=hop, local_interp=interp, **kw)
    net.load_state_dict(LR.state_dict(w, V, E, Vg))
    net.to_gpu()
    assert net._nine_workgroup_shape(_lib.default_exec_flags())
    return net


def _same_rows(net, h, cw, phase=0):
    """The premise of the equalities below: the first rows of the table are the same floats whether the projection runs over
    the window's ``cw`` columns (the opening call) or over the whole utterance's (``generate``).  -> the whole table."""
    rows = net.local_biases(h, phase)
    head = net.local_biases(h[:, :cw], phase)
    assert torch.equal(head, rows[:head.shape[0]]), "the window's rows depend on the columns projected with them"
    return rows


def _drive(st, n, u, pulls, rest=None, lag=None):
    """Pull ``n`` samples in the pieces ``pulls`` (cycled); ahead of every pull feed each utterance the next rows of ``rest[i]``
    -- as many as its ring takes, less ``lag[i]``.  -> (tokens (N, n), chosen or None, [(steps run before, steps, frames fed)
    per launch])."""
    N, Rr = st.book.n, st.ring_frames
    at, toks, ch, done, launches = [0] * N, [], [], 0, []
    for m in itertools.cycle(pulls):
        m = min(m, n - done)
        if rest is not None:
            k = [max(0, min(len(rest[i]) - at[i], st.book.frames(i).current + Rr - (lag[i] if lag else 0) - st.book.fed[i]))
                 for i in range(N)]
            st.push_rows([rest[i][at[i]:at[i] + k[i]] for i in range(N)] if N > 1 else rest[0][at[0]:at[0] + k[0]])
            at = [a + b for a, b in zip(at, k)]
        assert all(a is None or a >= m for a in st.available()), (st.available(), m)
        launches.append((list(st.book.done), st.book.steps_of(m), list(st.book.fed)))
        got = st.pull(m, u[:, done:done + m])
        t, c = got if st.return_chosen else (got, None)
        assert t.shape == (N, m) and t.dtype == torch.int32 and t.is_cuda
        toks.append(t)
        if c is not None:
            ch.append(c)
        done += m
        if done >= n:
            break
    return torch.cat(toks, dim=1), (torch.cat(ch, dim=1) if ch else None), launches


def _slot(book, i, k, Rr):
    return ((book.phases[i] + k) // book.hop) % Rr


# ---- 1. the any-shape kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_any_shape_stream_is_generate_bit_for_bit_across_borders_and_wraps(interp):
    """The tiny locally conditioned model at hop 4, phase 3, a ring of the minimum size for pulls of 7 samples (3 rows, 4 with
    linear interpolation), 60 samples in pulls of 1, 3, 4, 7, 2, 6, 5, 3, ...: launches start and end on frame borders and ring
    wraps -- one wraps exactly at its first step and one exactly at its last, counted below -- and with linear interpolation
    steps read slot R - 1 with the neighbour in slot 0."""
    hop, ph, n, lin = 4, 3, 60, interp == "linear"
    net = _local_model(interp, False, hop=hop)
    W = net.input_width
    rs = np.random.RandomState(41)
    h = rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, hop, ph, interp))).astype(np.float32)
    prompt = rs.randint(0, Q, (W,)).astype(np.int32)
    u = rs.random_sample((1, n))
    cw = frames_needed(W, hop, ph, interp)
    rows = _same_rows(net, h, cw, ph)
    want, want_ch = net.generate(n, u[0], initial_tokens=prompt, local=h, local_phase=ph, return_chosen=True)
    Rr = stream_frames(hop, lin, 0, pull=7).min_ring
    assert Rr == (4 if lin else 3)
    col0 = (ph + W) // hop
    with net.open_stream(initial_tokens=prompt, local=h[:, :cw], local_phase=ph, return_chosen=True, ring_frames=Rr, max_pull=7) as st:
        assert st.book.phases == [(ph + W) % hop] and st.book.fed == [cw - col0]
        got, got_ch, launches = _drive(st, n, u, [1, 3, 4, 7, 2, 6, 5, 3], [rows[cw:]])
        book = st.book
        first = last = edge = 0
        for (d0,), steps, _ in launches:
            ks = range(d0, d0 + steps)
            wraps = [k for k in ks if k > 0 and _slot(book, 0, k, Rr) == 0 and _slot(book, 0, k - 1, Rr) == Rr - 1]
            first += bool(steps and d0 in wraps)
            last += bool(steps and d0 + steps - 1 in wraps)
            edge += sum(_slot(book, 0, k, Rr) == Rr - 1 for k in ks)
        assert first >= 1 and last >= 1 and edge >= 4, (first, last, edge)
        assert book.done == [n - 1] and book.fed[0] > 3 * Rr                        # the ring went round several times
        with pytest.raises(Exception, match="push more first"):
            st.pull(hop * 3, np.zeros((1, hop * 3)))
    assert torch.equal(got[0], want) and torch.equal(got_ch[0], want_ch)
    assert len(set(to_np(want).tolist())) > 8
    # a larger ring, other pieces: the same samples
    with net.open_stream(initial_tokens=prompt, local=h[:, :cw], local_phase=ph, ring_frames=Rr + 3, max_pull=7) as st:
        got2, _, _ = _drive(st, n, u, [7, 7, 1], [rows[cw:]])
    assert torch.equal(got2[0], want)


# ---- 2. the specialised kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
@pytest.mark.parametrize("one_wg", [False, True], ids=["nine", "one_workgroup"])
def test_specialised_stream_of_one_utterance_is_generate_bit_for_bit(monkeypatch, interp, one_wg):
    if one_wg:
        monkeypatch.setenv("WAVENET_HIP_DECODER_ONE_WORKGROUP", "1")
    else:
        monkeypatch.delenv("WAVENET_HIP_DECODER_ONE_WORKGROUP", raising=False)
    hop, ph, n, lin = 5, 2, 48, interp == "linear"
    net = _nine_model(interp, False, hop)
    assert bool(_lib.default_exec_flags() & _lib.WN_DECODER_ONE_WORKGROUP) == one_wg
    W = net.input_width
    rs = np.random.RandomState(43)
    h = rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, hop, ph, interp))).astype(np.float32)
    prompt = rs.randint(0, Q, (W,)).astype(np.int32)
    u = rs.random_sample((1, n))
    cw = frames_needed(W, hop, ph, interp)
    rows = _same_rows(net, h, cw, ph)
    want, want_ch = net.generate(n, u[0], initial_tokens=prompt, local=h, local_phase=ph, return_chosen=True)
    Rr = stream_frames(hop, lin, 0, pull=7).min_ring
    with net.open_stream(initial_tokens=prompt, local=h[:, :cw], local_phase=ph, return_chosen=True, ring_frames=Rr, max_pull=7) as st:
        assert st.book.two_steps == (not one_wg)
        if not one_wg:
            with pytest.raises(Exception, match="ONE decoder step"):
                st.pull(2, u[:, :2])
        got, got_ch, launches = _drive(st, n, u, [3, 2, 5, 4, 7, 2, 6] if not one_wg else [1, 1, 3, 2, 7, 1, 5], [rows[cw:]])
        assert st.book.fed[0] > 2 * Rr
        assert _lib.lib().wn_decoder_status(st._hs[0], None) == _lib.WN_OK
    assert torch.equal(got[0], want) and torch.equal(got_ch[0], want_ch)
    assert len(set(to_np(want).tolist())) > 8


@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_specialised_batched_stream_is_generate_batch_bit_for_bit(interp):
    """Three utterances on the nine-workgroup form: a prompt, a class, a phase, a feature array and a lag of the feed per
    utterance -- so the three rings stand at different slots and hold different numbers of rows at every launch --, sampling
    controls on the last one, pulls of two samples and more.  One batched launch per pull, none of ``generate``."""
    hop, n, N, lin = 5, 45, 3, interp == "linear"
    net = _nine_model(interp, True, hop)
    W = net.input_width
    rs = np.random.RandomState(47)
    phases, classes = [0, 3, 4], [2, 0, 1]
    # (more columns than the samples read, and another number per utterance: the feed never runs dry, so the lags hold)
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, hop, ph, interp) + 8 + i)).astype(np.float32) for i, ph in enumerate(phases)]
    prompts = rs.randint(0, Q, (N, W)).astype(np.int32)
    u = rs.random_sample((N, n))
    kw = dict(temperature=[1.0, 1.0, 0.8], top_k=[0, 0, 20], top_p=[1.0, 1.0, 0.9], condition=classes)
    cws = [frames_needed(W, hop, ph, interp) for ph in phases]
    rows = [_same_rows(net, hs[i], cws[i], phases[i]) for i in range(N)]
    with spy(net) as s:
        want, want_ch = net.generate_batch(n, u, initial_tokens=prompts, local=hs, local_phase=phases, return_chosen=True, **kw)
    assert s.calls == 0
    Rr = stream_frames(hop, lin, 0, pull=7).min_ring + 2
    calls = []
    lib = _lib.lib()
    inner = lib.wn_decoder_run_batch
    lib.wn_decoder_run_batch = lambda *a: (calls.append(int(a[1])), inner(*a))[1]
    try:
        with net.open_stream(utterances=N, initial_tokens=prompts, local=[hs[i][:, :cws[i]] for i in range(N)], local_phase=phases,
                             return_chosen=True, ring_frames=Rr, max_pull=7, **kw) as st, spy(net) as s:
            got, got_ch, launches = _drive(st, n, u, [3, 2, 7, 4, 2, 5, 6], [rows[i][cws[i]:] for i in range(N)], lag=[0, 1, 2])
            for i in range(N):
                assert lib.wn_decoder_status(st._hs[i], None) == _lib.WN_OK
            book = st.book
    finally:
        lib.wn_decoder_run_batch = inner
    assert s.calls == 0 and calls == [N] * len(launches) and len(launches) > 8
    for d0, steps, fed in launches:          # at every launch the rings differ in where they are written or where they are read ...
        assert steps >= 2 and len({(fed[i] % Rr, _slot(book, i, d0[i], Rr)) for i in range(N)}) > 1, (d0, steps, fed)
    for i in range(N):                       # ... and every ring is entered at (almost) every slot by some launch
        assert len({_slot(book, i, d0[i], Rr) for d0, _, _ in launches}) >= Rr - 1
    assert torch.equal(got, want) and torch.equal(got_ch, want_ch)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------
class _Abi(object):
    """Handles of one locally conditioned model, seeded from ONE prefill over one prompt."""

    def __init__(self, net, hop):
        self.net, self.hop, self.handles = net, hop, []
        rs = np.random.RandomState(21)
        self.rows = net.local_biases(rs.standard_normal((LR.FEATS, 12)).astype(np.float32))        # (12, width) on the device
        self.width = int(self.rows.shape[1])
        self.tok = dev(rs.randint(0, Q, (1, net.input_width)).astype(np.int32))
        self.u = dev(rs.random_sample(40))
        with torch.no_grad():
            net.prev_causal_outputs = None
            net.forward_one_step(self.tok, local=rs.standard_normal((LR.FEATS, net.input_width // hop + 3)).astype(np.float32))
        self._keep = ([t.contiguous() for t in net._last_causal_outputs], list(net._last_layer_inputs))     # (later prefills make new ones)
        self.state = (ptr_array(self._keep[0]), ptr_array(self._keep[1]))

    def desc(self, table, ring, interp=0):
        d, keep = self.net._desc(None, table, ring=ring)
        d.frame_interp = interp
        return d, keep

    def handle(self, table, ring, interp=0):
        d, keep = self.desc(table, ring, interp)
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        check(_lib.lib().wn_decoder_load_state(h, ptr(self.tok), int(self.tok.shape[1]), self.state[0], self.state[1], None),
              "wn_decoder_load_state")
        return h

    def run(self, h, n, u, first=7):
        out = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        probs = torch.zeros((n, Q), device="cuda")
        rc = _lib.lib().wn_decoder_run(h, first, ptr(u), n, ptr(out), ptr(probs), None)
        torch.cuda.synchronize()
        return rc, out, probs

    def close(self):
        for h in self.handles:
            _lib.lib().wn_decoder_destroy(h)


@pytest.mark.parametrize("shape", ["any", "nine"])
@pytest.mark.parametrize("interp", [0, 1], ids=["repeat", "linear"])
def test_frame_ring_through_the_c_abi(shape, interp):
    hop, ph = 5, 2
    net = _local_model("linear" if interp else "repeat", False, hop=hop) if shape == "any" else _nine_model("linear" if interp else "repeat", False, hop)
    D = _Abi(net, hop)
    lib = _lib.lib()
    try:
        rows, u = D.rows, D.u
        # the flat table: 12 rows cover (12 - interp) * 5 - 2 steps; the reference for everything below
        rc, t_ref, p_ref = D.run(D.handle((rows, hop, ph), False, interp), 30, u)
        assert rc == 0, lib.wn_last_error()
        # ---- refusals at create, before any device work -------------------------------------------------------------------------
        h = C.c_void_p()
        d, keep = D.desc(None, True)
        assert lib.wn_decoder_create(C.byref(h), C.byref(d), None) == _lib.WN_EARG and b"WN_DECODER_FRAME_RING without frame_bias" in lib.wn_last_error()
        d, keep = D.desc((rows, hop, ph), True, interp)
        d.frame_bias = rows.data_ptr() + 2
        assert lib.wn_decoder_create(C.byref(h), C.byref(d), None) == _lib.WN_EARG and b"multiple of 4 bytes" in lib.wn_last_error()
        d, keep = D.desc((rows, hop, ph), True, interp)
        d.frame_stride = D.width - 1
        assert lib.wn_decoder_create(C.byref(h), C.byref(d), None) == _lib.WN_EARG and b"frame_stride" in lib.wn_last_error()
        assert not h.value
        # ---- a ring of 4 rows, rows 8 floats of padding apart, filled with frames 0 .. 3 ------------------------------------------
        Rr = 4
        ring = torch.zeros((Rr, D.width + 8), device="cuda")
        ring[:, :D.width] = rows[:Rr]
        hr = D.handle((ring, hop, ph), True, interp)
        # a run that reads more than R frames at once: refused, the state left alone
        too_many = (Rr - interp) * hop - ph + 1                                     # one step into frame 4 (linear: into frame 3)
        rc, t_x, p_x = D.run(hr, too_many, u)
        assert rc == _lib.WN_EARG and b"ring of 4 rows" in lib.wn_last_error() and b"cannot be refilled" in lib.wn_last_error()
        assert int(t_x.min()) == -1 and float(p_x.abs().max()) == 0.0
        n1 = too_many - 1
        rc, t_1, p_1 = D.run(hr, n1, u)
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(t_1, t_ref[:n1]) and torch.equal(p_1, p_ref[:n1])
        # ---- by reference: rows rewritten between two runs are read by the second ---------------------------------------------------
        # frames 4 .. 6 go where frames 0 .. 2 were (the flat table's refusal for "past row n_frames - 1" does not apply);
        # the next run starts in frame 3 (linear: 2), wraps, and reads them
        ring[:3, :D.width] = rows[4:7]
        n2 = 10
        assert n1 + n2 <= 30
        rc, t_2, p_2 = D.run(hr, n2, u[n1:], first=int(t_1[-1]))
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(t_2, t_ref[n1:n1 + n2]) and torch.equal(p_2, p_ref[n1:n1 + n2])
        # ... and OTHER rows there give another run: that of a flat table holding them
        other = rows.clone()
        other[4:7] = rows[9:12]
        h_flat = D.handle((other, hop, ph), False, interp)
        rc, t_o, p_o = D.run(h_flat, n1 + n2, u)
        hr2 = D.handle((ring, hop, ph), True, interp)
        ring[:, :D.width] = rows[:Rr]
        rc2, t_a, p_a = D.run(hr2, n1, u)
        ring[:3, :D.width] = rows[9:12]
        rc3, t_b, p_b = D.run(hr2, n2, u[n1:], first=int(t_a[-1]))
        assert rc == 0 and rc2 == 0 and rc3 == 0
        assert torch.equal(torch.cat([t_a, t_b]), t_o) and torch.equal(torch.cat([p_a, p_b]), p_o)
        assert not torch.equal(p_o[n1:], p_ref[n1:n1 + n2])
        # ---- the form is fixed at create ---------------------------------------------------------------------------------------------
        d, keep = D.desc((rows, hop, ph), False, interp)
        assert lib.wn_decoder_update_weights(hr, C.byref(d), None) == _lib.WN_EARG and b"WN_DECODER_FRAME_RING" in lib.wn_last_error()
        d, keep = D.desc((ring, hop, ph), True, interp)
        assert lib.wn_decoder_update_weights(h_flat, C.byref(d), None) == _lib.WN_EARG and b"WN_DECODER_FRAME_RING" in lib.wn_last_error()
        # with the bit kept an update brings another ring and phase and restarts the count
        ring2 = rows[:6].clone()
        d, keep = D.desc((ring2, hop, ph), True, interp)
        check(lib.wn_decoder_update_weights(hr, C.byref(d), None), "wn_decoder_update_weights")
        check(lib.wn_decoder_load_state(hr, ptr(D.tok), int(D.tok.shape[1]), D.state[0], D.state[1], None), "wn_decoder_load_state")
        rc, t_u, p_u = D.run(hr, 20, u)
        assert rc == 0 and torch.equal(t_u, t_ref[:20]) and torch.equal(p_u, p_ref[:20])
        # ---- a batched launch: the handles agree on the flag --------------------------------------------------------------------------
        ring[:, :D.width] = rows[:Rr]
        a, b = D.handle((ring, hop, ph), True, interp), D.handle((rows, hop, ph), False, interp)
        toks = [torch.full((8,), -1, device="cuda", dtype=torch.int32) for _ in range(2)]
        rc = lib.wn_decoder_run_batch((C.c_void_p * 2)(a.value, b.value), 2, (C.c_int32 * 2)(7, 7), ptr_array([u, u]), 8,
                                      ptr_array(toks), None, 0, None)
        msg = lib.wn_last_error()
        torch.cuda.synchronize()
        assert rc == _lib.WN_EARG and b"utterance 1" in msg and b"WN_DECODER_FRAME_RING" in msg and int(toks[0].max()) == -1
        # ... and two ring handles run side by side, each from its own ring: a second ring holding the frames one slot on
        ring_b = torch.zeros((Rr + 1, D.width), device="cuda")
        ring_b[:Rr] = rows[:Rr]
        c = D.handle((ring_b, hop, ph), True, interp)
        rc = lib.wn_decoder_run_batch((C.c_void_p * 2)(a.value, c.value), 2, (C.c_int32 * 2)(7, 7), ptr_array([u, u]), 8,
                                      ptr_array(toks), None, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(toks[0], t_ref[:8]) and torch.equal(toks[1], t_ref[:8])
        for hh in (a, c):
            assert lib.wn_decoder_status(hh, None) == _lib.WN_OK
    finally:
        D.close()


# ---- 4. push(features) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
@pytest.mark.parametrize("U", [1, 2])
def test_pushed_features_make_the_rows_of_the_projection(U, interp):
    """Features pushed a few columns at a time -- one column, none, three, five: the rows found in the ring lie within ATOL (tests/test_gpu_local_condition.py,
    tests/test_gpu_local_upsample.py) of the float64 rows V y, y the float64 layer's fine features (U = 2) or the features
    themselves.  Pushed in ONE call, the rows are ``net.local_biases`` of the same columns, bit for bit."""
    H = 12
    p = R.make_params(**LR.TINY)
    V = LR.init_local(p)[0]
    sd = LR.state_dict(R.init_weights(p, 1234), V)
    Wu = LU.random_weight(U, LR.FEATS) if U > 1 else None
    net = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=H, local_interp=interp, local_upsample=U)
    net.load_state_dict(dict(sd, **({"local_condition_upsample/W": Wu.reshape(U * LR.FEATS, 2 * LR.FEATS, 1, 1)} if U > 1 else {})))
    net.to_gpu()
    W, fine = net.input_width, H // U
    rs = np.random.RandomState(51)
    cw = coarse_frames_needed(W, H, U, 0, interp)
    h = rs.standard_normal((LR.FEATS, cw + 9)).astype(np.float32)
    y = LU.upsample(Wu, h[None])[0] if U > 1 else h.astype(np.float64)             # (F, fine columns)
    want = (V.astype(np.float64) @ y).T                                            # (fine columns, width)
    col0 = W // fine
    Rr = 64
    with net.open_stream(local=h[:, :cw], ring_frames=Rr, max_pull=8) as st:
        fed0 = st.book.fed[0]
        assert fed0 == (cw - 1) * U - col0 if U > 1 else fed0 == cw - col0
        for a, b in ((cw, cw + 1), (cw + 1, cw + 1), (cw + 1, cw + 4), (cw + 4, cw + 9)):
            st.push(h[:, a:b])
        total = st.book.fed[0]
        assert total == fed0 + 9 * U
        got = to_np(st._rings[0][:total])
        err = float(np.abs(got - want[col0:col0 + total]).max())
        print("push(features), U = %d: max |ring row - float64| = %.3g of %.3g" % (U, err, np.abs(want).max()))
        assert np.abs(want).max() > 0.5 and err <= ATOL
        with pytest.raises(Exception, match=r"utterance 0: %d more rows on top of the %d fed would overwrite" % (Rr * U, total)):
            st.push(np.zeros((LR.FEATS, Rr), np.float32))
    with net.open_stream(local=h[:, :cw], ring_frames=Rr, max_pull=8) as st:
        st.push(h[:, cw:])
        one = net.local_biases(h[:, cw - 1:] if U > 1 else h[:, cw:])
        assert torch.equal(st._rings[0][fed0:fed0 + one.shape[0]], one) and st.book.fed[0] == fed0 + one.shape[0] == total


# ---- 5. streams without a ring ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["any", "nine"])
def test_unconditioned_and_globally_conditioned_streams_are_generate_batch(shape):
    over = LR.TINY if shape == "any" else NINE3
    p = R.make_params(**over)
    w = R.init_weights(p, 1234)
    E, Vg = cond_ref.init_condition(p)
    plain = FasterWaveNet(Params(p), seed=0)
    plain.load_state_dict(w)
    plain.to_gpu()
    glob = FasterWaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    glob.load_state_dict(cond_ref.state_dict(w, E, Vg))
    glob.to_gpu()
    rs = np.random.RandomState(53)
    n, N = 33, 3
    u = rs.random_sample((N, n))
    prompts = rs.randint(0, Q, (N, plain.input_width)).astype(np.int32)
    pulls = [3, 2, 6, 9] if shape == "nine" else [1, 1, 4, 2, 9]
    for net, kw in ((plain, {}), (glob, dict(condition=[1, 0, 2]))):
        want, want_ch = net.generate_batch(n, u, initial_tokens=prompts, return_chosen=True, top_k=[0, 30, 0], **kw)
        with net.open_stream(utterances=N, initial_tokens=prompts, return_chosen=True, top_k=[0, 30, 0], **kw) as st:
            assert st.available() == [None] * N and st.ring_frames == 0
            with pytest.raises(Exception, match="has no ring"):
                st.push_rows([np.zeros((1, 4), np.float32)] * N)
            got, got_ch, _ = _drive(st, n, u, pulls)
        assert torch.equal(got, want) and torch.equal(got_ch, want_ch)
        with pytest.raises(Exception, match="closed"):
            st.pull(2, u[:, :2])
        # one utterance: wn_decoder_run
        w1 = net.generate(n, u[1], initial_tokens=prompts[1], top_k=30, **({"condition": 0} if kw else {}))
        with net.open_stream(initial_tokens=prompts[1], top_k=30, **({"condition": 0} if kw else {})) as st:
            g1, _, _ = _drive(st, n, u[1:2], pulls)
        assert torch.equal(g1[0], w1)


# ---- 6. the command --------------------------------------------------------------------------------------------------------------
def test_generate_chunk_frames_end_to_end(tmp_path, capsys):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import generate as cli_generate
    hop, sr, extra = 4, 8000, 11
    model = tmp_path / "model"
    model.mkdir()
    net = _local_model("linear", False, hop=hop)
    W = net.input_width
    assert W % hop == 0
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(LR.TINY, sampling_rate=sr)))
    (model / "local.json").write_text(json.dumps({"channels": LR.FEATS, "hop": hop, "interp": "linear"}))
    feat = str(tmp_path / "f.npy")
    np.save(feat, np.random.RandomState(16).standard_normal((LR.FEATS, W // hop + extra)).astype(np.float32))
    want = extra * hop + 1                                                         # (W / hop + extra) hop - W + 1
    common = ["-m", str(model), "--fast", "--seed", "2", "--local", feat]
    whole, t_whole = cli_generate.main(common + ["-o", str(tmp_path / "whole")])
    assert t_whole.shape == (want,)
    capsys.readouterr()
    # three columns at a time: the expected length, a file per sample as the writer counts them, the time to the first chunk
    fn, t_3 = cli_generate.main(common + ["-o", str(tmp_path / "c3"), "--chunk-frames", "3"])
    rate, pcm = wavfile.read(fn)
    assert rate == sr and pcm.shape[0] == want and t_3.shape == (want,)
    assert "first chunk (" in capsys.readouterr().out
    # C >= the columns: one projection over the same array, the same bytes
    fn, t_all = cli_generate.main(common + ["-o", str(tmp_path / "call"), "--chunk-frames", "1000"])
    np.testing.assert_array_equal(t_all, t_whole)
    assert open(fn, "rb").read() == open(whole, "rb").read()
    # --report and --best-of: chosen collected per pull
    rep = tmp_path / "r.json"
    fn, t_b = cli_generate.main(common + ["-o", str(tmp_path / "best"), "--chunk-frames", "3", "--best-of", "3", "--report", str(rep)])
    table = json.loads(rep.read_text())
    assert t_b.shape == (want,) and table["files"][0]["samples"] == want and len(table["files"][0]["candidates"]) == 3
    assert table["files"][0]["nats_per_sample"] == min(table["files"][0]["candidates"])
    assert wavfile.read(fn)[1].shape[0] == want


def test_a_stream_of_more_utterances_than_a_launch_takes_is_dealt_over_launches():
    """30 unconditioned utterances on the nine-workgroup form, whose launches take 28: every pull is two launches, 28 and 2, and the
    rows are ``generate_batch``'s."""
    p = R.make_params(**NINE3)
    net = FasterWaveNet(Params(p), seed=0)
    net.load_state_dict(R.init_weights(p, 1234))
    net.to_gpu()
    lib = _lib.lib()
    N, n = int(lib.wn_decoder_batch_max()) + 2, 12
    rs = np.random.RandomState(59)
    u = rs.random_sample((N, n))
    prompts = rs.randint(0, Q, (N, net.input_width)).astype(np.int32)
    want = net.generate_batch(n, u, initial_tokens=prompts)
    calls = []
    inner = lib.wn_decoder_run_batch
    lib.wn_decoder_run_batch = lambda *a: (calls.append(int(a[1])), inner(*a))[1]
    try:
        with net.open_stream(utterances=N, initial_tokens=prompts) as st:
            got, _, launches = _drive(st, n, u, [4, 3, 5])
    finally:
        lib.wn_decoder_run_batch = inner
    assert calls == [N - 2, 2] * len(launches) and len(launches) == 3
    assert torch.equal(got, want) and len({tuple(r) for r in to_np(got).tolist()}) > N // 2
