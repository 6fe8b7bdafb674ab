"""GPU: batched decoding in utterance tiles (``wn_decoder_run_batch`` with ``same_weights`` = U in {2, 4, 8, 16} on any-shape
handles; ``generate_batch(..., tile=U)``, ``open_stream(..., tile=U)``).

Workgroup g of ``k_decode_tile<U>`` decodes utterances [gU, gU + U) of a launch against handle 0's copy of the weights and forms
every output element by ``decode_steps``' operations in its order, so everything here is equality, bit for bit: a row is the row
``generate`` gives, a trace the trace of ``wn_decoder_run`` on a twin handle (floats compared as ``uint32``).  What shows that the
tile kernel ran is the ``same_weights`` argument the launches carried (spied) and, in the C ABI tests, the flag itself -- and that
the weights really are shared shows in test 4, where handle 1 holds OTHER weights and still decodes with handle 0's.

The models are those of test_gpu_batched_generation.py, restated: A (Q = 256, one causal layer, fw 2) and B (Q = 64, two causal
layers of filter width 3, residual filter width 3).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from gpu_util import CFG2, build, to_np
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd.faster_wavenet import stream_frames, tile_fit
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

A = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[16] * 4, residual_num_blocks=2,
         softmax_conv_channels=[32, 256])
B = dict(quantization_steps=64, causal_conv_channels=[8, 8], causal_conv_filter_width=3, residual_conv_filter_width=3,
         residual_conv_channels=[8] * 3, residual_num_blocks=2, softmax_conv_channels=[16, 64])
CFGS = {"A": A, "B": B}
NMAX, LONGEST = 2 * 16 + 3, 20
_MODELS = {}


def model(name):
    """(oracle params, oracle weights, GPU model, uniforms (35, 20), the oracle's rows, generate()'s rows): built once."""
    if name not in _MODELS:
        p, w, net = build(CFGS[name], cls=FasterWaveNet)
        u = np.random.RandomState(7 * len(name) + ord(name[0])).random_sample((NMAX, LONGEST))
        oracle = np.stack([R.generate(p, w, LONGEST, u[i], fast=True) for i in range(NMAX)])
        single = np.stack([to_np(net.generate(LONGEST, u[i])) for i in range(NMAX)])
        _MODELS[name] = (p, w, net, u, oracle, single)
    return _MODELS[name]


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def _bits(t):
    return to_np(t).view(np.uint32)


class launches(object):
    """``with launches(net) as l:`` -- ``l.same`` lists the ``same_weights`` argument of every ``wn_decoder_run_batch`` call made
    inside, and any call of ``net.generate`` inside fails the block."""

    def __init__(self, net):
        self.net, self.same, self.loops = net, [], 0

    def __enter__(self):
        lib = _lib.lib()
        self._inner, self._gen = lib.wn_decoder_run_batch, self.net.generate

        def run_batch(*a):
            self.same.append(int(a[7]))
            return self._inner(*a)

        def gen(*a, **kw):
            self.loops += 1
            return self._gen(*a, **kw)
        lib.wn_decoder_run_batch, self.net.generate = run_batch, gen
        return self

    def __exit__(self, *exc):
        _lib.lib().wn_decoder_run_batch = self._inner
        del self.net.generate
        if exc[0] is None:
            assert self.loops == 0, "generate_batch ran generate() %d times instead of a batched launch" % self.loops


# ---- 1. rows equal generate() and the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [2, 4, 8, 16])
@pytest.mark.parametrize("name", ["A", "B"])
def test_tiled_rows_equal_generate_and_the_oracle(name, U):
    """N = 1 (no tile: one live utterance), U - 1 (one short tile), U, U + 1 (a tile and a tile of one), 2U + 3; n = 2 (one decode
    step) and 20."""
    p, w, net, u, oracle, single = model(name)
    np.testing.assert_array_equal(single, oracle)
    for N in sorted({1, U - 1, U, U + 1, 2 * U + 3}):
        for n in (2, 20):
            with launches(net) as l:
                got = to_np(net.generate_batch(n, u[:N, :n], tile=U))
            assert l.same == [U if N > 1 else 1], (N, n, l.same)
            assert got.shape == (N, n) and got.dtype == np.int32
            np.testing.assert_array_equal(got, single[:N, :n], err_msg="N = %d, n = %d" % (N, n))
            np.testing.assert_array_equal(got, oracle[:N, :n], err_msg="N = %d, n = %d" % (N, n))


# ---- 2. a length per utterance inside one tile ----------------------------------------------------------------------------------
@pytest.mark.parametrize("longest_first", [True, False])
@pytest.mark.parametrize("U", [4, 8])
@pytest.mark.parametrize("name", ["A", "B"])
def test_a_length_per_utterance_inside_one_tile(name, U, longest_first):
    """Slots of one tile end at steps of their own (one utterance decodes nothing and joins no launch); every utterance's uniforms
    are an array of exactly its own length, and in the (N, max) variant NaN sits behind every prefix."""
    net, u, single = model(name)[2], model(name)[3], model(name)[5]
    lengths = [20, 3, 11, 1, 7, 20, 2, 5]
    N = len(lengths)
    net.batch_longest_first = longest_first
    try:
        with launches(net) as l:
            got = net.generate_batch(lengths, [u[i, :n].copy() for i, n in enumerate(lengths)], tile=U)
        shared = np.full((N, max(lengths)), np.nan)
        for i, n in enumerate(lengths):
            shared[i, :n] = u[i, :n]
        with launches(net) as l2:
            got2 = net.generate_batch(lengths, shared, tile=U)
    finally:
        del net.batch_longest_first
    assert l.same == [U] and l2.same == [U]
    for i, n in enumerate(lengths):
        assert got[i].shape == (n,) and got2[i].shape == (n,)
        np.testing.assert_array_equal(to_np(got[i]), single[i, :n], err_msg="utterance %d" % i)
        np.testing.assert_array_equal(to_np(got2[i]), single[i, :n], err_msg="utterance %d (shared array)" % i)


# ---- 3. the C ABI on twin handles -----------------------------------------------------------------------------------------------
class _Seeded(object):
    """Decoder handles of one model, all seeded from ONE prefill over one window."""

    def __init__(self, net, window, **prefill):
        self.net, self.lib, self.hs = net, _lib.lib(), []
        net.prev_causal_outputs = None
        keep, net.keep_window = net.keep_window, False
        try:
            net.forward_one_step(torch.as_tensor(window.reshape(1, -1)).cuda(), apply_softmax=True, **prefill)
        finally:
            net.keep_window = keep
        self.tok = torch.as_tensor(window.reshape(1, -1)).cuda().to(torch.int32).contiguous()
        self.causal = [t.contiguous().clone() for t in net._last_causal_outputs]
        self.layers = [t.contiguous().clone() for t in net._last_layer_inputs]

    def handle(self, **desc):
        d, self._held = self.net._desc(**desc)
        h = C.c_void_p()
        _lib.check(self.lib.wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        _lib.check(self.lib.wn_decoder_load_state(h, _lib.ptr(self.tok), self.tok.shape[1], _lib.ptr_array(self.causal),
                                                  _lib.ptr_array(self.layers), None), "wn_decoder_load_state")
        torch.cuda.synchronize()
        self.hs.append(h)
        return h

    def close(self):
        for h in self.hs:
            self.lib.wn_decoder_destroy(h)


def _launch(hs, firsts, u, out, probs, done, n, same):
    """wn_decoder_run_batch over utterances ``hs``; utterance i's buffers are entered behind its ``done[i]`` steps."""
    k = len(hs)
    return _lib.lib().wn_decoder_run_batch(
        _arr(C.c_void_p, [h.value for h in hs]), k, _arr(C.c_int32, firsts), _arr(C.c_void_p, [u[i][done[i]:].data_ptr() for i in range(k)]),
        n, _arr(C.c_void_p, [out[i][done[i]:].data_ptr() for i in range(k)]),
        None if probs is None else _arr(C.c_void_p, [probs[i][done[i]:].data_ptr() for i in range(k)]), same, None)


@pytest.mark.parametrize("U", [2, 4])
@pytest.mark.parametrize("name", ["A", "B"])
def test_c_abi_tiled_launches_equal_wn_decoder_run_on_twin_handles(name, U):
    """Five utterances with a step limit each (20, 5, 14, none, 9), the third with sampling controls: launches of 12, 5 and 3 steps
    flagged ``same_weights = U`` -- finished utterances left out, so the tiles change from launch to launch and the last tile is
    short -- against ONE ``wn_decoder_run`` of the utterance's count on a twin: tokens and the full (n, Q) traces.  Every buffer is
    exactly the utterance's own count long plus guard elements, which must be untouched."""
    p, w, net = model(name)[:3]
    lib = _lib.lib()
    Q = p["quantization_steps"]
    S = _Seeded(net, np.random.RandomState(5).randint(0, Q, (net.input_width,)).astype(np.int32))
    limits, n, G = [20, 5, 14, 0, 9], 20, 3
    counts = [l or n for l in limits]
    N = len(limits)
    batch = [S.handle(step_limit=l) for l in limits]
    twins = [S.handle() for _ in limits]
    for h in (batch[2], twins[2]):
        _lib.check(lib.wn_decoder_set_sampling(h, 0.8, 40 if Q > 64 else 9, 0.9), "wn_decoder_set_sampling")
    firsts = [3, Q - 1, Q // 2, 0, 7]
    rs = np.random.RandomState(6)
    u = [torch.as_tensor(rs.random_sample(c)).cuda() for c in counts]              # exactly the utterance's own count
    want = [torch.zeros((c,), device="cuda", dtype=torch.int32) for c in counts]
    want_p = [torch.zeros((c, Q), device="cuda", dtype=torch.float32) for c in counts]
    for i in range(N):
        _lib.check(lib.wn_decoder_run(twins[i], firsts[i], u[i].data_ptr(), counts[i], want[i].data_ptr(), want_p[i].data_ptr(), None),
                   "wn_decoder_run")
    got = [torch.full((c + G,), -7, device="cuda", dtype=torch.int32) for c in counts]
    got_p = [torch.full((c + G, Q), -7.0, device="cuda", dtype=torch.float32) for c in counts]
    done = [0] * N
    for steps in (12, 5, 3):
        sel = [i for i in range(N) if done[i] < counts[i]]
        tok = [firsts[i] if not done[i] else int(got[i][done[i] - 1]) for i in sel]
        rc = _launch([batch[i] for i in sel], tok, [u[i] for i in sel], [got[i] for i in sel], [got_p[i] for i in sel],
                     [done[i] for i in sel], steps, U)
        assert rc == 0, lib.wn_last_error().decode()
        assert lib.wn_decoder_status(batch[sel[0]], None) == _lib.WN_OK
        for i in sel:
            done[i] = min(counts[i], done[i] + steps)
    assert done == counts
    for i in range(N):
        np.testing.assert_array_equal(to_np(got[i])[:counts[i]], to_np(want[i]), err_msg="tokens of utterance %d" % i)
        np.testing.assert_array_equal(_bits(got_p[i])[:counts[i]], _bits(want_p[i]), err_msg="trace of utterance %d" % i)
        assert (to_np(got[i])[counts[i]:] == -7).all() and (to_np(got_p[i])[counts[i]:] == -7.0).all(), "guards of utterance %d" % i
    assert len({tuple(to_np(t)[:5].tolist()) for t in got}) == N
    S.close()


# ---- 4. the weights really are shared -------------------------------------------------------------------------------------------
def test_a_tile_reads_handle_zeros_weights_for_every_utterance():
    """Handle 0 is packed from the model; then the model's head tensor is overwritten in place -- same pointers, other values --
    and handle 1 is packed from it.  Flagged ``same_weights = 2``, utterance 1 emits what a twin of handle 0 emits (it reads handle
    0's copy); with ``same_weights = 0`` it emits what its own copy gives.  Without tiles the library reads own copies whatever the
    claim, and the first equality fails."""
    p, w, net = build(A, cls=FasterWaveNet)
    lib = _lib.lib()
    Q, n = 256, 16
    S = _Seeded(net, np.random.RandomState(15).randint(0, Q, (net.input_width,)).astype(np.int32))
    old = [S.handle() for _ in range(3)]                # handle 0 of the tiled launch, handle 0 of the plain one, the twin
    with torch.no_grad():
        W = net.softmax_conv_layers[-1].W
        W.copy_(torch.roll(W, 5, 0).clone())            # the logits move five tokens up
    new = [S.handle() for _ in range(3)]
    u = torch.as_tensor(np.random.RandomState(16).random_sample((2, n))).cuda()
    firsts = [9, 200]

    def run_twin(h):
        out = torch.zeros((n,), device="cuda", dtype=torch.int32)
        _lib.check(lib.wn_decoder_run(h, firsts[1], u[1].data_ptr(), n, out.data_ptr(), None, None), "wn_decoder_run")
        return to_np(out)
    with_old, with_new = run_twin(old[2]), run_twin(new[2])
    assert (with_old != with_new).any()
    for same, h0, h1, want in ((2, old[0], new[0], with_old), (0, old[1], new[1], with_new)):
        out = torch.zeros((2, n), device="cuda", dtype=torch.int32)
        assert _launch([h0, h1], firsts, list(u), list(out), None, [0, 0], n, same) == 0, lib.wn_last_error().decode()
        assert lib.wn_decoder_status(h0, None) == _lib.WN_OK
        np.testing.assert_array_equal(to_np(out)[1], want, err_msg="same_weights = %d" % same)
    S.close()


# ---- 5. per-utterance state in one tile -----------------------------------------------------------------------------------------
def test_sampling_controls_chosen_and_forced_per_slot():
    p, w, net, u = model("A")[:4]
    N, n = 5, LONGEST
    temps, ks, ps = [1.0, 0.8, 1.3, 1.0, 0.7], [0, 40, 3, 0, 0], [1.0, 0.9, 0.5, 0.6, 1.0]
    with launches(net) as l:
        got, ch = net.generate_batch(n, u[:N], temperature=temps, top_k=ks, top_p=ps, return_chosen=True, tile=4)
    assert l.same == [4]
    for i in range(N):
        want, want_ch = net.generate(n, u[i], temperature=temps[i], top_k=ks[i], top_p=ps[i], return_chosen=True)
        np.testing.assert_array_equal(to_np(got[i]), to_np(want), err_msg="utterance %d" % i)
        np.testing.assert_array_equal(_bits(ch[i]), _bits(want_ch), err_msg="chosen of utterance %d" % i)
    assert (to_np(got[1]) != model("A")[5][1]).any()                               # the controls changed something
    # given samples: an utterance given throughout, one drawn throughout (None), mixed ones, one with a filter on
    rs = np.random.RandomState(31)
    forced = [rs.randint(0, 256, (n,)).astype(np.int32), None]
    for _ in range(3):
        f = rs.randint(0, 256, (n,)).astype(np.int32)
        f[rs.random_sample(n) < 0.5] = -1
        forced.append(f)
    with launches(net) as l:
        got, ch = net.generate_batch(n, u[:N], top_k=[0, 0, 0, 30, 0], forced=forced, return_chosen=True, tile=4)
    assert l.same == [4]
    for i in range(N):
        want, want_ch = net.generate(n, u[i], top_k=[0, 0, 0, 30, 0][i], forced=forced[i], return_chosen=True)
        np.testing.assert_array_equal(to_np(got[i]), to_np(want), err_msg="utterance %d" % i)
        np.testing.assert_array_equal(_bits(ch[i]), _bits(want_ch), err_msg="chosen of utterance %d" % i)
    np.testing.assert_array_equal(to_np(got[0]), forced[0])


def test_a_class_per_slot():
    """A globally conditioned model: the static gate biases are an utterance's own, everything else is handle 0's."""
    p = R.make_params(**cond_ref.TINY)
    E, V = cond_ref.init_condition(p, seed=99)
    net = FasterWaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    net.load_state_dict(cond_ref.state_dict(R.init_weights(p, 1234), E, V))
    net.to_gpu()
    N, n = 6, 16
    classes = [0, 2, 1, 1, 2, 0]
    u = np.random.RandomState(33).random_sample((N, n))
    with launches(net) as l:
        got = to_np(net.generate_batch(n, u, condition=classes, tile=4))
    assert l.same == [4]
    for i in range(N):
        np.testing.assert_array_equal(got[i], to_np(net.generate(n, u[i], condition=classes[i])), err_msg="utterance %d" % i)
    assert (got[0] != to_np(net.generate(n, u[0], condition=1))).any()             # the class matters


def _local_model(interp, hop):
    p = R.make_params(**LR.TINY)
    V, _ = LR.init_local(p)
    net = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=hop, local_interp=interp)
    net.load_state_dict(LR.state_dict(R.init_weights(p, 1234), V, None, None))
    net.to_gpu()
    return net


@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_a_table_and_a_phase_per_slot(interp):
    hop, n, N = 4, 18, 5
    net = _local_model(interp, hop)
    W = net.input_width
    rs = np.random.RandomState(35)
    phases = [0, 3, 1, 2, 3]
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, hop, ph, interp) + i)).astype(np.float32) for i, ph in enumerate(phases)]
    prompts = rs.randint(0, 256, (N, W)).astype(np.int32)
    u = rs.random_sample((N, n))
    with launches(net) as l:
        got = to_np(net.generate_batch(n, u, initial_tokens=prompts, local=hs, local_phase=phases, tile=4))
    assert l.same == [4]
    for i in range(N):
        want = to_np(net.generate(n, u[i], initial_tokens=prompts[i], local=hs[i], local_phase=phases[i]))
        np.testing.assert_array_equal(got[i], want, err_msg="utterance %d" % i)
    assert len({tuple(r) for r in got.tolist()}) == N


# ---- 6. streams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_a_tiled_stream_equals_one_generate_batch_call(interp):
    """Five utterances, tile 4, a ring each: rows pushed and samples pulled in uneven pieces; tokens and ``chosen`` are those of
    one (untiled) ``generate_batch`` call over the whole tables."""
    hop, n, N, lin = 4, 30, 5, interp == "linear"
    net = _local_model(interp, hop)
    W = net.input_width
    rs = np.random.RandomState(37)
    phases = [0, 3, 1, 2, 0]
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, hop, ph, interp) + 2)).astype(np.float32) for ph in phases]
    cws = [frames_needed(W, hop, ph, interp) for ph in phases]
    rows = [net.local_biases(hs[i], phases[i]) for i in range(N)]
    for i in range(N):                     # the premise: the window's rows do not depend on the columns projected with them
        head = net.local_biases(hs[i][:, :cws[i]], phases[i])
        assert torch.equal(head, rows[i][:head.shape[0]])
    prompts = rs.randint(0, 256, (N, W)).astype(np.int32)
    u = rs.random_sample((N, n))
    kw = dict(temperature=[1.0, 1.0, 0.8, 1.0, 1.0], top_k=[0, 0, 20, 0, 0])
    want, want_ch = net.generate_batch(n, u, initial_tokens=prompts, local=hs, local_phase=phases, return_chosen=True, **kw)
    Rr = stream_frames(hop, lin, 0, pull=7).min_ring + 2
    toks, chs, done, at = [], [], 0, list(cws)
    with launches(net) as l:
        with net.open_stream(utterances=N, initial_tokens=prompts, local=[hs[i][:, :cws[i]] for i in range(N)], local_phase=phases,
                             return_chosen=True, ring_frames=Rr, max_pull=7, tile=4, **kw) as st:
            assert st.tile == 4
            for m in [3, 1, 7, 4, 2, 5, 6, 2]:
                m = min(m, n - done)
                if not m:
                    break
                k = [max(0, min(int(rows[i].shape[0]) - at[i], st.book.frames(i).current + Rr - (i % 2) - st.book.fed[i])) for i in range(N)]
                st.push_rows([rows[i][at[i]:at[i] + k[i]] for i in range(N)])
                at = [a + b for a, b in zip(at, k)]
                t, c = st.pull(m, u[:, done:done + m])
                toks.append(t)
                chs.append(c)
                done += m
    assert done == n and l.same and set(l.same) == {4}
    assert torch.equal(torch.cat(toks, dim=1), want)
    np.testing.assert_array_equal(_bits(torch.cat(chs, dim=1)), _bits(want_ch))


# ---- 7. refusals touch nothing --------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing():
    lib = _lib.lib()
    net = model("A")[2]
    S = _Seeded(net, np.full((net.input_width,), 127, np.int32))
    hA = [S.handle(), S.handle()]
    u = torch.zeros((2, 8), device="cuda", dtype=torch.float64) + 0.5
    out = torch.zeros((2, 8), device="cuda", dtype=torch.int32)

    def call(handles, same):
        rc = _launch(handles, [5] * len(handles), list(u), list(out), None, [0, 0], 8, same)
        return rc, lib.wn_last_error().decode()
    for same in (3, 32, -1, 5, 17):
        rc, msg = call(hA, same)
        assert rc == _lib.WN_EARG and "same_weights = %d" % same in msg, (same, rc, msg)
    # a tile that does not fit: maxc = 512, two thin layers
    wide = dict(quantization_steps=256, causal_conv_channels=[8], residual_conv_channels=[8] * 2, residual_num_blocks=1,
                softmax_conv_channels=[512, 256])
    netW = build(wide, cls=FasterWaveNet)[2]
    assert tile_fit(netW.params) == 8
    SW = _Seeded(netW, np.full((netW.input_width,), 127, np.int32))
    hW = [SW.handle(), SW.handle()]
    rc, msg = call(hW, 16)
    assert rc == _lib.WN_ESHAPE and "largest tile that fits this model is 8" in msg, (rc, msg)
    with pytest.raises(ValueError, match="tile_fit. is 8"):
        netW.generate_batch(4, np.zeros((3, 4)) + 0.5, tile=16)
    # handles of another layout: one created with gate biases, one without
    p = R.make_params(**cond_ref.TINY)
    E, V = cond_ref.init_condition(p, seed=99)
    netG = FasterWaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    netG.load_state_dict(cond_ref.state_dict(R.init_weights(p, 1234), E, V))
    netG.to_gpu()
    SG = _Seeded(netG, np.full((netG.input_width,), 127, np.int32), condition=[1])
    hG = [SG.handle(cond=netG.condition_biases(1)), SG.handle(cond=netG.condition_biases(2)), SG.handle()]
    rc, msg = call([hG[0], hG[2]], 2)
    assert rc == _lib.WN_EARG and "utterance 1" in msg and "layout" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                        # nothing ran
    for h in hA + hW + hG:
        assert lib.wn_decoder_status(h, None) == _lib.WN_OK
    # ... while two classes of one layout share a tile, which same_weights = 1 refuses
    rc, msg = call(hG[:2], 1)
    assert rc == _lib.WN_EARG and "utterance 1" in msg, (rc, msg)
    rc, msg = call(hG[:2], 2)
    assert rc == 0, msg
    assert lib.wn_decoder_status(hG[0], None) == _lib.WN_OK
    for s in (S, SW, SG):
        s.close()


def test_nine_workgroup_handles_take_a_tile_size_as_same_weights_one():
    p, w, net = build(CFG2, cls=FasterWaveNet)
    lib = _lib.lib()
    n = 12
    S = _Seeded(net, np.random.RandomState(45).randint(0, 256, (net.input_width,)).astype(np.int32))
    hs = [S.handle() for _ in range(4)]
    u = torch.as_tensor(np.random.RandomState(46).random_sample((2, n))).cuda()
    firsts = [3, 250]
    want = torch.zeros((2, n), device="cuda", dtype=torch.int32)
    for i in range(2):
        _lib.check(lib.wn_decoder_run(hs[2 + i], firsts[i], u[i].data_ptr(), n, want[i].data_ptr(), None, None), "wn_decoder_run")
        assert lib.wn_decoder_status(hs[2 + i], None) == _lib.WN_OK
    got = torch.zeros((2, n), device="cuda", dtype=torch.int32)
    rc = _launch(hs[:2], firsts, list(u), list(got), None, [0, 0], n, 8)
    assert rc == 0, lib.wn_last_error().decode()
    for h in hs[:2]:
        assert lib.wn_decoder_status(h, None) == _lib.WN_OK
    np.testing.assert_array_equal(to_np(got), to_np(want))
    S.close()
