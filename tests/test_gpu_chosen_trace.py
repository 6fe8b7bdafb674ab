"""GPU: decoders report the probability of each token they emit (WN_DECODER_TRACE_CHOSEN, ``return_chosen``, ``--best-of``).

Every comparison is exact: ``chosen[i]`` is the float a full-row run holds at ``probs[i, tokens[i]]``, and the flag changes no
token.  The models are the smallest that reach each kernel: tests/cond_ref.py's TINY on the any-shape decoder, config 4's
channel shape at 2 x 3 layers on the specialised one -- on nine workgroups and with WN_DECODER_ONE_WORKGROUP.  Where a row of a
nine-workgroup BATCHED launch is held to the utterance's own single run, the model also comes at 2 x 5 layers, the depth at which
the rest of the suite compares the two.  (At six layers the specialised kernels' tokens used to differ from run to run -- DESIGN.md,
"The probability of each emitted token", "A finding on the way" --: the tests of one utterance here, which hold two runs from one
state to each other at 2 x 3 layers, fail on a library without that fix.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from gpu_util import CFG2, build, dev
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib, sampling
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.faster_wavenet import silence_window
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

Q = 256
N = 41                            # samples per utterance: the prefill's draw + 40 decode steps
SPEC = dict(CFG2, residual_conv_channels=[32] * 3, residual_num_blocks=2)       # config 4's channels, 2 x 3 layers
SPEC10 = dict(CFG2, residual_conv_channels=[32] * 5, residual_num_blocks=2)     # ... 2 x 5 layers
CHOSEN, GATE, ONE = _lib.WN_DECODER_TRACE_CHOSEN, _lib.WN_DECODER_GATE_ROWS, _lib.WN_DECODER_ONE_WORKGROUP
SENT = 0x7FC0BEEF                 # a NaN bit pattern no kernel computes: what an unwritten float of a trace holds
CONTROLS = {"off": {}, "on": dict(temperature=0.7, top_k=5, top_p=0.9)}
_NETS = {}


def _net(form):
    """"any" | "nine" | "one" | "nine10": built once per module."""
    if form not in _NETS:
        over = {"any": cond_ref.TINY, "nine": SPEC, "one": SPEC, "nine10": SPEC10}[form]
        net = build(over, cls=FasterWaveNet)[2]
        if form == "one":
            net.exec_flags = _lib.default_exec_flags() | ONE
        assert net._nine_workgroup_shape(_lib.default_exec_flags()) == (form != "any")
        _NETS[form] = net
    return _NETS[form]


def _gather(probs, tokens):
    return probs.gather(1, tokens.long()[:, None])[:, 0]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_floats(a, b):
    """Bit-identical float32 tensors (and no NaN among them: a sentinel that leaked would be one)."""
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(_bits(a), _bits(b)) and \
        not bool(torch.isnan(a).any())


# ---- 1. the Python face, one utterance ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctl", ["off", "on"])
@pytest.mark.parametrize("form", ["any", "nine", "one"])
def test_chosen_is_the_drawn_entry_of_the_full_trace_and_the_tokens_do_not_change(form, ctl):
    net, kw = _net(form), CONTROLS[ctl]
    rs = np.random.RandomState(31)
    prompt, u = rs.randint(0, Q, (net.input_width,)).astype(np.int32), rs.random_sample(N)
    plain = net.generate(N, u, initial_tokens=prompt, **kw)
    assert not net._dec.chosen
    tokens, chosen = net.generate(N, u, initial_tokens=prompt, return_chosen=True, **kw)
    assert net._dec.chosen                                                   # the handle was created anew, in the other form
    t_full, probs = net.generate(N, u, initial_tokens=prompt, return_probs=True, **kw)
    assert not net._dec.chosen
    assert torch.equal(tokens, plain) and torch.equal(t_full, plain)
    assert chosen.shape == (N,) and chosen.is_cuda
    assert _same_floats(chosen, _gather(probs, t_full))                      # element 0, the prefill's row, included
    assert float(chosen.min()) > 0.0 and float(chosen.max()) <= 1.0 and len(set(plain.cpu().tolist())) > 3
    # both at once: the full-row handle, the same floats
    t_b, p_b, c_b = net.generate(N, u, initial_tokens=prompt, return_probs=True, return_chosen=True, **kw)
    assert not net._dec.chosen and torch.equal(t_b, plain) and torch.equal(_bits(p_b), _bits(probs)) and _same_floats(c_b, chosen)
    nll = sampling.chosen_nll(chosen)
    assert nll == float(np.mean(-np.log(chosen.cpu().numpy().astype(np.float64)))) and 0.0 < nll < 2.0 * np.log(Q)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
class _Abi(object):
    """Decoder handles of one unconditioned model, every one seeded from ONE prefill over one random prompt."""

    def __init__(self, form, seed=5):
        self.net = _net(form)
        rs = np.random.RandomState(seed)
        self.tok = dev(rs.randint(0, Q, (1, self.net.input_width)).astype(np.int32))
        self.u = [dev(rs.random_sample(64)) for _ in range(3)]
        with torch.no_grad():
            self.net.forward_one_step(self.tok)
        self.causal = [t.contiguous() for t in self.net._last_causal_outputs]
        self.layers = list(self.net._last_layer_inputs)
        self.handles = []

    def desc(self, chosen, step_limit=0):
        return self.net._desc(None, None, step_limit, chosen)

    def create(self, chosen, step_limit=0, controls=None):
        d, keep = self.desc(chosen, step_limit)
        assert bool(d.flags & CHOSEN) == bool(chosen)
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        check(_lib.lib().wn_decoder_load_state(h, ptr(self.tok), int(self.tok.shape[1]), ptr_array(self.causal),
                                               ptr_array(self.layers), None), "wn_decoder_load_state")
        if controls:
            check(_lib.lib().wn_decoder_set_sampling(h, *controls), "wn_decoder_set_sampling")
        return h

    def run(self, h, n, trace=None, u=0, first=7):
        out = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        rc = _lib.lib().wn_decoder_run(h, first, ptr(self.u[u]), n, ptr(out), None if trace is None else trace.data_ptr(), None)
        torch.cuda.synchronize()
        return rc, out

    def run_batch(self, hs, n, traces=None, firsts=None):
        k = len(hs)
        outs = [torch.full((n,), -1, device="cuda", dtype=torch.int32) for _ in range(k)]
        rc = _lib.lib().wn_decoder_run_batch((C.c_void_p * k)(*[h.value for h in hs]), k, (C.c_int32 * k)(*(firsts or [7] * k)),
                                             ptr_array([self.u[i] for i in range(k)]), n, ptr_array(outs),
                                             None if traces is None else ptr_array(traces), 1, None)
        msg = _lib.lib().wn_last_error().decode()
        torch.cuda.synchronize()
        return rc, outs, msg

    def close(self):
        for h in self.handles:
            _lib.lib().wn_decoder_destroy(h)


@pytest.fixture
def abi(request):
    a = _Abi(request.param)
    yield a
    a.close()


# ---- 2. the trace is n floats ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abi", ["any", "nine", "one"], indirect=True)
def test_the_chosen_trace_is_exactly_n_floats(abi):
    """The trace sits inside a tensor of sentinels large enough for rows of Q, a guard in front and everything behind its n
    floats must come back untouched: a kernel still writing rows of Q would trip this."""
    n, G = 40, 64
    big = torch.full((G + n * Q + G,), SENT, device="cuda", dtype=torch.int32)
    trace = big.view(torch.float32)[G:]
    rc, tokens = abi.run(abi.create(True, controls=(0.7, 5, 0.9)), n, trace)
    assert rc == 0, _lib.lib().wn_last_error()
    got = big.cpu().numpy()
    assert (got[:G] == SENT).all() and (got[G + n:] == SENT).all() and (got[G:G + n] != SENT).all()
    full = torch.full((n, Q), float("nan"), device="cuda")
    rc, t_full = abi.run(abi.create(False, controls=(0.7, 5, 0.9)), n, full)
    assert rc == 0 and torch.equal(tokens, t_full)
    assert _same_floats(trace[:n], _gather(full, t_full))


# ---- 3. batches --------------------------------------------------------------------------------------------------------------------
def _batch_args(net, lengths, seed):
    """A prompt, uniforms and controls of its own per utterance."""
    rs = np.random.RandomState(seed)
    k = len(lengths)
    prompts = rs.randint(0, Q, (k, net.input_width)).astype(np.int32)
    u = [rs.random_sample(n) for n in lengths]
    kw = dict(temperature=[1.0, 0.7, 0.9][:k], top_k=[0, 5, 0][:k], top_p=[1.0, 0.9, 0.8][:k])
    return prompts, u, kw


@pytest.mark.parametrize("form,lengths,launched", [("nine", [7, 2, 19], False), ("any", [1, 9, 4], True),
                                                   ("nine10", [8, 3, 20], True)], ids=["nine", "any", "nine-2x5-launched"])
def test_a_batched_row_is_its_own_generate_call(form, lengths, launched):
    """(On the nine-workgroup form an utterance of two samples sends the call through the loop over ``generate``; the third
    case has the step counts 7, 2, 19 and is one launch.)"""
    net = _net(form)
    prompts, u, kw = _batch_args(net, lengths, 41)
    singles = [net.generate(lengths[i], u[i], initial_tokens=prompts[i], return_chosen=True, **{k: v[i] for k, v in kw.items()})
               for i in range(len(lengths))]
    plain = net.generate_batch(lengths, u, initial_tokens=prompts, **kw)
    calls = []
    inner = net.generate
    net.generate = lambda *a, **k: calls.append(1) or inner(*a, **k)
    try:
        rows, chosen = net.generate_batch(lengths, u, initial_tokens=prompts, return_chosen=True, **kw)
    finally:
        del net.generate
    assert (not calls) == launched
    if launched:
        assert all(h.chosen for h in net._handles[:len(lengths)])            # created anew in the other form, never mixed
    assert isinstance(rows, list) and isinstance(chosen, list) and len(rows) == len(chosen) == len(lengths)
    for i, n in enumerate(lengths):
        assert rows[i].shape == (n,) and chosen[i].shape == (n,) and chosen[i].is_cuda
        assert torch.equal(rows[i], plain[i]) and torch.equal(rows[i], singles[i][0]), i
        assert _same_floats(chosen[i], singles[i][1]), i
    assert len({tuple(t.cpu().tolist()[:2]) for t, _ in singles if t.numel() > 1}) > 1      # the utterances are distinct
    if not launched:
        return
    # one length for all: (N, n) tensors
    n = 6
    u6 = np.stack([np.resize(r, n) for r in u])
    t6, c6 = net.generate_batch(n, u6, initial_tokens=prompts, return_chosen=True, **kw)
    assert t6.shape == c6.shape == (len(lengths), n) and c6.dtype == torch.float32
    for i in range(len(lengths)):
        t1, c1 = net.generate(n, u6[i], initial_tokens=prompts[i], return_chosen=True, **{k: v[i] for k, v in kw.items()})
        assert torch.equal(t6[i], t1) and _same_floats(c6[i], c1), i


@pytest.mark.parametrize("abi,steps,exact", [("nine", [7, 2, 19], False), ("any", [1, 9, 4], True), ("nine10", [7, 2, 19], True)],
                         indirect=["abi"], ids=["nine", "any", "nine-2x5"])
def test_a_batched_trace_is_n_u_floats_and_the_rest_keeps_the_sentinel(abi, steps, exact):
    """``exact``: the first n_u floats and tokens are also those of the utterance's own wn_decoder_run on a fresh handle."""
    n = max(steps)
    ctl = [None, (0.7, 5, 0.9), (0.9, 0, 0.8)]
    hs = [abi.create(True, step_limit=s, controls=c) for s, c in zip(steps, ctl)]
    traces = [torch.full((n,), SENT, device="cuda", dtype=torch.int32) for _ in steps]
    rc, outs, msg = abi.run_batch(hs, n, traces)
    assert rc == 0, msg
    for i, s in enumerate(steps):
        got, tok = traces[i].cpu().numpy(), outs[i].cpu().numpy()
        assert (got[s:] == SENT).all() and (got[:s] != SENT).all() and (tok[s:] == -1).all() and (tok[:s] >= 0).all(), i
        p = traces[i].view(torch.float32)[:s]
        assert float(p.min()) > 0.0 and float(p.max()) <= 1.0
        if exact:
            mine = torch.full((s,), SENT, device="cuda", dtype=torch.int32)
            rc, t1 = abi.run(abi.create(True, controls=ctl[i]), s, mine.view(torch.float32), u=i)
            assert rc == 0 and torch.equal(t1, outs[i][:s]) and torch.equal(mine, traces[i][:s]), i


# ---- 4. conditioned: GATE_ROWS | TRACE_CHOSEN ------------------------------------------------------------------------------------
def test_a_conditioned_model_of_the_specialised_shape():
    """Globally plus locally conditioned, linear interpolation, 2 x 5 layers (its batched rows are held to single runs)."""
    hop = 5
    p = R.make_params(**SPEC10)
    w = R.init_weights(p, 1234)
    V, _ = LR.init_local(p)
    E, Vg = cond_ref.init_condition(p)
    net = FasterWaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS,
                        local_channels=LR.FEATS, local_hop=hop, local_interp="linear")
    net.load_state_dict(LR.state_dict(w, V, E, Vg))
    net.to_gpu()
    assert net._nine_workgroup_shape(_lib.default_exec_flags())
    assert net._desc(None, None, 0, True)[0].flags & (GATE | CHOSEN) == GATE | CHOSEN
    rs = np.random.RandomState(51)
    W = net.input_width
    prompts = rs.randint(0, Q, (2, W)).astype(np.int32)
    u = rs.random_sample((2, N))
    phases, classes = [3, 1], [2, 0]
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + N - 1, hop, ph, "linear"))).astype(np.float32) for ph in phases]
    singles = []
    for i in range(2):
        kw = dict(initial_tokens=prompts[i], condition=classes[i], local=hs[i], local_phase=phases[i])
        plain = net.generate(N, u[i], **kw)
        tokens, chosen = net.generate(N, u[i], return_chosen=True, **kw)
        t_full, probs = net.generate(N, u[i], return_probs=True, **kw)
        assert torch.equal(tokens, plain) and torch.equal(t_full, plain) and _same_floats(chosen, _gather(probs, t_full)), i
        singles.append((tokens, chosen))
    assert not torch.equal(singles[0][0], singles[1][0])
    kw = dict(initial_tokens=prompts, condition=classes, local=hs, local_phase=phases)
    plain = net.generate_batch(N, u, **kw)
    tokens, chosen = net.generate_batch(N, u, return_chosen=True, **kw)
    assert torch.equal(tokens, plain) and tokens.shape == chosen.shape == (2, N)
    assert all(h.chosen for h in net._handles[:2])
    for i in range(2):                               # a class and a table per utterance
        assert torch.equal(tokens[i], singles[i][0]) and _same_floats(chosen[i], singles[i][1]), i


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abi", ["any", "nine"], indirect=True)
def test_a_handles_form_is_fixed_and_a_launch_takes_one_form(abi):
    lib = _lib.lib()
    n = 6
    rc, fresh = abi.run(abi.create(True), n)
    assert rc == 0
    # wn_decoder_update_weights with the bit flipped, both ways
    flagged, plain = abi.create(True), abi.create(False)
    for h, other in ((flagged, False), (plain, True)):
        d, keep = abi.desc(other)
        assert lib.wn_decoder_update_weights(h, C.byref(d), None) == _lib.WN_EARG
        msg = lib.wn_last_error().decode()
        assert "WN_DECODER_TRACE_CHOSEN" in msg and "fixed at create" in msg, msg
    for h in (flagged, plain):                       # the handles are as they were: the flag changes no token either
        rc, t = abi.run(h, n)
        assert rc == 0 and torch.equal(t, fresh)
    # wn_decoder_run_batch over one flagged and one unflagged handle
    a, b, c = abi.create(True), abi.create(False), abi.create(True)
    traces = [torch.full((n,), SENT, device="cuda", dtype=torch.int32) for _ in range(2)]
    rc, outs, msg = abi.run_batch([a, b], n, traces)
    assert rc == _lib.WN_EARG and "utterance 1" in msg and "WN_DECODER_TRACE_CHOSEN" in msg, (rc, msg)
    assert all((t == SENT).all() for t in traces) and all((o == -1).all() for o in outs)
    rc, outs, msg = abi.run_batch([b, c], n)
    assert rc == _lib.WN_EARG and "utterance 1" in msg, (rc, msg)
    # ... and a valid launch of the two flagged ones emits what fresh handles emit
    mine = [abi.run(abi.create(True), n, u=i)[1] for i in range(2)]
    rc, outs, msg = abi.run_batch([a, c], n, traces)
    assert rc == 0, msg
    rc, t_b = abi.run(b, n)
    assert rc == 0 and torch.equal(t_b, fresh)
    assert torch.equal(outs[0], mine[0]) and torch.equal(outs[1], mine[1])
    assert all((t != SENT).all() for t in traces)


# ---- 6. the command line ----------------------------------------------------------------------------------------------------------
def test_best_of_3_of_2_utterances_with_a_report_end_to_end(tmp_path):
    from wavenet_amd.train_audio import generate as cli_generate
    net = _net("any")
    model, out, report = tmp_path / "model", tmp_path / "out", tmp_path / "report.json"
    model.mkdir()
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(cond_ref.TINY, sampling_rate=41)))
    files, tokens = cli_generate.main(["-m", str(model), "-o", str(out), "-s", "1", "--fast", "--seed", "2", "--utterances", "2",
                                       "--best-of", "3", "--report", str(report), "--temperature", "0.9"])
    n, K = 40, 3
    assert [os.path.basename(f) for f in files] == ["generated_000.wav", "generated_001.wav"] == sorted(os.listdir(str(out)))
    assert tokens.shape == (2, n)
    table = json.loads(report.read_text())
    U = np.random.RandomState(2).random_sample((2 * K, n))
    silence = silence_window(Q, net.input_width)
    total = 0.0
    for i, row in enumerate(table["files"]):
        assert row["file"] == "generated_%03d.wav" % i and row["samples"] == n and len(row["candidates"]) == K
        assert row["kept"] == sampling.pick_best(row["candidates"])
        assert row["nats_per_sample"] == row["candidates"][row["kept"]]
        assert row["bits_per_sample"] == row["nats_per_sample"] / np.log(2.0)
        for c in range(K):                           # every candidate is the direct generate() with its row of uniforms
            t, ch = net.generate(n, U[i * K + c], initial_tokens=silence, temperature=0.9, return_chosen=True)
            assert sampling.chosen_nll(ch) == row["candidates"][c], (i, c)
            if c == row["kept"]:
                assert np.array_equal(t.cpu().numpy(), tokens[i])
        total += row["nats_per_sample"] * n
    assert len(table["files"]) == 2 and len({tuple(r["candidates"]) for r in table["files"]}) == 2
    assert table["total"]["samples"] == 2 * n and table["total"]["nats_per_sample"] == total / (2 * n)
