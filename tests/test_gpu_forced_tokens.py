"""GPU: decoders keep given samples and draw the rest (WN_DECODER_FORCED_TOKENS, ``forced=``, ``generate --keep``).

Comparisons between two runs of the library are exact.  The models are the smallest that reach each kernel: tests/cond_ref.py's
TINY on the any-shape decoder, config 4's channel shape at 2 x 3 layers on the specialised one -- on nine workgroups and with
WN_DECODER_ONE_WORKGROUP -- and 2 x 5 layers wherever a row of a nine-workgroup BATCHED launch is held to its own single run."""
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
from oracle.data_ref import onehot_pixel_image
from wavenet_amd import FasterWaveNet, Params, _lib, data, sampling
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

Q = 256
N = 41                            # samples per utterance: the prefill's + 40 decode steps
SPEC = dict(CFG2, residual_conv_channels=[32] * 3, residual_num_blocks=2)       # config 4's channels, 2 x 3 layers
SPEC10 = dict(CFG2, residual_conv_channels=[32] * 5, residual_num_blocks=2)     # ... 2 x 5 layers
CHOSEN, GATE, ONE, FORCED = (_lib.WN_DECODER_TRACE_CHOSEN, _lib.WN_DECODER_GATE_ROWS, _lib.WN_DECODER_ONE_WORKGROUP,
                             _lib.WN_DECODER_FORCED_TOKENS)
SENT = 0x7FC0BEEF                 # as a float a NaN no kernel computes, as a token far outside [0, Q)
CONTROLS = {"off": {}, "on": dict(temperature=0.7, top_k=5, top_p=0.9)}
MASK = np.zeros((N,), bool)       # the given positions of the replay tests: 0, 5..17 and 30..33
MASK[[0] + list(range(5, 18)) + list(range(30, 34))] = True
_NETS = {}


def _model(form):
    """"any" | "nine" | "one" | "nine10" -> (oracle params, oracle weights, GPU model), built once per module."""
    if form not in _NETS:
        over = {"any": cond_ref.TINY, "nine": SPEC, "one": SPEC, "nine10": SPEC10}[form]
        p, w, net = build(over, cls=FasterWaveNet)
        if form == "one":
            net.exec_flags = _lib.default_exec_flags() | ONE
        assert net._nine_workgroup_shape(_lib.default_exec_flags()) == (form != "any")
        _NETS[form] = (p, w, net)
    return _NETS[form]


def _net(form):
    return _model(form)[2]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_floats(a, b):
    return a.dtype == b.dtype == torch.float32 and a.shape == b.shape and torch.equal(_bits(a), _bits(b)) and \
        not bool(torch.isnan(a).any())


# ---- 1. replay, exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctl", ["off", "on"])
@pytest.mark.parametrize("form", ["any", "nine", "one"])
def test_a_replay_with_some_samples_given_is_the_free_run(form, ctl):
    net, kw = _net(form), CONTROLS[ctl]
    rs = np.random.RandomState(61)
    prompt, u = rs.randint(0, Q, (net.input_width,)).astype(np.int32), rs.random_sample(N)
    tokens, chosen = net.generate(N, u, initial_tokens=prompt, return_chosen=True, **kw)
    assert not net._dec.forced
    t_full, probs = net.generate(N, u, initial_tokens=prompt, return_probs=True, **kw)
    assert torch.equal(tokens, t_full) and len(set(tokens.cpu().tolist())) > 3
    forced = np.where(MASK, tokens.cpu().numpy(), -1).astype(np.int32)
    nan_u = np.where(MASK, np.nan, u)                                # a given step never looks at its uniform
    for uu in (u, nan_u):
        t2, c2 = net.generate(N, uu, initial_tokens=prompt, return_chosen=True, forced=forced, **kw)
        assert net._dec.forced and net._dec.chosen                   # the handle was created anew, in the other form
        t3, p3 = net.generate(N, uu, initial_tokens=prompt, return_probs=True, forced=forced, **kw)
        assert net._dec.forced and not net._dec.chosen
        assert torch.equal(t2, tokens) and torch.equal(t3, tokens)
        assert _same_floats(c2, chosen) and _same_floats(p3, probs)
    plain = net.generate(N, u, initial_tokens=prompt, **kw)          # ... and back on an unflagged handle
    assert not net._dec.forced and torch.equal(plain, tokens)


# ---- 2. given tokens steer the run; against the oracle ---------------------------------------------------------------------------
def _oracle_run(p, w, u, forced):
    """``R.generate``'s fast loop from silence, a given position appending its token instead of the draw -> (tokens, rows, the
    smallest |normalised cumulative value - uniform| over the drawn steps)."""
    iw = R.input_width(p)
    buf = np.full((iw,), 127, dtype=np.int32)
    model = R.RefFasterWaveNet(p, w, "elu")
    rows, margin = [], np.inf
    for step in range(len(u)):
        prob = model._forward_one_step(onehot_pixel_image(buf[-iw:].reshape(1, -1), Q), apply_softmax=True)[0, :, 0, -1]
        rows.append(prob.copy())
        if forced[step] >= 0:
            tok = int(forced[step])
        else:
            tok = R.choice_from_uniform(prob, u[step])
            cdf = np.cumsum(prob.astype(np.float64))
            margin = min(margin, float(np.abs(cdf / cdf[-1] - u[step]).min()))
        buf = np.append(buf, [tok]).astype(np.int32)
    return buf[iw:], np.array(rows), margin


@pytest.mark.parametrize("form", ["any", "nine", "one"])
def test_given_tokens_steer_the_run_as_the_oracle_says(form):
    p, w, net = _model(form)
    forced = np.full((N,), -1, np.int32)
    forced[8:20] = np.random.RandomState(71).randint(0, Q, 12)
    # the seed is picked here, on the CPU: the first whose oracle run has no normalised cumulative value within 1e-6 of its
    # uniform at a drawn step.  Rows agree to 2e-5, so a tie that close is the only way a drawn index can differ.
    for seed in range(72, 80):
        u = np.random.RandomState(seed).random_sample(N)
        want, rows, margin = _oracle_run(p, w, u, forced)
        if margin > 1e-6:
            break
    assert margin > 1e-6
    tokens, probs = net.generate(N, u, return_probs=True, forced=forced)
    got = tokens.cpu().numpy()
    np.testing.assert_allclose(probs.cpu().numpy(), rows, atol=2e-5)
    assert np.array_equal(got[8:20], forced[8:20])
    assert np.array_equal(got, want)
    t_free, p_free = net.generate(N, u, return_probs=True)
    assert torch.equal(_bits(p_free[:9]), _bits(probs[:9]))                       # the same run up to the first given token's row
    assert not np.array_equal(t_free.cpu().numpy()[8:20], forced[8:20])
    assert float((p_free[20:] - probs[20:]).abs().max()) > 1e-3                   # the given tokens really entered the rings


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

    def desc(self, forced, chosen=False, step_limit=0):
        return self.net._desc(None, None, step_limit, chosen, forced=forced)

    def create(self, forced, chosen=False, step_limit=0, controls=None):
        d, keep = self.desc(forced, chosen, step_limit)
        assert bool(d.flags & FORCED) == bool(forced) and bool(d.flags & CHOSEN) == bool(chosen)
        h = C.c_void_p()
        check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        self.handles.append(h)
        check(_lib.lib().wn_decoder_load_state(h, ptr(self.tok), int(self.tok.shape[1]), ptr_array(self.causal),
                                               ptr_array(self.layers), None), "wn_decoder_load_state")
        if controls:
            check(_lib.lib().wn_decoder_set_sampling(h, *controls), "wn_decoder_set_sampling")
        return h

    def run(self, h, n, trace=None, u=0, first=7, out=None):
        out = torch.full((n,), -1, device="cuda", dtype=torch.int32) if out is None else out
        rc = _lib.lib().wn_decoder_run(h, first, ptr(self.u[u]), n, ptr(out), None if trace is None else trace.data_ptr(), None)
        torch.cuda.synchronize()
        return rc, out

    def run_batch(self, hs, n, traces=None, outs=None):
        k = len(hs)
        outs = [torch.full((n,), -1, device="cuda", dtype=torch.int32) for _ in range(k)] if outs is None else outs
        rc = _lib.lib().wn_decoder_run_batch((C.c_void_p * k)(*[h.value for h in hs]), k, (C.c_int32 * k)(*([7] * k)),
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


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abi", ["any", "nine", "one"], indirect=True)
def test_the_flag_alone_changes_nothing_and_the_compare_is_a_fence(abi):
    n, G, ctl = 40, 8, (0.7, 5, 0.9)
    for chosen in (False, True):
        shape = (n,) if chosen else (n, Q)
        tr0 = torch.full(shape, float("nan"), device="cuda")
        rc, plain = abi.run(abi.create(False, chosen, controls=ctl), n, tr0)
        assert rc == 0, _lib.lib().wn_last_error()
        # all -1, and entries that are no token (Q, -7, the sentinel): every step draws, tokens and trace are the unflagged handle's
        for fill in (None, {3: Q, 4: -7, 11: SENT, 12: -(2 ** 31), 13: 2 ** 31 - 1}):
            buf = torch.full((n + G,), SENT, device="cuda", dtype=torch.int32)
            buf[:n] = -1
            for i, v in (fill or {}).items():
                buf[i] = v
            tr1 = torch.full(shape, float("nan"), device="cuda")
            rc, out = abi.run(abi.create(True, chosen, controls=ctl), n, tr1, out=buf)
            assert rc == 0, _lib.lib().wn_last_error()
            assert torch.equal(out[:n], plain) and _same_floats(tr1, tr0)
            assert (out[n:] == SENT).all()                                    # behind n: neither read nor written
    # a given token is emitted, stays in the buffer, and a chosen trace holds its entry of the full row
    given = torch.full((n,), -1, device="cuda", dtype=torch.int32)
    given[10:14] = torch.tensor([0, 255, 9, 200], dtype=torch.int32)
    full = torch.full((n, Q), float("nan"), device="cuda")
    rc, t_full = abi.run(abi.create(True, False, controls=ctl), n, full, out=given.clone())
    one = torch.full((n,), float("nan"), device="cuda")
    rc2, t_one = abi.run(abi.create(True, True, controls=ctl), n, one, out=given.clone())
    assert rc == 0 and rc2 == 0 and torch.equal(t_full, t_one) and t_full[10:14].tolist() == [0, 255, 9, 200]
    assert torch.equal(t_full[:10], plain[:10]) and (t_full >= 0).all() and (t_full < Q).all()
    assert _same_floats(one, full.gather(1, t_full.long()[:, None])[:, 0])


@pytest.mark.parametrize("abi,steps,exact", [("nine", [7, 2, 19], False), ("any", [1, 9, 4], True), ("nine10", [7, 2, 19], True)],
                         indirect=["abi"], ids=["nine", "any", "nine-2x5"])
def test_a_ragged_batch_reads_and_writes_n_u_entries(abi, steps, exact):
    """Elements [n_u, n) hold a token: were they read it would be emitted (and change the tokens behind it), were they written
    it would be gone."""
    n = max(steps)
    hs = [abi.create(True, True, step_limit=s) for s in steps]
    outs = []
    for s in steps:
        o = torch.full((n,), 9, device="cuda", dtype=torch.int32)
        o[:s] = -1
        if s > 1:
            o[1] = 33                                                          # one given sample inside every utterance
        outs.append(o)
    traces = [torch.full((n,), SENT, device="cuda", dtype=torch.int32) for _ in steps]
    rc, outs, msg = abi.run_batch(hs, n, traces, outs)
    assert rc == 0, msg
    for i, s in enumerate(steps):
        tok = outs[i].cpu().numpy()
        assert (tok[s:] == 9).all() and (tok[:s] >= 0).all() and (tok[:s] < Q).all() and (s < 2 or tok[1] == 33), i
        assert (traces[i][s:] == SENT).all() and (traces[i][:s] != SENT).all(), i
        if exact:
            mine = torch.full((s,), -1, device="cuda", dtype=torch.int32)
            if s > 1:
                mine[1] = 33
            tr = torch.full((s,), SENT, device="cuda", dtype=torch.int32)
            rc, t1 = abi.run(abi.create(True, True), s, tr.view(torch.float32), u=i, out=mine)
            assert rc == 0 and torch.equal(t1, outs[i][:s]) and torch.equal(tr, traces[i][:s]), i


# ---- 4. batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,lengths,launched", [("nine", [7, 2, 19], False), ("any", [1, 9, 4], True),
                                                   ("nine10", [8, 3, 20], True)], ids=["nine", "any", "nine-2x5-launched"])
def test_a_batched_row_is_its_own_generate_call(form, lengths, launched):
    net = _net(form)
    rs = np.random.RandomState(81)
    k = len(lengths)
    prompts = rs.randint(0, Q, (k, net.input_width)).astype(np.int32)
    u = [rs.random_sample(n) for n in lengths]
    kw = dict(temperature=[1.0, 0.7, 0.9], top_k=[0, 5, 0], top_p=[1.0, 0.9, 0.8])
    # utterance 0: nothing given (None); utterance 1: everything given; utterance 2: partly, element 0 included
    part = np.full((lengths[2],), -1, np.int32)
    part[[0, 2]] = [17, 240]
    forced = [None, rs.randint(0, Q, lengths[1]).astype(np.int32), part]
    singles = [net.generate(lengths[i], u[i], initial_tokens=prompts[i], return_chosen=True, forced=forced[i],
                            **{key: v[i] for key, v in kw.items()}) for i in range(k)]
    calls = []
    inner = net.generate
    net.generate = lambda *a, **kws: calls.append(1) or inner(*a, **kws)
    try:
        rows, chosen = net.generate_batch(lengths, u, initial_tokens=prompts, return_chosen=True, forced=forced, **kw)
    finally:
        del net.generate
    assert (not calls) == launched
    if launched:
        assert all(h.forced and h.chosen for h in net._handles[:k])           # one form for the whole launch
    for i, n in enumerate(lengths):
        assert rows[i].shape == (n,) and torch.equal(rows[i], singles[i][0]), i
        assert _same_floats(chosen[i], singles[i][1]), i
    assert rows[1].cpu().tolist() == forced[1].tolist() and rows[2][0] == 17 and rows[2][2] == 240
    # tokens alone, and one array for all utterances
    plain = net.generate_batch(lengths, u, initial_tokens=prompts, forced=forced, **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, rows))
    one = np.full((max(lengths),), -1, np.int32)
    one[1] = 99
    got = net.generate_batch(lengths, u, initial_tokens=prompts, forced=one, **kw)
    for i, n in enumerate(lengths):
        t1 = net.generate(n, u[i], initial_tokens=prompts[i], forced=one[:n], **{key: v[i] for key, v in kw.items()})
        assert torch.equal(got[i], t1) and (n < 2 or got[i][1] == 99), i
    with pytest.raises(ValueError, match="utterance 1"):
        net.generate_batch(lengths, u, initial_tokens=prompts, forced=[None, np.full((lengths[1],), Q, np.int32), None])
    back = net.generate_batch(lengths, u, initial_tokens=prompts, **kw)        # forced=None: unflagged handles again
    if launched:
        assert not any(h.forced for h in net._handles[:k])
    assert torch.equal(back[0], rows[0])


# ---- 5. conditioned: GATE_ROWS | TRACE_CHOSEN | FORCED_TOKENS ---------------------------------------------------------------------
def test_a_conditioned_model_of_the_specialised_shape():
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
    want = GATE | CHOSEN | FORCED
    assert net._desc(None, None, 0, True, forced=True)[0].flags & want == want
    rs = np.random.RandomState(91)
    W = net.input_width
    prompts = rs.randint(0, Q, (2, W)).astype(np.int32)
    u = rs.random_sample((2, N))
    phases, classes = [3, 1], [2, 0]
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + N - 1, hop, ph, "linear"))).astype(np.float32) for ph in phases]
    free, forced = [], []
    for i in range(2):
        kw = dict(initial_tokens=prompts[i], condition=classes[i], local=hs[i], local_phase=phases[i])
        tokens, chosen = net.generate(N, u[i], return_chosen=True, **kw)
        f = np.where(MASK, tokens.cpu().numpy(), -1).astype(np.int32)
        t2, c2 = net.generate(N, np.where(MASK, np.nan, u[i]), return_chosen=True, forced=f, **kw)
        assert net._dec.forced and torch.equal(t2, tokens) and _same_floats(c2, chosen), i
        free.append((tokens, chosen))
        forced.append(f)
    assert not torch.equal(free[0][0], free[1][0])
    tokens, chosen = net.generate_batch(N, u, initial_tokens=prompts, condition=classes, local=hs, local_phase=phases,
                                        return_chosen=True, forced=forced)
    assert all(h.forced and h.chosen for h in net._handles[:2])
    for i in range(2):
        assert torch.equal(tokens[i], free[i][0]) and _same_floats(chosen[i], free[i][1]), i


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("abi", ["any", "nine"], indirect=True)
def test_a_handles_form_is_fixed_and_a_launch_takes_one_form(abi):
    lib = _lib.lib()
    n = 6
    rc, fresh = abi.run(abi.create(False), n)
    assert rc == 0
    flagged, plain = abi.create(True), abi.create(False)
    for h, other in ((flagged, False), (plain, True)):
        d, keep = abi.desc(other)
        assert lib.wn_decoder_update_weights(h, C.byref(d), None) == _lib.WN_EARG
        msg = lib.wn_last_error().decode()
        assert "WN_DECODER_FORCED_TOKENS" in msg and "fixed at create" in msg, msg
    for h in (flagged, plain):                       # the handles are as they were
        rc, t = abi.run(h, n)
        assert rc == 0 and torch.equal(t, fresh)
    a, b, c = abi.create(True), abi.create(False), abi.create(True)
    traces = [torch.full((n, Q), float("nan"), device="cuda") for _ in range(2)]
    for pair in ([a, b], [b, c]):
        outs = [torch.full((n,), 5, device="cuda", dtype=torch.int32) for _ in range(2)]
        rc, outs, msg = abi.run_batch(pair, n, traces, outs)
        assert rc == _lib.WN_EARG and "utterance 1" in msg and "WN_DECODER_FORCED_TOKENS" in msg, (rc, msg)
        assert all(bool(torch.isnan(t).all()) for t in traces) and all((o == 5).all() for o in outs)
    # ... and a valid launch of the two flagged ones emits what fresh handles emit
    mine = [abi.run(abi.create(True), n, u=i)[1] for i in range(2)]
    rc, outs, msg = abi.run_batch([a, c], n, traces)
    assert rc == 0, msg
    rc, t_b = abi.run(b, n)
    assert rc == 0 and torch.equal(t_b, fresh)
    assert torch.equal(outs[0], mine[0]) and torch.equal(outs[1], mine[1]) and torch.equal(mine[0], fresh)


# ---- 7. all given = the decoder's score ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["any", "nine", "one"])
def test_everything_given_is_the_decoders_likelihood_of_it(form):
    net = _net(form)
    rs = np.random.RandomState(101)
    prompt = rs.randint(0, Q, (net.input_width,)).astype(np.int32)
    audio = rs.randint(0, Q, (N,)).astype(np.int32)
    u = np.full((N,), np.nan)
    tokens, chosen = net.generate(N, u, initial_tokens=prompt, return_chosen=True, forced=audio, temperature=0.8, top_k=3)
    t2, probs = net.generate(N, u, initial_tokens=prompt, return_probs=True, forced=audio, temperature=0.8, top_k=3)
    assert tokens.cpu().tolist() == audio.tolist() == t2.cpu().tolist()
    rows = probs.cpu().numpy()
    assert sampling.chosen_nll(chosen) == float(np.mean(-np.log(rows[np.arange(N), audio].astype(np.float64))))
    # never truncated: top_k = 3 would have zeroed most of these entries
    assert float(chosen.min()) > 0.0 and int((rows > 0).sum(axis=1).min()) > 3


# ---- 8. the command line ----------------------------------------------------------------------------------------------------------
def test_keep_with_a_redraw_range_best_of_3_and_a_report_end_to_end(tmp_path):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import generate as cli_generate
    net = _net("any")
    W, sr, K = net.input_width, 100, 3
    model, out, report, wav = tmp_path / "model", tmp_path / "out", tmp_path / "report.json", str(tmp_path / "take.wav")
    model.mkdir()
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(cond_ref.TINY, sampling_rate=sr)))
    loud = np.random.RandomState(111).randint(0, 100, (W + 40,)).astype(np.int32)      # (far from the silence that is trimmed)
    data.save_audio_file(wav, loud, Q, format="16bit_pcm", sampling_rate=sr)
    t = np.asarray(data.load_audio_file(wav, quantization_steps=Q)[0], dtype=np.int32)
    M = len(t)
    n = M - W
    assert n >= 30
    lo, hi = W + 8, W + 20
    fn, whole = cli_generate.main(["-m", str(model), "-o", str(out), "--fast", "--seed", "4", "--keep", wav,
                                   "--redraw", "%.2f:%.2f" % (lo / float(sr), hi / float(sr)), "--best-of", str(K),
                                   "--report", str(report), "--temperature", "0.9"])
    assert os.path.basename(fn) == "generated.wav" and os.listdir(str(out)) == ["generated.wav"]
    assert wavfile.read(fn)[1].shape[0] == M == len(whole)
    assert np.array_equal(whole[:lo], t[:lo]) and np.array_equal(whole[hi:], t[hi:])
    forced = t[W:].copy()
    forced[lo - W:hi - W] = -1
    table = json.loads(report.read_text())
    (row,) = table["files"]
    assert row["file"] == "generated.wav" and row["samples"] == n and len(row["candidates"]) == K
    assert row["kept"] == sampling.pick_best(row["candidates"]) and row["nats_per_sample"] == row["candidates"][row["kept"]]
    U = np.random.RandomState(4).random_sample((K, n))
    drawn = set()
    for c in range(K):                               # every candidate is the direct generate() with its row of uniforms
        tk, ch = net.generate(n, U[c], initial_tokens=t[:W], temperature=0.9, return_chosen=True, forced=forced)
        assert sampling.chosen_nll(ch) == row["candidates"][c], c
        drawn.add(tuple(tk.cpu().tolist()[lo - W:hi - W]))
        if c == row["kept"]:
            assert np.array_equal(tk.cpu().numpy(), whole[W:])
    assert len(drawn) > 1 and len(set(row["candidates"])) == K
    assert table["total"]["samples"] == n
