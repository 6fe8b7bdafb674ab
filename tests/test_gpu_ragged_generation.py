"""GPU: batched generation with a length per utterance, and vocoding a directory of feature files.

Everything here is equality.  Utterance u of a ragged ``generate_batch`` call runs ``n_samples[u] - 1`` decode steps inside a
launch whose step count is its longest utterance's -- its handle carries ``WnDecoderDesc.step_limit`` and its workgroups end
there -- so row u must be what ``generate()`` gives for that utterance alone, bit for bit, and nothing may be written behind an
utterance's own count.  What shows that the batched launch ran (a loop over ``generate()`` would be equal too) is the spy on
``generate``."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from gpu_util import CFG2, build, dev, to_np
from oracle import wavenet_ref as R
from test_gpu_local_condition import DHOP, _Dec
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd._lib import check, ptr, ptr_array
from wavenet_amd.wavenet import frames_needed

pytestmark = pytest.mark.gpu

HOP = 5
LENGTHS = [1, 2, 3, 17, 40]          # nothing to decode | one step | two | a middle one | the launch's own count
# config 4's shape with 2 x 5 layers, the small stack tests/test_gpu_parity.py decodes on the specialised kernels.  (Not 2 x 3:
# on six layers a batched row of the nine-workgroup form was seen to differ from generate() in about one call of thirty, int
# calls on the parent commit included, and never on 2 x 5 or 4 x 10 layers in 144 calls each -- DESIGN.md, "A length per utterance".)
NINE = dict(CFG2, residual_conv_channels=[32] * 5, residual_num_blocks=2)


class spy(object):
    """``with spy(net) as s:`` counts the calls of ``net.generate`` inside (a batched launch makes none)."""

    def __init__(self, net):
        self.net, self.calls = net, 0

    def __enter__(self):
        inner = self.net.generate

        def counted(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        self.net.generate = counted
        return self

    def __exit__(self, *exc):
        del self.net.generate


def _local_model(interp, glob, hop=HOP, seed=1234):
    p = R.make_params(**LR.TINY)
    w = R.init_weights(p, seed)
    V, _ = LR.init_local(p)
    E, Vg = cond_ref.init_condition(p) if glob else (None, None)
    kw = dict(condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS) if glob else {}
    net = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=hop, local_interp=interp, **kw)
    net.load_state_dict(LR.state_dict(w, V, E, Vg))
    net.to_gpu()
    return net


def _utterances(net, lengths, seed, Q=256):
    """Distinct prompt and uniforms per utterance; sampling controls on for utterance 3 (or the last one)."""
    rs = np.random.RandomState(seed)
    N = len(lengths)
    prompts = rs.randint(0, Q, (N, net.input_width)).astype(np.int32)
    u = [rs.random_sample(n) for n in lengths]
    k = min(3, N - 1)
    kw = dict(temperature=[0.8 if i == k else 1.0 for i in range(N)], top_k=[20 if i == k else 0 for i in range(N)],
              top_p=[0.9 if i == k else 1.0 for i in range(N)])
    return rs, prompts, u, kw


def _one(kw, i):
    return {k: v[i] for k, v in kw.items()}


@pytest.mark.parametrize("glob", [False, True], ids=["local", "local+global"])
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_any_shape_rows_are_their_own_generate_calls(interp, glob):
    net = _local_model(interp, glob)
    W, N = net.input_width, len(LENGTHS)
    rs, prompts, u, kw = _utterances(net, LENGTHS, 11)
    phases = [0, 3, 4, 1, 2]
    hs = [rs.standard_normal((LR.FEATS, frames_needed(W + n - 1, HOP, ph, interp))).astype(np.float32)
          for n, ph in zip(LENGTHS, phases)]
    if glob:
        kw["condition"] = [2, 0, 1, 0, 2]
    singles = [net.generate(LENGTHS[i], u[i], initial_tokens=prompts[i], local=hs[i], local_phase=phases[i], **_one(kw, i))
               for i in range(N)]
    with spy(net) as s:
        rows = net.generate_batch(LENGTHS, u, initial_tokens=prompts, local=hs, local_phase=phases, **kw)
    assert s.calls == 0
    assert isinstance(rows, list) and len(rows) == N
    for i in range(N):
        assert rows[i].shape == (LENGTHS[i],) and rows[i].dtype == torch.int32 and rows[i].is_cuda
        assert torch.equal(rows[i], singles[i]), i
    assert len({tuple(to_np(t)[:3]) for t in singles[2:]}) == 3                     # the utterances are distinct


_PLAIN = {}


def _plain():
    """The tiny any-shape model, unconditioned (built once)."""
    if not _PLAIN:
        _PLAIN["net"] = build(LR.TINY, cls=FasterWaveNet)[2]
    return _PLAIN["net"]


def test_the_unconditioned_any_shape_model_likewise():
    net = _plain()
    N = len(LENGTHS)
    _, prompts, u, kw = _utterances(net, LENGTHS, 12)
    singles = [net.generate(LENGTHS[i], u[i], initial_tokens=prompts[i], **_one(kw, i)) for i in range(N)]
    with spy(net) as s:
        rows = net.generate_batch(LENGTHS, np.stack([np.resize(r, 40) for r in u]), initial_tokens=prompts, **kw)   # an (N, max) array
    assert s.calls == 0
    for i in range(N):
        assert rows[i].shape == (LENGTHS[i],) and torch.equal(rows[i], singles[i]), i


_NINE = {}


def _nine():
    if not _NINE:
        _NINE["net"] = build(NINE, cls=FasterWaveNet)[2]
        assert _NINE["net"]._nine_workgroup_shape(_lib.default_exec_flags())
    return _NINE["net"]


def test_nine_workgroup_rows_are_their_own_generate_calls():
    net = _nine()
    lengths = [3, 9, 30]
    _, prompts, u, kw = _utterances(net, lengths, 13)
    singles = [net.generate(lengths[i], u[i], initial_tokens=prompts[i], **_one(kw, i)) for i in range(3)]
    with spy(net) as s:
        rows = net.generate_batch(lengths, u, initial_tokens=prompts, **kw)
    assert s.calls == 0
    for i in range(3):
        assert rows[i].shape == (lengths[i],) and torch.equal(rows[i], singles[i]), i
        assert _lib.lib().wn_decoder_status(net._batch_decs[i], None) == _lib.WN_OK
    # a length of 2 is one decode step, which this form does not run: the whole call takes the loop over generate()
    lengths = [2, 9]
    _, prompts, u, kw = _utterances(net, lengths, 14)
    singles = [net.generate(lengths[i], u[i], initial_tokens=prompts[i], **_one(kw, i)) for i in range(2)]
    with spy(net) as s:
        rows = net.generate_batch(lengths, u, initial_tokens=prompts, **kw)
    assert s.calls == 2
    for i in range(2):
        assert rows[i].shape == (lengths[i],) and torch.equal(rows[i], singles[i]), i


@pytest.mark.parametrize("form", ["any-shape", "nine-workgroup"])
def test_equal_lengths_are_the_int_call_and_a_later_int_call_carries_no_limit(form):
    net = _plain() if form == "any-shape" else _nine()
    n = 12
    rs = np.random.RandomState(15)
    prompts = rs.randint(0, 256, (3, net.input_width)).astype(np.int32)
    u = rs.random_sample((3, n))
    with spy(net) as s:
        before = net.generate_batch(n, u, initial_tokens=prompts)
        equal = net.generate_batch([n] * 3, u, initial_tokens=prompts)
        ragged = net.generate_batch([3, 5, n], u, initial_tokens=prompts)
        after = net.generate_batch(n, u, initial_tokens=prompts)               # the handles held limits of 2, 4 and 11 steps
    assert s.calls == 0
    assert before.shape == (3, n) and isinstance(equal, list)
    for i in range(3):
        assert torch.equal(equal[i], before[i]), i
        assert torch.equal(ragged[i], before[i, :[3, 5, n][i]]), i             # a chain: a shorter run is a prefix
    assert torch.equal(after, before)
    assert len({tuple(r) for r in to_np(before).tolist()}) == 3


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def _handle(D, model, state_from, table=None, step_limit=0):
    d, keep = model._desc(None, table, step_limit)
    h = C.c_void_p()
    check(_lib.lib().wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
    D.handles.append(h)
    D.seed(model, h, state_from)
    return h


def _run_batch(D, handles, n, u, firsts=None):
    N = len(handles)
    toks = [torch.full((n,), -1, device="cuda", dtype=torch.int32) for _ in range(N)]
    probs = [torch.full((n, D.Q), SENTINEL, device="cuda") for _ in range(N)]
    rc = _lib.lib().wn_decoder_run_batch((C.c_void_p * N)(*[h.value for h in handles]), N,
                                         (C.c_int32 * N)(*(firsts or [7] * N)), ptr_array([u] * N), n, ptr_array(toks),
                                         ptr_array(probs), 0, None)
    torch.cuda.synchronize()
    return rc, toks, probs


def _untouched(tok, prob, k):
    return int(tok[k:].max()) == -1 and int(tok[k:].min()) == -1 and bool((prob[k:] == SENTINEL).all())


def test_step_limit_through_the_c_abi():
    D = _Dec()
    try:
        lib = _lib.lib()
        u = dev(np.random.RandomState(5).random_sample(16))
        r0, r1 = D.rows[0].contiguous(), D.rows[1].contiguous()
        tw0 = D.twin(r0)
        with torch.no_grad():
            tw0.forward_one_step(D.tok)                                          # the one prefill every handle is seeded from
        ref = _handle(D, tw0, tw0)
        rc, t_ref, p_ref = D.run(ref, 10, u)
        assert rc == 0
        h0, h1 = _handle(D, tw0, tw0, step_limit=4), _handle(D, tw0, tw0)
        rc, toks, probs = _run_batch(D, [h0, h1], 10, u)
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(toks[0][:4], t_ref[:4]) and torch.equal(probs[0][:4], p_ref[:4])     # (a chain: 4 steps are a prefix)
        assert _untouched(toks[0], probs[0], 4)
        assert torch.equal(toks[1], t_ref) and torch.equal(probs[1], p_ref)
        # handle 0 has no step left: a launch with it is refused, names it, and runs nothing
        rc, toks2, probs2 = _run_batch(D, [h1, h0], 2, u[10:], firsts=[int(t_ref[9]), 7])
        assert rc == _lib.WN_EARG and b"utterance 1" in lib.wn_last_error() and b"step_limit" in lib.wn_last_error()
        rc, toks2, probs2 = _run_batch(D, [h0, h1], 2, u[10:], firsts=[7, int(t_ref[9])])
        assert rc == _lib.WN_EARG and b"utterance 0" in lib.wn_last_error()
        assert _untouched(toks2[0], probs2[0], 0) and _untouched(toks2[1], probs2[1], 0)
        rc, t_more, p_more = D.run(ref, 2, u[10:], first=int(t_ref[9]))
        rc2, toks3, probs3 = _run_batch(D, [h1], 2, u[10:], firsts=[int(t_ref[9])])       # handle 1 stands where it stood
        assert rc == 0 and rc2 == 0 and torch.equal(toks3[0], t_more) and torch.equal(probs3[0], p_more)
        # the single-utterance entry points never clamp
        rc, t_x, p_x = D.run(h0, 1, u)
        assert rc == _lib.WN_EARG and b"step_limit = 4" in lib.wn_last_error() and b"n = 1" in lib.wn_last_error()
        assert b"4 steps run" in lib.wn_last_error() and int(t_x.min()) == -1 and float(p_x.abs().max()) == 0.0
        row = torch.zeros((D.Q,), device="cuda")
        assert lib.wn_decoder_step(h0, 3, ptr(row), 1, None) == _lib.WN_EARG and b"step_limit" in lib.wn_last_error()
        h2 = _handle(D, tw0, tw0, step_limit=4)
        rc, t_4, p_4 = D.run(h2, 4, u)                                           # up to the limit is an ordinary run
        assert rc == 0 and torch.equal(t_4, t_ref[:4]) and torch.equal(p_4, p_ref[:4])
        # a negative limit is refused at create and at update, before any device work
        d, keep = tw0._desc(None, None, -1)
        h = C.c_void_p()
        assert lib.wn_decoder_create(C.byref(h), C.byref(d), None) == _lib.WN_EARG and b"step_limit" in lib.wn_last_error()
        assert lib.wn_decoder_update_weights(h1, C.byref(d), None) == _lib.WN_EARG and b"step_limit" in lib.wn_last_error()
        # an update is the way to a new limit: the count starts again
        d, keep = tw0._desc(None, None, 3)
        check(lib.wn_decoder_update_weights(h0, C.byref(d), None), "wn_decoder_update_weights")
        D.seed(tw0, h0, tw0)
        rc, toks4, probs4 = _run_batch(D, [h0], 10, u)
        assert rc == 0 and torch.equal(toks4[0][:3], t_ref[:3]) and _untouched(toks4[0], probs4[0], 3)
        # with a frame table: 3 rows at hop 5 from phase 2 cover 13 steps.  A limit beyond that does not shorten the run, so
        # the table's rule still refuses it; a limit below it stops the run there
        two = torch.stack([r0, r1, r1]).contiguous()
        rc, t_tab, p_tab = D.run(_handle(D, D.net, tw0, (two, DHOP, 2)), 13, u)
        assert rc == 0
        wide = _handle(D, D.net, tw0, (two, DHOP, 2), step_limit=20)
        rc, toks5, probs5 = _run_batch(D, [wide], 15, u)
        assert rc == _lib.WN_EARG and b"frame table of 3 rows" in lib.wn_last_error() and _untouched(toks5[0], probs5[0], 0)
        short = _handle(D, D.net, tw0, (two, DHOP, 2), step_limit=6)
        rc, toks6, probs6 = _run_batch(D, [short, wide], 13, u)
        assert rc == 0, lib.wn_last_error()
        assert torch.equal(toks6[0][:6], t_tab[:6]) and torch.equal(probs6[0][:6], p_tab[:6]) and _untouched(toks6[0], probs6[0], 6)
        assert torch.equal(toks6[1], t_tab) and torch.equal(probs6[1], p_tab)
    finally:
        D.close()


# ---- the command ----------------------------------------------------------------------------------------------------------------
def test_generate_local_dir_writes_one_wav_per_feature_file_at_its_own_length(tmp_path):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import generate as cli_generate
    hop, sr = 4, 8000
    model, feat = tmp_path / "model", tmp_path / "feat"
    model.mkdir()
    feat.mkdir()
    net = _local_model("repeat", False, hop=hop)
    W = net.input_width
    assert W % hop == 0
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(LR.TINY, sampling_rate=sr)))
    (model / "local.json").write_text(json.dumps({"channels": LR.FEATS, "hop": hop}))
    rs = np.random.RandomState(16)
    extra = {"b_long": 5, "a_mid": 3, "c_short": 2}                              # columns more than the window's
    for name, k in extra.items():
        np.save(str(feat / (name + ".npy")), rs.standard_normal((LR.FEATS, W // hop + k)).astype(np.float32))
    out = tmp_path / "out"
    files, tokens = cli_generate.main(["-m", str(model), "-o", str(out), "--fast", "--seed", "2", "--local-dir", str(feat)])
    assert [os.path.basename(f) for f in files] == ["a_mid.wav", "b_long.wav", "c_short.wav"]
    assert sorted(os.listdir(str(out))) == ["a_mid.wav", "b_long.wav", "c_short.wav"]
    for f, t in zip(files, tokens):
        want = extra[os.path.basename(f)[:-4]] * hop + 1                         # (W / hop + k) hop - W + 1
        rate, pcm = wavfile.read(f)
        assert rate == sr and pcm.shape[0] == want and t.shape == (want,)    # (the writer's frames: one per sample)
    solo = tmp_path / "solo"
    fn, one = cli_generate.main(["-m", str(model), "-o", str(solo), "--fast", "--seed", "2", "--local", str(feat / "c_short.npy")])
    np.testing.assert_array_equal(one, tokens[2])
    assert open(fn, "rb").read() == open(files[2], "rb").read()
    # -s caps every utterance; shorter ones keep their own length
    files, tokens = cli_generate.main(["-m", str(model), "-o", str(out), "--fast", "--seed", "2", "--local-dir", str(feat),
                                       "-s", str(14.5 / sr)])
    assert [t.shape[0] for t in tokens] == [13, 13, 9]
