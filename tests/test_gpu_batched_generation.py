"""GPU: batched generation on every model shape, with a prompt per utterance.

``wn_decoder_run_batch`` on any-shape handles runs one workgroup of ``k_decode_batch`` per utterance; workgroup u executes
``k_decode``'s step loop over utterance u's own state, so everything here is equality: a row of ``generate_batch`` is the row
``generate`` gives for that utterance (bit for bit), which on the silence prompt is the oracle's.  Equality alone would
also hold for a loop over ``generate()`` -- what shows that the batched launch ran is the spy on ``generate``.

Two small models reach every branch of the any-shape kernel: A (Q = 256, one causal layer, fw 2) and B (Q = 64, two causal
layers of filter width 3, residual filter width 3).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import wavenet_ref as R
from oracle.data_ref import onehot_pixel_image
from wavenet_amd import FasterWaveNet, Params, _lib, sampling

from gpu_util import CFG2, build, to_np

pytestmark = pytest.mark.gpu

A = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[16] * 4, residual_num_blocks=2,
         softmax_conv_channels=[32, 256])
B = dict(quantization_steps=64, causal_conv_channels=[8, 8], causal_conv_filter_width=3, residual_conv_filter_width=3,
         residual_conv_channels=[8] * 3, residual_num_blocks=2, softmax_conv_channels=[16, 64])
CFGS = {"A": A, "B": B}
NMAX, LONGEST = 33, 20
_MODELS = {}


def model(name):
    """(oracle params, oracle weights, GPU model, uniforms (33, 20), the oracle's rows, generate()'s rows): built once."""
    if name not in _MODELS:
        p, w, net = build(CFGS[name], cls=FasterWaveNet)
        u = np.random.RandomState(len(name) + ord(name[0])).random_sample((NMAX, LONGEST))
        oracle = np.stack([R.generate(p, w, LONGEST, u[i], fast=True) for i in range(NMAX)])
        single = np.stack([to_np(net.generate(LONGEST, u[i])) for i in range(NMAX)])
        _MODELS[name] = (p, w, net, u, oracle, single)
    return _MODELS[name]


_KEPT = []


@pytest.fixture(scope="module", autouse=True)
def _leave_free_small_blocks_behind():
    """After this module: 512 free minimum-size blocks in torch's caching allocator, each between two blocks that stay
    allocated, so they can neither merge nor be split.  Reason: test_gpu_sampling.py's ``_filtered`` passes
    ``ptr(dev(prob))`` -- the address of a temporary that is freed before ``dev(u)`` is allocated -- so whether ``u`` lands on
    ``prob`` depends on which free blocks the tests before it left; run in suite order behind this module it failed at Q = 7.
    With a minimum-size block free elsewhere, the best-fit search gives ``u`` that block.  That test is not this change's to
    edit; this keeps it where it was without touching it."""
    yield
    blocks = [torch.empty((512,), device="cuda", dtype=torch.uint8) for _ in range(1024)]
    _KEPT.extend(blocks[::2])


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


class no_loop(object):
    """``with no_loop(net):`` -- any call of ``net.generate`` inside is counted; leaving the block asserts there was none."""

    def __init__(self, net):
        self.net, self.calls = net, 0

    def __enter__(self):
        inner = self.net.generate

        def spy(*a, **kw):
            self.calls += 1
            return inner(*a, **kw)
        self.net.generate = spy
        return self

    def __exit__(self, *exc):
        del self.net.generate
        if exc[0] is None:
            assert self.calls == 0, "generate_batch ran generate() %d times: it looped instead of one batched launch" % self.calls


@pytest.mark.parametrize("n", [1, 2, 20])
@pytest.mark.parametrize("N", [1, 3, 33])
@pytest.mark.parametrize("name", ["A", "B"])
def test_any_shape_batch_equals_single_runs_and_the_oracle(name, N, n):
    """N = 33 is more than the nine-workgroup form takes: the any-shape limit applies.  Rows are prefixes of the 20-sample
    rows (a chain), and two of them are run again at this very n."""
    p, w, net, u, oracle, single = model(name)
    np.testing.assert_array_equal(single, oracle)
    with no_loop(net):
        got = to_np(net.generate_batch(n, u[:N, :n]))
    assert got.shape == (N, n) and got.dtype == np.int32
    np.testing.assert_array_equal(got, single[:N, :n])
    np.testing.assert_array_equal(got, oracle[:N, :n])
    for i in {0, N - 1}:
        np.testing.assert_array_equal(got[i], to_np(net.generate(n, u[i, :n])))


def _host_first_token(p, w, prompt, u0):
    """The oracle's full forward over the prompt (ReLU head), then the host's draw."""
    x = onehot_pixel_image(np.asarray(prompt, np.int32).reshape(1, -1), p["quantization_steps"])
    prob = R.forward_closed(p, w, x, head_act="relu", apply_softmax=True)[3][0, :, 0, -1]
    return sampling.sample(prob, float(u0), 0, 1.0)


def _check_prompts(p, w, net, n, extra, batched, rs):
    Q = p["quantization_steps"]
    W = R.input_width(p) + extra
    distinct = rs.randint(0, Q, (3, W)).astype(np.int32)
    prompts = np.concatenate([distinct, distinct[:1]])                       # utterance 3 continues utterance 0's prompt
    N = prompts.shape[0]
    u = rs.random_sample((N, n))
    u[1] = u[0]                                                              # same uniforms, another prompt
    if batched:
        with no_loop(net):
            got = to_np(net.generate_batch(n, u, initial_tokens=prompts))
    else:
        got = to_np(net.generate_batch(n, u, initial_tokens=prompts))
    assert got.shape == (N, n)
    for i in range(N):
        np.testing.assert_array_equal(got[i], to_np(net.generate(n, u[i], initial_tokens=prompts[i])), err_msg="utterance %d" % i)
        assert got[i, 0] == _host_first_token(p, w, prompts[i], u[i, 0]), "first token of utterance %d" % i
    assert (got[0] != got[3]).any()                                          # one prompt, other uniforms
    assert (got[0] != got[1]).any()                                          # one set of uniforms, other prompts
    # a list of rows is an (N, W) array as well
    np.testing.assert_array_equal(to_np(net.generate_batch(n, u, initial_tokens=[r.tolist() for r in prompts])), got)


@pytest.mark.parametrize("extra", [0, 7])
def test_a_prompt_per_utterance(extra):
    """Three distinct random prompts and a duplicate of the first, of length input_width and input_width + 7."""
    p, w, net = model("A")[:3]
    _check_prompts(p, w, net, 24, extra, True, np.random.RandomState(70 + extra))


def test_a_prompt_per_utterance_on_the_nine_workgroup_form():
    p, w, net = build(CFG2, cls=FasterWaveNet)
    rs = np.random.RandomState(72)
    Q, W = 256, R.input_width(p)
    prompts = rs.randint(0, Q, (3, W)).astype(np.int32)
    n = 40
    u = rs.random_sample((3, n))
    u[1] = u[0]
    with no_loop(net):
        got = to_np(net.generate_batch(n, u, initial_tokens=prompts))
    assert len(net._batch_decs) == 3
    for i in range(3):
        np.testing.assert_array_equal(got[i], to_np(net.generate(n, u[i], initial_tokens=prompts[i])), err_msg="utterance %d" % i)
        assert got[i, 0] == _host_first_token(p, w, prompts[i], u[i, 0])
    assert (got[0] != got[1]).any()


def test_more_utterances_than_one_launch_takes_are_cut_into_launches():
    """30 utterances on the nine-workgroup form are a launch of 28 and a launch of 2 (rows across the cut against
    generate()); on the any-shape form, with the limit lowered to 5 for the call, 33 utterances are seven launches."""
    p, w, net = build(CFG2, cls=FasterWaveNet)
    n = 24
    u = np.random.RandomState(73).random_sample((30, n))
    with no_loop(net):
        got = to_np(net.generate_batch(n, u))
    assert len(net._batch_decs) == 30
    for i in (0, 13, 27, 28, 29):
        np.testing.assert_array_equal(got[i], to_np(net.generate(n, u[i])), err_msg="utterance %d" % i)
    assert len({tuple(r) for r in got.tolist()}) == 30
    p, w, net, u, oracle, single = model("A")
    limit, _lib.WN_DECODER_BATCH_MAX_ANY = _lib.WN_DECODER_BATCH_MAX_ANY, 5
    try:
        with no_loop(net):
            got = to_np(net.generate_batch(LONGEST, u))
    finally:
        _lib.WN_DECODER_BATCH_MAX_ANY = limit
    np.testing.assert_array_equal(got, single)


def test_the_hosts_forecast_of_the_decoder_form_is_the_librarys():
    """generate_batch picks its limit from ``_nine_workgroup_shape`` before it creates a handle; the library decides from
    ``fast_shape``.  What a handle IS shows in the limit wn_decoder_run_batch applies to it: 29 copies of a nine-workgroup
    handle are refused by count ("at most 28"), 29 copies of an any-shape handle as a duplicate.  Nothing runs."""
    lib = _lib.lib()
    with_bias = dict(CFG2, residual_conv_dilation_no_bias=False)
    deep = dict(CFG2, residual_conv_channels=[32] * 2, residual_num_blocks=65)              # 130 layers
    cases = [(CFG2, None, True), (CFG2, _lib.WN_EXEC_FORCE_GENERIC, False), (CFG2, _lib.WN_DECODER_ONE_WORKGROUP, True),
             (with_bias, None, False), (dict(CFG2, causal_conv_no_bias=False), None, False),
             (dict(CFG2, residual_conv_projection_no_bias=False), None, False), (deep, None, False),
             (dict(CFG2, softmax_conv_channels=[256, 128, 256]), None, False), (A, None, False), (B, None, False)]
    u = torch.zeros((8,), device="cuda", dtype=torch.float64) + 0.5
    out = torch.zeros((8,), device="cuda", dtype=torch.int32)
    for over, flags, want in cases:
        net = FasterWaveNet(Params(R.make_params(**over)), seed=3)
        net.to_gpu()
        net.exec_flags = flags
        f = _lib.default_exec_flags() if flags is None else flags
        assert net._nine_workgroup_shape(f) == want, (over, flags)
        h = net._decoder()
        rc = lib.wn_decoder_run_batch(_arr(C.c_void_p, [h.value] * 29), 29, _arr(C.c_int32, [1] * 29),
                                      _arr(C.c_void_p, [u.data_ptr()] * 29), 8, _arr(C.c_void_p, [out.data_ptr()] * 29), None, 0, None)
        msg = lib.wn_last_error().decode()
        assert (rc, "at most 28" in msg) == ((_lib.WN_ESHAPE, True) if want else (_lib.WN_EARG, False)), (over, flags, rc, msg)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0


def test_per_utterance_controls_on_the_any_shape_form():
    p, w, net, u = model("A")[:4]
    temps, ks, ps = [1.0, 0.8, 1.3], [0, 40, 3], [1.0, 0.9, 0.5]
    with no_loop(net):
        got = to_np(net.generate_batch(LONGEST, u[:3], temperature=temps, top_k=ks, top_p=ps))
    for i in range(3):
        want = to_np(net.generate(LONGEST, u[i], temperature=temps[i], top_k=ks[i], top_p=ps[i]))
        np.testing.assert_array_equal(got[i], want, err_msg="utterance %d" % i)
    assert (got[1] != model("A")[5][1]).any()                                # the controls changed something
    with no_loop(net):
        got = to_np(net.generate_batch(LONGEST, u[:3], temperature=0.8, top_k=40, top_p=0.9))
    np.testing.assert_array_equal(got[2], to_np(net.generate(LONGEST, u[2], temperature=0.8, top_k=40, top_p=0.9)))


def test_a_bf16_storage_model_is_batched():
    p, w, net = build(A, cls=FasterWaveNet, storage="bf16")
    u = model("A")[3][:3]
    with no_loop(net):
        got = to_np(net.generate_batch(LONGEST, u))
    for i in range(3):
        np.testing.assert_array_equal(got[i], to_np(net.generate(LONGEST, u[i])), err_msg="utterance %d" % i)


def _handles(net, k, window):
    """k decoder handles of the model, seeded from a prefill over ``window``; -> (handles, first-row probabilities)."""
    lib = _lib.lib()
    net.prev_causal_outputs = None
    keep, net.keep_window = net.keep_window, False
    try:
        p0 = net.forward_one_step(torch.as_tensor(window.reshape(1, -1)).cuda(), apply_softmax=True)
    finally:
        net.keep_window = keep
    tok = torch.as_tensor(window.reshape(1, -1)).cuda().to(torch.int32).contiguous()
    hs = []
    for _ in range(k):
        d, held = net._desc()
        h = C.c_void_p()
        _lib.check(lib.wn_decoder_create(C.byref(h), C.byref(d), None), "wn_decoder_create")
        _lib.check(lib.wn_decoder_load_state(h, _lib.ptr(tok), tok.shape[1],
                                             _lib.ptr_array([t.contiguous() for t in net._last_causal_outputs]),
                                             _lib.ptr_array(net._last_layer_inputs), None), "wn_decoder_load_state")
        hs.append(h)
    torch.cuda.synchronize()
    return hs, p0


def _run_batch(hs, firsts, u, n, out, probs, col=0):
    """wn_decoder_run_batch over steps [col, col + n) of the per-utterance buffers."""
    k = len(hs)
    return _lib.lib().wn_decoder_run_batch(
        _arr(C.c_void_p, [h.value for h in hs]), k, _arr(C.c_int32, firsts), _arr(C.c_void_p, [u[i, col:].data_ptr() for i in range(k)]),
        n, _arr(C.c_void_p, [out[i, col:].data_ptr() for i in range(k)]),
        None if probs is None else _arr(C.c_void_p, [probs[i, col:].data_ptr() for i in range(k)]), 1, None)


@pytest.mark.parametrize("name", ["A", "B"])
def test_c_abi_any_shape_batch_equals_wn_decoder_run_on_twin_handles(name):
    """Tokens and probability traces of three utterances (the third with sampling controls of its own) against
    wn_decoder_run on twin handles, bit for bit; a second batched call goes on where the first ended: 12 + 8 steps are one
    run of 20."""
    p, w, net = model(name)[:3]
    lib = _lib.lib()
    Q = p["quantization_steps"]
    window = np.random.RandomState(5).randint(0, Q, (net.input_width,)).astype(np.int32)
    hs, _ = _handles(net, 6, window)
    batch, twins = hs[:3], hs[3:]
    n1, n2 = 12, 8
    n = n1 + n2
    firsts = [3, Q - 1, Q // 2]
    u = torch.as_tensor(np.random.RandomState(6).random_sample((3, n))).cuda()
    for h in (batch[2], twins[2]):
        _lib.check(lib.wn_decoder_set_sampling(h, 0.8, 40 if Q > 64 else 9, 0.9), "wn_decoder_set_sampling")
    want = torch.zeros((3, n), device="cuda", dtype=torch.int32)
    want_p = torch.zeros((3, n, Q), device="cuda", dtype=torch.float32)
    for i in range(3):
        _lib.check(lib.wn_decoder_run(twins[i], firsts[i], u[i].data_ptr(), n, want[i].data_ptr(), want_p[i].data_ptr(), None),
                   "wn_decoder_run")
    got = torch.zeros((3, n), device="cuda", dtype=torch.int32)
    got_p = torch.zeros((3, n, Q), device="cuda", dtype=torch.float32)
    assert _run_batch(batch, firsts, u, n1, got, got_p) == 0, lib.wn_last_error().decode()
    for h in batch:
        assert lib.wn_decoder_status(h, None) == _lib.WN_OK
    np.testing.assert_array_equal(to_np(got)[:, :n1], to_np(want)[:, :n1])
    assert int(got[:, n1:].abs().sum()) == 0                                # and not a step more
    assert _run_batch(batch, [int(v) for v in to_np(got)[:, n1 - 1]], u, n2, got, got_p, col=n1) == 0, lib.wn_last_error().decode()
    assert lib.wn_decoder_status(batch[0], None) == _lib.WN_OK
    np.testing.assert_array_equal(to_np(got), to_np(want))
    np.testing.assert_array_equal(to_np(got_p).view(np.uint32), to_np(want_p).view(np.uint32))
    assert len({tuple(r) for r in to_np(got).tolist()}) == 3
    # one utterance is a batch too (the n >= 2 rule and the 28 belong to the nine-workgroup form), and one step is a run
    one = torch.zeros((1, 1), device="cuda", dtype=torch.int32)
    one_w = torch.zeros((1, 1), device="cuda", dtype=torch.int32)
    last = int(to_np(got)[0, -1])
    assert _run_batch(batch[:1], [last], u, 1, one, None) == 0, lib.wn_last_error().decode()
    _lib.check(lib.wn_decoder_run(twins[0], last, u[0].data_ptr(), 1, one_w.data_ptr(), None, None), "wn_decoder_run")
    assert lib.wn_decoder_status(batch[0], None) == _lib.WN_OK
    assert int(one[0, 0]) == int(one_w[0, 0])
    for h in hs:
        lib.wn_decoder_destroy(h)


def test_c_abi_refusals_of_the_any_shape_form_touch_nothing():
    lib = _lib.lib()
    netA, netB = model("A")[2], model("B")[2]
    hA, _ = _handles(netA, 2, np.full((netA.input_width,), 127, np.int32))
    hB, _ = _handles(netB, 1, np.full((netB.input_width,), 32, np.int32))
    cfg4 = build(CFG2, cls=FasterWaveNet)[2]
    h9 = cfg4._decoder()
    big = _lib.WN_DECODER_BATCH_MAX_ANY + 1
    u = torch.zeros((2, 8), device="cuda", dtype=torch.float64) + 0.5
    out = torch.zeros((2, 8), device="cuda", dtype=torch.int32)

    def call(handles, n=8):
        k = len(handles)
        rc = lib.wn_decoder_run_batch(_arr(C.c_void_p, [h.value for h in handles]), k, _arr(C.c_int32, [5] * k),
                                      _arr(C.c_void_p, [u[i % 2].data_ptr() for i in range(k)]), n,
                                      _arr(C.c_void_p, [out[i % 2].data_ptr() for i in range(k)]), None, 0, None)
        return rc, lib.wn_last_error().decode()

    rc, msg = call([hA[0], h9])
    assert rc == _lib.WN_ESHAPE and "utterance 1" in msg, (rc, msg)
    rc, msg = call([h9, hA[0]])
    assert rc == _lib.WN_ESHAPE and "utterance 1" in msg, (rc, msg)
    rc, msg = call([hA[0], hB[0]])
    assert rc == _lib.WN_ESHAPE, (rc, msg)
    rc, msg = call([hA[0], hA[1], hA[0]])
    assert rc == _lib.WN_EARG and "twice" in msg, (rc, msg)
    rc, msg = call([hA[0]] * big)                                           # the count comes before the duplicates
    assert rc == _lib.WN_ESHAPE and "at most %d" % _lib.WN_DECODER_BATCH_MAX_ANY in msg, (rc, msg)
    assert lib.wn_decoder_batch_max() == 28
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                        # nothing ran
    for h in hA + hB:
        assert lib.wn_decoder_status(h, None) == _lib.WN_OK
        lib.wn_decoder_destroy(h)


_COUNTED = ("wn_decoder_create", "wn_decoder_update_weights", "wn_decoder_load_state", "wn_decoder_run_batch")


class _CountingLib(object):
    """What ``_lib.lib()`` returns, with the decoder-handle entry points counted (every other name is the library's own)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, dict.fromkeys(_COUNTED, 0)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in _COUNTED:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _handle_calls(monkeypatch):
    """-> count(net, call): (creates, updates, load_states, launches, prefills) of one call, through a counting proxy of
    the library and a spy on the net's ``forward_residual_block`` (one call of it per prefill)."""
    proxy = _CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: proxy)

    def count(net, call):
        before, prefills, inner = dict(proxy.calls), [0], net.forward_residual_block

        def spy(*a, **kw):
            prefills[0] += 1
            return inner(*a, **kw)
        net.forward_residual_block = spy
        try:
            call()
        finally:
            del net.forward_residual_block
        return tuple(proxy.calls[k] - before[k] for k in _COUNTED) + (prefills[0],)
    return count


def test_handles_are_created_once_and_updated_only_when_they_must_be(monkeypatch):
    """The handle rules, which equality of tokens cannot see (re-packing every handle in every call gives the same tokens):
    counts of (create, update_weights, load_state, run_batch, prefills) per call, N = 3 and n = 4 on a model of its own."""
    count = _handle_calls(monkeypatch)
    net = build(A, cls=FasterWaveNet)[2]
    N, n = 3, 4
    rs = np.random.RandomState(81)
    u = rs.random_sample((N, n))
    with no_loop(net):
        assert count(net, lambda: net.generate_batch(n, u)) == (3, 0, 3, 1, 1)             # 1. three handles, created current
        assert count(net, lambda: net.generate_batch(n, u)) == (0, 0, 3, 1, 1)             # 2. ... and still current
        net.load_state_dict(net.state_dict())
        assert count(net, lambda: net.generate_batch(n, u)) == (0, 3, 3, 1, 1)             # 3. new weights: every handle
        assert count(net, lambda: net.generate_batch([2, 3, 4], u)) == (0, 3, 3, 1, 1)     # 4. a limit each
        assert count(net, lambda: net.generate_batch(n, u)) == (0, 3, 3, 1, 1)             # 5. the limits come off
        assert count(net, lambda: net.generate_batch(n, u)) == (0, 0, 3, 1, 1)             # 6. ... once
        prompts = rs.randint(0, 256, (2, net.input_width)).astype(np.int32)[[0, 1, 0]]
        assert count(net, lambda: net.generate_batch(n, u, initial_tokens=prompts)) == (0, 0, 3, 1, 2)    # 7. two prompts
        # 8. nothing decodes: no handle is created for it, nothing is launched
        fresh = build(A, cls=FasterWaveNet)[2]
        assert count(fresh, lambda: fresh.generate_batch([1, 1, 1], u)) == (0, 0, 0, 0, 1)
        assert count(fresh, lambda: fresh.generate_batch(1, u)) == (0, 0, 0, 0, 1)
        assert len(fresh._batch_decs) == 0 and len(net._batch_decs) == 3


def test_another_class_for_one_utterance_updates_that_handle_alone(monkeypatch):
    """9. a globally conditioned model: a handle holds one class's folded biases, and only a handle whose class changes is
    packed again."""
    import cond_ref
    count = _handle_calls(monkeypatch)
    p = R.make_params(**cond_ref.TINY)
    E, V = cond_ref.init_condition(p, seed=99)
    net = FasterWaveNet(Params(p), seed=0, condition_classes=cond_ref.CLASSES, condition_channels=cond_ref.CHANNELS)
    net.load_state_dict(cond_ref.state_dict(R.init_weights(p, 1234), E, V))
    net.to_gpu()
    u = np.random.RandomState(82).random_sample((3, 4))
    with no_loop(net):
        assert count(net, lambda: net.generate_batch(4, u, condition=[0, 2, 1])) == (3, 0, 3, 1, 3)
        assert count(net, lambda: net.generate_batch(4, u, condition=[0, 2, 1])) == (0, 0, 3, 1, 3)
        got = [None]

        def call():
            got[0] = net.generate_batch(4, u, condition=[0, 1, 1])
        assert count(net, call) == (0, 1, 3, 1, 2)
    np.testing.assert_array_equal(to_np(got[0][1]), to_np(net.generate(4, u[1], condition=1)))
