"""GPU: temperature / top-k / top-p inside the decode kernels and in wn_sample_categorical_filtered.

What is exact here is exact by construction: the truncation and the draw are integer and float64 arithmetic in a fixed
order on given float32 rows, so a host restatement fed the rows the device traced (``return_probs``: the post-temperature,
pre-truncation probabilities, the very values the sampler consumed) must reproduce every token; how those rows were
computed (``expf``, summation orders) does not enter.  Only the distance of the rows to the float64 oracle has a tolerance.
"""
import numpy as np
import pytest
import torch

from oracle import wavenet_ref as R
from oracle.data_ref import onehot_pixel_image
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd._lib import check, ptr

from gpu_util import CFG1, CFG2, build, dev, to_np
from test_sampling_cpu import QS, TOP_PS, restate_draw, restate_filter, rows, top_ks, uniforms

pytestmark = pytest.mark.gpu

CONTROLS = (dict(temperature=0.8, top_k=40, top_p=0.9), dict(top_k=40), dict(top_p=0.9))


def restate_rows(P, U, top_k, top_p, chunk=128):
    """Steps 2-5 of the contract for many rows at once -- the literal restatement of test_sampling_cpu.py in array form:
    ranks are counts over the full (i, j) table of "j precedes i"; every float64 sum is a ``np.cumsum`` (sequential, in
    index order) of selected values; the draw is the first index with cumsum / last > u, Q - 1 when there is none (the
    decode kernels' clamp)."""
    P = np.asarray(P, dtype=np.float32)
    U = np.asarray(U, dtype=np.float64)
    n, Q = P.shape
    idx = np.arange(Q)
    earlier = idx[None, None, :] < idx[None, :, None]                  # [., i, j]: j < i
    out = np.empty(n, dtype=np.int64)
    for s in range(0, n, chunk):
        p = P[s:s + chunk].astype(np.float64)                           # exact
        pj, pi = p[:, None, :], p[:, :, None]
        pre = (pj > pi) | ((pj == pi) & earlier)                        # [row, i, j]: j precedes i
        rank = pre.sum(axis=2)
        pk = p.copy()
        if 0 < top_k < Q:
            pk[rank >= top_k] = 0.0
        if top_p < 1.0:
            total = np.cumsum(pk, axis=1)[:, -1]
            before = np.cumsum(np.where(pre, pk[:, None, :], 0.0), axis=2)[:, :, -1]
            keep = (before < (top_p * total)[:, None]) | (rank == 0)
            pk = np.where(keep, pk, 0.0)
        cdf = np.cumsum(pk, axis=1)
        gt = cdf / cdf[:, -1:] > U[s:s + chunk, None]
        out[s:s + chunk] = np.where(gt.any(axis=1), gt.argmax(axis=1), Q - 1)
    return out


def _filtered(prob, u, top_k, top_p):
    n, Q = prob.shape
    out = torch.full((n,), -7, device="cuda", dtype=torch.int32)
    check(_lib.lib().wn_sample_categorical_filtered(ptr(dev(prob)), ptr(dev(np.asarray(u, np.float64))), ptr(out), n, Q,
                                                    int(top_k), float(top_p), None), "wn_sample_categorical_filtered")
    return to_np(out)


@pytest.mark.parametrize("Q", QS)
def test_filtered_draw_equals_the_literal_restatement_on_every_case(Q):
    """wn_sample_categorical_filtered -- the decoders' own truncation stage behind a row loader -- against the literal double
    loop of test_sampling_cpu.py: random rows, exact ties, zeros, one-hot, a flat row; top_k in {0, 1, 2, Q-1, Q} x top_p in
    {1, 0.9, 0.5, 1e-9}; uniforms including 0 and the largest double below 1.  Token for token, no case left out; the array
    form used by the chain tests below is held against the same literal tokens."""
    rr = rows(Q)
    us = uniforms(Q)
    prob = np.stack([row for _, row in rr for _ in us])                 # every row with every uniform
    u = np.asarray([v for _ in rr for v in us], np.float64)
    cases = 0
    for k in top_ks(Q):
        for tp in TOP_PS:
            want = np.asarray([restate_draw(restate_filter(row, k, tp), v) for _, row in rr for v in us])
            got = _filtered(prob, u, k, tp)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, "Q %d top_k %d top_p %g: row %s u %r: device %d, restatement %d" % (
                Q, k, tp, rr[int(bad[0]) // len(us)][0], u[bad[0]], got[bad[0]], want[bad[0]])
            np.testing.assert_array_equal(restate_rows(prob, u, k, tp), want)
            cases += len(want)
    assert cases == 5 * 4 * len(rr) * len(us)


def test_filtered_draw_with_the_controls_off_is_wn_sample_categorical():
    rs = np.random.RandomState(4)
    for Q in QS:
        n = 200
        x = rs.standard_normal((n, Q)) * 2.0
        p = np.exp(x - x.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True)).astype(np.float32)
        u = rs.random_sample(n)
        plain = torch.empty((n,), device="cuda", dtype=torch.int32)
        check(_lib.lib().wn_sample_categorical(ptr(dev(p)), ptr(dev(u)), ptr(plain), n, Q, None), "wn_sample_categorical")
        for k, tp in ((0, 1.0), (Q, 1.0), (Q + 5, 1.0)):
            np.testing.assert_array_equal(_filtered(p, u, k, tp), to_np(plain))
        # and switched on it is another draw (the stage really runs)
        assert (_filtered(p, u, 1, 1.0) == p.argmax(1)).all()
        if Q > 7:
            assert (_filtered(p, u, 2, 0.5) != to_np(plain)).any()


def _cfg4(flags=0):
    net = FasterWaveNet(Params(R.make_params(**CFG2)), seed=1234)
    net.exec_flags = flags
    net.to_gpu()
    return net


def _kernel_models():
    """(name, model factory): the three samplers -- nine workgroups, one workgroup, and the any-shape k_decode (a 16-channel
    model, and cfg4's shape with biases, which the specialised kernels do not take)."""
    return (
        ("nine workgroups", lambda: _cfg4(0)),
        ("one workgroup", lambda: _cfg4(_lib.WN_DECODER_ONE_WORKGROUP)),
        ("k_decode, 16 channels", lambda: build(CFG1, cls=FasterWaveNet)[2]),
        ("k_decode, biases", lambda: build(CFG2, bias_scale=0.1, cls=FasterWaveNet)[2]),
    )


@pytest.mark.parametrize("which", range(4))
def test_every_emitted_token_follows_from_the_traced_row(which):
    """Chain self-consistency, 3,000 steps, for (temperature 0.8, top-k 40, top-p 0.9), top-k alone and top-p alone: the
    restatement's steps 2-5 applied to every traced row with the same uniforms give the emitted tokens, all of them."""
    name, make = _kernel_models()[which]
    net = make()
    n = 3000
    u = np.random.RandomState(31 + which).random_sample(n)
    plain = to_np(net.generate(n, u))
    for ctl in CONTROLS:
        toks, probs = net.generate(n, u, return_probs=True, **ctl)
        toks, probs = to_np(toks), to_np(probs)
        assert np.isfinite(probs).all() and np.abs(probs.sum(1) - 1.0).max() < 1e-4
        want = restate_rows(probs, u, ctl.get("top_k", 0), ctl.get("top_p", 1.0))
        bad = np.nonzero(toks != want)[0]
        assert bad.size == 0, "%s %r: first differing step %d of %d (%d differ): device %d, restatement %d" % (
            name, ctl, int(bad[0]), n, bad.size, toks[bad[0]], want[bad[0]])
        assert (toks != plain).any(), "%s %r: the controls changed nothing" % (name, ctl)
        if "top_k" in ctl:                              # every token is one of its row's 40 most probable
            rank = (probs > probs[np.arange(n), toks][:, None]).sum(1)
            assert rank.max() < ctl["top_k"]
        assert len(set(toks.tolist())) > 3                  # not a degenerate chain


def test_traced_rows_lie_within_the_decode_bar_of_the_float64_oracle():
    """The oracle's queue-cached model (RefFasterWaveNet), teacher-forced with the device's first 512 tokens: every traced
    row within 2e-5 * max(1, 1 / temperature) of the float64 softmax(oracle logits / temperature).  2e-5 is the project's
    decode bar; the factor is the softmax's sensitivity to a logit error under a temperature."""
    T, n = 0.8, 512
    net = _cfg4(0)
    u = np.random.RandomState(41).random_sample(n)
    toks, probs = net.generate(n, u, return_probs=True, temperature=T, top_k=40, top_p=0.9)
    toks, probs = to_np(toks), to_np(probs)
    p = R.make_params(**CFG2)
    w = R.init_weights(p, 1234)
    ref = R.RefFasterWaveNet(p, w, "elu")
    iw = R.input_width(p)
    buf = np.full((iw,), 127, dtype=np.int32)
    bar = 2e-5 * max(1.0, 1.0 / T)
    worst = 0.0
    for step in range(n):
        x = onehot_pixel_image(buf[-iw:].reshape(1, -1), 256)
        lg = ref._forward_one_step(x, apply_softmax=False)[0, :, 0, -1].astype(np.float64) / T
        e = np.exp(lg - lg.max())
        err = float(np.abs(probs[step] - e / e.sum()).max())
        worst = max(worst, err)
        assert err <= bar, "step %d: |device - oracle| = %g > %g" % (step, err, bar)
        buf = np.append(buf, [toks[step]]).astype(np.int32)
    print("worst |device row - float64 oracle| over %d steps: %.3g (bar %.3g)" % (n, worst, bar))


@pytest.mark.parametrize("which", [0, 1, 3])
def test_explicit_defaults_are_the_run_without_controls_bit_for_bit(which):
    net = _kernel_models()[which][1]()
    n = 1500
    u = np.random.RandomState(51).random_sample(n)
    t0, p0 = net.generate(n, u, return_probs=True)
    t0, p0 = to_np(t0).copy(), to_np(p0).copy()
    net.generate(64, u, temperature=0.7, top_k=5, top_p=0.5)              # the handle's state must not leak into the next run
    t1, p1 = net.generate(n, u, return_probs=True, temperature=1.0, top_k=0, top_p=1.0)
    np.testing.assert_array_equal(to_np(t1), t0)
    np.testing.assert_array_equal(to_np(p1).view(np.uint32), p0.view(np.uint32))
    t2 = net.generate(n, u, top_k=256)                                     # top_k >= Q is off
    np.testing.assert_array_equal(to_np(t2), t0)


def _mixed_controls(N):
    temps = [(1.0, 0.8, 1.3, 0.6)[i % 4] for i in range(N)]
    ks = [(0, 40, 0, 3, 256)[i % 5] for i in range(N)]
    ps = [(1.0, 0.9, 0.5)[i % 3] for i in range(N)]
    return temps, ks, ps


def test_generate_batch_with_per_utterance_controls_equals_generate_row_by_row():
    """28 utterances in one launch, each with controls of its own (utterances 0 and 12 have all of them off): row u is
    generate(n, uniforms[u], controls[u]) bit for bit; 30 utterances fall back to the loop with the same result; a scalar
    applies to every utterance."""
    net = _cfg4(0)
    n = 400
    for N in (28, 30):
        u = np.random.RandomState(60 + N).random_sample((N, n))
        temps, ks, ps = _mixed_controls(N)
        assert (temps[0], ks[0], ps[0]) == (1.0, 0, 1.0)
        got = to_np(net.generate_batch(n, u, temperature=temps, top_k=ks, top_p=ps))
        assert got.shape == (N, n)
        for i in (range(N) if N == 28 else (0, 7, 29)):
            want = to_np(net.generate(n, u[i], temperature=temps[i], top_k=ks[i], top_p=ps[i]))
            np.testing.assert_array_equal(got[i], want, err_msg="utterance %d of %d" % (i, N))
        np.testing.assert_array_equal(got[0], to_np(net.generate(n, u[0])))
    u = np.random.RandomState(7).random_sample((3, n))
    got = to_np(net.generate_batch(n, u, temperature=0.8, top_k=40, top_p=0.9))
    np.testing.assert_array_equal(got[2], to_np(net.generate(n, u[2], temperature=0.8, top_k=40, top_p=0.9)))
    np.testing.assert_array_equal(to_np(net.generate_batch(n, u)), to_np(net.generate_batch(n, u, None, 1.0, 0, 1.0)))
    with pytest.raises(ValueError):
        net.generate_batch(n, u, temperature=[0.8, 0.9])
    with pytest.raises(ValueError):
        net.generate(n, u[0], top_p=0.0)


def test_decoder_step_is_unaffected_by_the_handles_sampling_state():
    """wn_decoder_set_sampling is state of the handle for wn_decoder_run / _run_batch (generate() sets it through the C ABI on
    every call); wn_decoder_step keeps returning the plain probabilities whatever that state is."""
    net = build(CFG1, cls=FasterWaveNet)[2]
    lib = _lib.lib()
    tok = dev(np.full((1, net.input_width), 127, np.int32))
    net.keep_window = False
    res = []
    for ctl in ((0.7, 10, 0.8), (1.0, 0, 1.0)):
        net.prev_causal_outputs = None
        net.forward_one_step(tok, apply_softmax=True)
        check(lib.wn_decoder_set_sampling(net._decoder(), *ctl), "wn_decoder_set_sampling")
        prob = torch.empty((256,), device="cuda", dtype=torch.float32)
        check(lib.wn_decoder_step(net._decoder(), 127, ptr(prob), 1, None), "wn_decoder_step")
        res.append(to_np(prob).copy())
    np.testing.assert_array_equal(res[0].view(np.uint32), res[1].view(np.uint32))
    assert abs(float(res[0].sum()) - 1.0) < 1e-5
    # ... and a wrong value is refused with the handle's state left alone
    assert lib.wn_decoder_set_sampling(net._decoder(), 0.0, 0, 1.0) == _lib.WN_EARG
