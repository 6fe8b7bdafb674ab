"""Per-sample log-likelihood scoring on the GPU: the row form of wn_head_xent (WN_EXEC_HEAD_ROW_NLL), WaveNet.token_nll /
score against the training loss and the float64 oracle, and the evaluate command's evaluate_dir."""
import math

import numpy as np
import pytest
import torch

from gpu_util import EX, build, dev, to_np
from oracle import wavenet_ref as R
from wavenet_amd import _lib, data, scoring
from wavenet_amd._lib import check, ptr
from wavenet_amd.graph import default_loss
from wavenet_amd.train_audio import evaluate

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


@pytest.mark.parametrize("with_bias", [True, False])
def test_row_form_of_the_fused_head_and_loss_through_the_c_abi(with_bias):
    """wn_head_xent under WN_EXEC_HEAD_ROW_NLL at N = 200 (two workgroups, the second with 72 rows: two full 32-column tiles and
    one with 8 valid columns), Cin = 64, ReLU: the first N floats are the rows' negative log-likelihoods within 2e-4 of float64
    numpy (the project's logits bar is 1e-4, and a row is a log-sum-exp minus one logit), rows whose label is -1 or 256 are
    exactly 0, and NOTHING else is written -- the buffer is N x 256 floats, so a library that ignores the flag writes a gradient
    inside it and fails here instead of faulting.  loss[0] is the mean over the rows that count, as without the flag."""
    N, Cin, Q = 200, 64, 256
    rs = np.random.RandomState(11 + with_bias)
    x = rs.standard_normal((N, Cin)).astype(np.float32) * 2.0
    W = (rs.standard_normal((Q, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = (rs.standard_normal(Q) * 0.3).astype(np.float32) if with_bias else None
    tgt = rs.randint(0, Q, N).astype(np.int32)
    tgt[0::8] = rs.randint(0, 128, tgt[0::8].size)          # labels held by lane j ...
    tgt[1::8] = rs.randint(128, 256, tgt[1::8].size)        # ... and by its partner lane j + 32
    tgt[[3, 77, 131, 195, 199]] = -1
    tgt[[4, 127, 128, 192]] = 256
    counts = (tgt >= 0) & (tgt < Q)
    assert (tgt[counts] < 128).any() and (tgt[counts] >= 128).any() and (tgt == -1).any() and (tgt == 256).any()
    lib = _lib.lib()
    xd, Wd, td = dev(x), dev(W), dev(tgt)
    bd = None if b is None else dev(b)
    rows = torch.full((N, Q), SENTINEL, device="cuda")
    loss = torch.zeros((_lib.XENT_LOSS_WORDS,), device="cuda")
    flags = _lib.default_exec_flags() | _lib.WN_EXEC_HEAD_ROW_NLL
    check(lib.wn_head_xent(ptr(xd), ptr(Wd), ptr(bd), ptr(td), ptr(loss), ptr(rows), N, Cin, Q, _lib.WN_ACT_RELU, -1,
                           EX("fp16x2", flags=flags), None), "wn_head_xent (rows)")
    dlog = torch.empty((N, Q), device="cuda")
    loss2 = torch.zeros_like(loss)
    check(lib.wn_head_xent(ptr(xd), ptr(Wd), ptr(bd), ptr(td), ptr(loss2), ptr(dlog), N, Cin, Q, _lib.WN_ACT_RELU, -1,
                           EX("fp16x2"), None), "wn_head_xent")
    torch.cuda.synchronize()
    lg = np.maximum(x.astype(np.float64), 0) @ W.astype(np.float64).T + (0 if b is None else b.astype(np.float64))
    m = lg.max(1)
    want = m + np.log(np.exp(lg - m[:, None]).sum(1)) - lg[np.arange(N), np.clip(tgt, 0, Q - 1)]
    want[~counts] = 0.0
    got = to_np(rows).reshape(-1)
    err = float(np.abs(got[:N] - want).max())
    print("row form: max |nll - float64| = %.3g, loss %.6f / %.6f" % (err, float(loss[0]), float(loss2[0])))
    assert err < 2e-4, err
    assert (got[:N][~counts] == 0.0).all() and (got[:N][counts] > 0.0).all()
    assert (got[N:] == SENTINEL).all(), int((got[N:] != SENTINEL).sum())
    cnt = int(counts.sum())
    total = float(got[:N].astype(np.float64).sum())
    assert abs(float(loss[0]) * cnt - total) <= 1e-5 * total, (float(loss[0]) * cnt, total)
    assert abs(float(loss[0]) - float(loss2[0])) <= 1e-6, (float(loss[0]), float(loss2[0]))


def test_token_nll_sums_to_the_training_loss_and_takes_the_fused_launch():
    """WaveNet.token_nll on the fused-head test's model (2 x 5 layers of 32 channels, head [64, 256], B = 3, T = 500, 333
    targets, 17 of them ignored): the float64 mean of the rows over the rows that count is graph.default_loss within 1e-5
    relative, ignored rows are exactly 0, and the launch is wn_head_xent alone -- or wn_pointwise_fwd and no wn_head_xent with
    fuse_head_loss off."""
    over = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 5, residual_num_blocks=2,
                softmax_conv_channels=[64, 256])
    p, w, net = build(over, bias_scale=0.2)
    rs = np.random.RandomState(4)
    B, T, tw = 3, 500, 333
    x = dev(rs.randint(0, 256, (B, T)).astype(np.int32))
    lab = rs.randint(0, 256, (B, tw)).astype(np.int32)
    lab[0, :17] = -1
    labd = dev(lab)
    flags_before = net.exec_flags
    for fused in (True, False):
        net.fuse_head_loss = fused
        want = float(default_loss(net, x, labd).detach())
        with _lib.profile() as prof:
            rows = net.token_nll(x, labd)
            torch.cuda.synchronize()
        names = set(prof.result())
        assert ("wn_head_xent" in names) == fused and ("wn_pointwise_fwd" in names) == (not fused), sorted(names)
        assert rows.shape == (B, tw) and rows.dtype == torch.float32 and rows.is_cuda and not rows.requires_grad
        got = to_np(rows).astype(np.float64)
        assert (got[lab == -1] == 0.0).all() and (got[lab != -1] > 0.0).all()
        mean = got.sum() / int((lab != -1).sum())
        print("token_nll (fused=%s): mean %.7f, default_loss %.7f" % (fused, mean, want))
        assert abs(mean - want) <= 1e-5 * abs(want), (fused, mean, want)
        assert net.exec_flags is flags_before                        # the row flag travels with the one call only
        assert np.array_equal(to_np(net.token_nll(x, lab)), to_np(rows))          # host labels, same rows


_SCORE_MODELS = {
    256: dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 3, residual_num_blocks=2,
              softmax_conv_channels=[256, 256]),
    64: dict(quantization_steps=64, causal_conv_channels=[32], residual_conv_channels=[32] * 3, residual_num_blocks=2,
             softmax_conv_channels=[256, 64]),
}
_SCORE_CACHE = {}


def _score_case(Q):
    """(model, tokens, float64 per-sample NLL from ONE oracle pass over the whole padded signal), built once per Q."""
    if Q not in _SCORE_CACHE:
        p, w, net = build(_SCORE_MODELS[Q], bias_scale=0.2)
        C = scoring.context_width(net.params)
        assert C == 16
        n = 1000
        tokens = np.random.RandomState(Q).randint(0, Q, n).astype(np.int32)
        s = np.concatenate([np.full((C,), scoring.silence_token(Q), np.int32), tokens])
        ref = R.RefWaveNet(p, w, dtype=torch.float64)
        with torch.no_grad():
            logits = ref.forward_one_step(R.onehot_t(s[None, :], Q, torch.float64), apply_softmax=False)[0, :, 0, :].numpy()
        cols = logits[:, C - 1:C - 1 + n]                              # column C - 1 + i scores sample i
        m = cols.max(0)
        want = m + np.log(np.exp(cols - m).sum(0)) - cols[tokens, np.arange(n)]
        _SCORE_CACHE[Q] = (net, tokens, want)
    return _SCORE_CACHE[Q]


@pytest.mark.parametrize("Q,precision,fused", [(256, None, True), (256, "fp32", False), (64, None, False)])
def test_score_matches_one_oracle_pass_whatever_the_chunking(Q, precision, fused):
    """WaveNet.score of 1000 random tokens (context width 16) against ONE float64 oracle pass over the whole silence-padded
    signal: every sample within 2e-4 for pieces of 96 x 3, 250 x 2 and one piece of everything, and the three results within
    2e-4 of each other.  The same under fp32 arithmetic and on a 64-step model: both take the torch fallback."""
    net, tokens, want = _score_case(Q)
    net.gemm_precision = precision
    try:
        got = {}
        for cw, bs in ((96, 3), (250, 2), (16384, 8)):
            with _lib.profile() as prof:
                out = net.score(tokens, chunk_width=cw, batch_size=bs)
                torch.cuda.synchronize()
            assert ("wn_head_xent" in prof.result()) == fused, sorted(prof.result())
            assert out.shape == (tokens.size,) and out.dtype == torch.float32 and out.is_cuda
            got[(cw, bs)] = to_np(out).astype(np.float64)
            err = float(np.abs(got[(cw, bs)] - want).max())
            print("score Q=%d %s chunk %d x %d: max |nll - oracle| = %.3g" % (Q, precision or "fp16x2", cw, bs, err))
            assert err < 2e-4, (cw, bs, err)
        keys = list(got)
        for a in keys:
            for b in keys:
                assert float(np.abs(got[a] - got[b]).max()) < 2e-4, (a, b)
        one = net.score(tokens[:1])
        assert one.shape == (1,) and abs(float(one[0]) - want[0]) < 2e-4
        assert abs(float(net.score(dev(tokens[:1]))[0]) - want[0]) < 2e-4                 # a device tensor works as well
        empty = net.score(tokens[:0])
        assert empty.shape == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    finally:
        net.gemm_precision = None


def test_evaluate_dir_reports_each_file_and_the_sample_weighted_total(tmp_path, capsys):
    net, _, _ = _score_case(256)
    rs = np.random.RandomState(21)
    for name, n in (("a.wav", 700), ("b.wav", 431)):
        data.save_audio_file(str(tmp_path / name), rs.randint(0, 256, n).astype(np.int32), sampling_rate=8000)
    (tmp_path / "notes.txt").write_text("not audio")
    table = evaluate.evaluate_dir(net, net.params, str(tmp_path), chunk_width=200, batch_size=2)
    assert [r["file"] for r in table["files"]] == ["a.wav", "b.wav"]
    nats = 0.0
    for r in table["files"]:
        tokens, _ = data.load_audio_file(str(tmp_path / r["file"]), quantization_steps=256)
        want = scoring.summarize(net.score(tokens, chunk_width=200, batch_size=2))
        assert r["samples"] == tokens.size == want["samples"] and tokens.size > 400
        assert r["bits_per_sample"] == pytest.approx(want["bits_per_sample"], rel=1e-6)
        assert r["nats_per_sample"] == pytest.approx(r["bits_per_sample"] * math.log(2.0), rel=1e-12)
        nats += r["nats_per_sample"] * r["samples"]
    tot = table["total"]
    assert tot["samples"] == sum(r["samples"] for r in table["files"])
    assert tot["nats_per_sample"] == pytest.approx(nats / tot["samples"], rel=1e-12)
    assert tot["bits_per_sample"] == pytest.approx(tot["nats_per_sample"] / math.log(2.0), rel=1e-12)
    printed = capsys.readouterr().out
    assert "a.wav" in printed and "b.wav" in printed and "total" in printed
