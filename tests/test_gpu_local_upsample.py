"""The learned upsampling layer ahead of the local projection (``local_upsample`` = U) on the GPU.

A U-model at hop H = 12 is, by construction, a U = 1 model at hop H' = H / U fed the layer's output: the first group of tests
holds the two against each other bit for bit (same shared weights; the twin gets ``upsampled_features(h)``, cut or gathered by
the alignment rule, at phase % H').  The layer itself -- its output and its two gradients -- is held against the float64
restatement of tests/local_upsample_ref.py at the tolerances the neighbouring files use for the same quantities.

The base case is local_cond_ref's: cond_ref.TINY (two blocks of three 32-channel layers), B = 3, T = 70, F = 5, hop 12."""
import numpy as np
import pytest
import torch

import local_cond_ref as LR
import local_upsample_ref as LU
from gpu_util import dev, to_np
from oracle import wavenet_ref as R
from test_gpu_local_condition import ATOL
from test_gpu_ragged_generation import NINE
from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, WaveNet
from wavenet_amd.graph import default_loss
from wavenet_amd.wavenet import coarse_frames_needed, frames_needed

pytestmark = pytest.mark.gpu

B, T, F, H = LU.B, LU.T, LU.FEATS, LU.HOP
TW = 40
KEY = "local_condition_upsample/W"
FACTORS = [2, 3, 4, 12]                      # H' = 6, 4, 3, 1
INTERPS = ["repeat", "linear"]
PRECS = [None, "fp32"]                      # None: the module default, fp16x2
PER_CLIP = [0, 5, 11]


def _pair(U, interp, cls=WaveNet, over=LR.TINY, W=None, twin=True, seed=1234):
    """(U-model, its U = 1 twin at hop H / U holding the same shared weights, the layer's weight (U F, 2 F))."""
    p = R.make_params(**over)
    sd = LR.state_dict(R.init_weights(p, seed), LR.init_local(p)[0])
    W = LU.random_weight(U, F) if W is None else W
    up = cls(Params(p), seed=0, local_channels=F, local_hop=H, local_interp=interp, local_upsample=U)
    up.load_state_dict(dict(sd, **{KEY: W.reshape(U * F, 2 * F, 1, 1)}))
    up.to_gpu()
    tw = None
    if twin:
        tw = cls(Params(p), seed=0, local_channels=F, local_hop=H // U, local_interp=interp)
        tw.load_state_dict(sd)
        tw.to_gpu()
    return up, tw, W


_DATA = {}


def _data():
    if not _DATA:
        rs = np.random.RandomState(8)
        _DATA.update(idx=dev(rs.randint(0, 256, (B, T)).astype(np.int32)), tgt=dev(rs.randint(0, 256, (B, TW)).astype(np.int32)),
                     h=rs.standard_normal((B, F, 12)).astype(np.float32))
    return _DATA


def _need(U, phase, interp, Tn=T):
    return LU.coarse_needed(Tn, H, U, None if isinstance(phase, list) else phase, interp)


def _cut(y, U, phase, interp, Tn=T):
    """The alignment rule on fine features y (B, F, m): -> (the twin's features, its phase)."""
    fine = H // U
    if not isinstance(phase, list):
        _, c0, ph = LU.alignment(H, U, phase)
        nf = LU.fine_needed(Tn, fine, ph, interp)
        assert c0 + nf <= y.shape[2]
        return y[:, :, c0:c0 + nf].contiguous(), ph
    nf = LU.fine_needed(Tn, fine, fine - 1, interp)
    assert U - 1 + nf <= y.shape[2]
    return torch.stack([y[b, :, p // fine:p // fine + nf] for b, p in enumerate(phase)]).contiguous(), [p % fine for p in phase]


def _step(net, feats, phase, prec):
    """One forward and backward: (loss, out, skip, every layer's input, logits, the gradient arena), detached copies."""
    d = _data()
    net.gemm_precision = prec
    c = net.forward_causal_block(d["idx"])
    out, s = net.forward_residual_block(c, t_off=T - TW, local=feats, local_phase=phase)
    xs = [t.detach().clone() for t in net._last_layer_inputs]
    lg = net.forward_softmax_block(s, apply_softmax=False)
    loss = net.cross_entropy(lg, d["tgt"])
    net.zero_grads()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), out.detach().clone(), s.detach().clone(), xs, lg.detach().clone(), net._grad_arena.clone()


# ---- 1. the reduction, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("interp", INTERPS)
@pytest.mark.parametrize("U", FACTORS)
def test_a_u_model_is_the_twin_at_the_fine_hop_fed_the_upsampled_features(U, interp, prec):
    """Int phases 0 and 5 and the phases [0, 5, 11]: loss, residual output, skip sum, every layer's input, logits and the
    gradient of every shared tensor -- the projection's included -- are the twin's, bit for bit."""
    up, tw, _ = _pair(U, interp)
    up.gemm_precision = tw.gemm_precision = prec
    n_shared = tw._arena.numel()
    assert up._arena.numel() > n_shared and up._spans[-1][0].name == "local_condition_upsample"
    for phase in (0, 5, PER_CLIP):
        h = dev(_data()["h"][:, :, :_need(U, phase, interp)])
        with torch.no_grad():
            y = up.upsampled_features(h)
        assert tuple(y.shape) == (B, F, (h.shape[2] - 1) * U)
        ft, ph = _cut(y, U, phase, interp)
        a = _step(up, h, phase, prec)
        b = _step(tw, ft, ph, prec)
        assert torch.equal(a[0], b[0]) and np.isfinite(float(a[0])), (phase, float(a[0]), float(b[0]))
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[4], b[4]), phase
        assert len(a[3]) == len(b[3]) == 6 and all(torch.equal(x, y_) for x, y_ in zip(a[3], b[3])), phase
        assert torch.equal(a[5][:n_shared], b[5]), phase
        v = [s for s in up._spans if s[0].name == "local_condition_projection"][0]
        assert float(a[5][v[2]:v[2] + v[3]].abs().max()) > 1e-6             # (the projection's gradient is there)
        assert float(a[5][n_shared:].abs().max()) > 1e-7                    # ... and so is the layer's
        # surplus coarse columns are ignored
        more = _step(up, dev(_data()["h"]), phase, prec)
        assert torch.equal(more[0], a[0]) and torch.equal(more[5], a[5]), phase


# ---- 2. the layer against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("U", FACTORS)
def test_the_layer_against_the_float64_restatement(U, prec):
    up, _, W = _pair(U, "repeat", twin=False)
    up.gemm_precision = prec
    h = _data()["h"][:, :, :9]
    got = to_np(up.upsampled_features(h))
    want = LU.upsample(W, h)
    assert got.shape == want.shape == (B, F, 8 * U)
    err = np.abs(got - want).max()
    print("U = %d, %s: max |y - float64| = %.3g of %.3g" % (U, prec, err, np.abs(want).max()))
    assert np.abs(want).max() > 0.5 and err <= ATOL
    init = _pair(U, "repeat", W=LU.initial_weight(U, F), twin=False)[0]
    np.testing.assert_allclose(to_np(init.upsampled_features(h)), LU.upsample(LU.initial_weight(U, F), h), atol=ATOL)


# ---- 3. the layer's gradients ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [None, "fp32", "bf16"])
@pytest.mark.parametrize("U,interp,phase", [(3, "repeat", 11), (3, "linear", 5), (4, "linear", PER_CLIP), (12, "repeat", 11),
                                            (2, "repeat", 0)])
def test_the_layers_weight_and_feature_gradients_against_float64(U, interp, phase, prec):
    """W.grad and the coarse features' gradient after one backward against float64 references formed from the fine-feature
    gradient the twin returns through the ``_LocalFn`` hook: the pair-matrix product and the add-back in float64.  2e-4 of the
    tensor's largest entry; bf16: 15 % in the 2-norm (tests/test_gpu_local_interp.py's bars for weight gradients).  Phase 11
    at T = 70 and U = 3: the last fine column read is the LAST column of the last coarse pair."""
    up, tw, W = _pair(U, interp)
    n = _need(U, phase, interp)
    if (U, phase) == (3, 11):
        fine, c0, ph = LU.alignment(H, U, phase)
        assert (c0 + LU.fine_needed(T, fine, ph, interp) - 1) == (n - 1) * U - 1
    h_np = _data()["h"][:, :, :n]
    h = dev(h_np).requires_grad_(True)
    _step(up, h, phase, prec)
    with torch.no_grad():
        y = up.upsampled_features(dev(h_np))
    ft, ph = _cut(y, U, phase, interp)
    ft = ft.clone().requires_grad_(True)
    _step(tw, ft, ph, prec)
    dcut = to_np(ft.grad).astype(np.float64)
    dy = np.zeros((B, F, (n - 1) * U))
    fine = H // U
    for b in range(B):
        c0 = (phase[b] if isinstance(phase, list) else phase) // fine
        dy[b, :, c0:c0 + dcut.shape[2]] = dcut[b]
    dW, dh = LU.upsample_grads(W, h_np, dy)
    span = up._spans[-1]
    got_W = to_np(up._grad_arena[span[2]:span[2] + span[3]]).reshape(U * F, 2 * F)
    for what, got, want in (("W", got_W, dW), ("h", to_np(h.grad), dh)):
        scale = np.abs(want).max()
        err = np.abs(got - want).max()
        rel = np.linalg.norm(got - want) / (np.linalg.norm(want) + 1e-30)
        print("U = %d, %s, phase %s, %s: d%s max err %.3g of %.3g, 2-norm %.3g" % (U, interp, phase, prec, what, err, scale, rel))
        assert scale > 1e-5
        if prec == "bf16":
            assert rel < 0.15, (what, rel)
        else:
            assert err <= 2e-4 * scale + 1e-7, (what, err, scale)


# ---- 4. the replayed step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phases", [(PER_CLIP, [7, 0, 3], [11, 11, 1]), (5, 5, 5)])
def test_train_step_graph_replays_the_eager_step_bit_for_bit(phases):
    """Captured with U = 3 (linear mode) and a phase per clip, replayed with two other phase vectors and other features -- and
    captured with an int phase: the loss and the whole gradient arena equal the eager step's from the same weights."""
    eager, _, _ = _pair(3, "linear", twin=False)
    net, _, _ = _pair(3, "linear", twin=False)
    rs = np.random.RandomState(0)
    iw = eager.input_width
    per_clip = isinstance(phases[0], list)
    nf = coarse_frames_needed(T, H, 3, None if per_clip else phases[0], "linear")
    batches = [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, T - iw)).astype(np.int32)),
                dev(rs.standard_normal((B, F, nf)).astype(np.float32))) for _ in range(3)]
    w0 = net._arena.clone()
    g = TrainStepGraph(net, batches[0][0], batches[0][1], local=batches[0][2], local_phase=phases[0])
    assert torch.equal(net._arena, w0)
    seen = []
    for (x, tg, ft), ph in zip(batches, phases):
        with torch.no_grad():
            net._arena.copy_(w0)
            eager._arena.copy_(w0)
        loss_e = default_loss(eager, x, tg, local=ft, local_phase=ph)
        eager.backprop(loss_e)
        loss_g = g.step(x, tg, local=ft, local_phase=ph)
        torch.cuda.synchronize()
        assert torch.equal(loss_g, loss_e.detach()), (ph, float(loss_g), float(loss_e))
        assert torch.equal(net._grad_arena, eager._grad_arena), ph
        assert float(net._grad_arena[-eager._spans[-1][3]:].abs().max()) > 1e-7
        seen.append(float(loss_g))
    assert len(set(seen)) == 3
    if per_clip:
        assert g.local_phase.hop == H and g.local_phase.tab.tolist() == phases[2]         # one buffer, refilled, in [0, H)
    else:
        with pytest.raises(Exception, match="captured with phase 5"):
            g.step(*batches[0][:2], local=batches[0][2], local_phase=0)


def test_the_weight_average_covers_the_layer():
    """``enable_ema`` plus one replayed step: the averaged arena's last tensor -- the layer's weight -- moves, and the
    ``ema_weights()`` swap carries it."""
    net, _, W = _pair(3, "linear", twin=False)
    net.enable_ema(0.5, warmup=False)
    net.update_laerning_rate(0.01)
    d = _data()
    n = coarse_frames_needed(T, H, 3, None, "linear")
    tg = dev(np.random.RandomState(1).randint(0, 256, (B, T - net.input_width)).astype(np.int32))
    g = TrainStepGraph(net, d["idx"], tg, local=dev(d["h"][:, :, :n]), local_phase=PER_CLIP)
    span = net._spans[-1]
    assert span[0].name == "local_condition_upsample" and span[2] + span[3] <= net._arena.numel()
    last = lambda a: a[span[2]:span[2] + span[3]]
    w_start = torch.from_numpy(W.reshape(-1))
    assert torch.equal(last(net._ema_arena).cpu(), w_start)
    g.step()
    torch.cuda.synchronize()
    assert float((last(net._arena).cpu() - w_start).abs().max()) > 1e-4
    moved = float((last(net._ema_arena).cpu() - w_start).abs().max())
    assert moved > 1e-5, moved
    with net.ema_weights():
        assert np.array_equal(net.state_dict()[KEY].reshape(-1), to_np(last(net._arena)))
        assert np.isfinite(float(default_loss(net, d["idx"], tg, local=dev(d["h"]), local_phase=PER_CLIP).detach()))


# ---- 5. the decoders ---------------------------------------------------------------------------------------------------------
def _twin_features(up, h, phase, U):
    """One utterance: (F, n) coarse features -> the twin's (F, m - c0) fine features and phase."""
    with torch.no_grad():
        y = up.upsampled_features(dev(h[None]))[0]
    fine = H // U
    return y[:, phase // fine:].contiguous(), phase % fine


@pytest.mark.parametrize("over,interp", [(LR.TINY, "linear"), (LR.TINY, "repeat"), (NINE, "linear")], ids=["tiny-linear", "tiny-repeat", "nine"])
def test_decoders_equal_the_twin_at_the_fine_hop(over, interp):
    """``generate`` (40 samples, return_chosen) and ``generate_batch`` (three utterances of different phases and lengths) with
    U = 3: tokens and ``chosen`` are the twin's at hop 4 given the upsampled features, bit for bit -- on the two-block TINY
    model and on config 4's shape at 2 x 5 layers, where the specialised decoder kernels see hop 4."""
    U = 3
    up, tw, _ = _pair(U, interp, cls=FasterWaveNet, over=over)
    if over is NINE:
        from wavenet_amd import _lib
        assert up._nine_workgroup_shape(_lib.default_exec_flags()) and tw._nine_workgroup_shape(_lib.default_exec_flags())
    W = up.input_width
    rs = np.random.RandomState(3)
    win = rs.randint(0, 256, (3, W)).astype(np.int32)
    lens, phases = [40, 25, 33], [5, 0, 11]
    hs = [rs.standard_normal((F, coarse_frames_needed(W + n - 1, H, U, ph, interp))).astype(np.float32) for n, ph in zip(lens, phases)]
    us = [rs.random_sample(n) for n in lens]
    tok, ch = up.generate(40, us[0], initial_tokens=win[0], local=hs[0], local_phase=phases[0], return_chosen=True)
    ft, ph = _twin_features(up, hs[0], phases[0], U)
    tok2, ch2 = tw.generate(40, us[0], initial_tokens=win[0], local=ft, local_phase=ph, return_chosen=True)
    assert torch.equal(tok, tok2) and torch.equal(ch, ch2)
    assert len(set(tok.tolist())) > 5 and float(ch.min()) > 0
    twins = [_twin_features(up, h, p, U) for h, p in zip(hs, phases)]
    toks, chs = up.generate_batch(lens, us, initial_tokens=win, local=hs, local_phase=phases, return_chosen=True)
    toks2, chs2 = tw.generate_batch(lens, us, initial_tokens=win, local=[t[0] for t in twins], local_phase=[t[1] for t in twins],
                                    return_chosen=True)
    for k in range(3):
        assert toks[k].shape[0] == lens[k] and torch.equal(toks[k], toks2[k]) and torch.equal(chs[k], chs2[k]), k
    assert torch.equal(toks[0], tok) and torch.equal(chs[0], ch)
    # the table holds one row per fine column
    assert tuple(up.local_biases(hs[0]).shape) == ((hs[0].shape[1] - 1) * U, up._cond_rows)


# ---- 6. too few columns ------------------------------------------------------------------------------------------------------
def test_one_coarse_column_short_raises_before_any_launch():
    up, _, _ = _pair(3, "linear", cls=FasterWaveNet, twin=False)
    d = _data()
    c = up.forward_causal_block(d["idx"])
    for phase in (5, PER_CLIP):
        n = coarse_frames_needed(T, H, 3, None if isinstance(phase, list) else phase, "linear")
        up.forward_residual_block(c, local=dev(d["h"][:, :, :n]), local_phase=phase)
        up._last_layer_inputs = None
        with pytest.raises(Exception, match="holds %d feature columns.*takes %d" % (n - 1, n)):
            up.forward_residual_block(c, local=dev(d["h"][:, :, :n - 1]), local_phase=phase)
        assert up._last_layer_inputs is None                                   # nothing ran
    W = up.input_width
    n = coarse_frames_needed(W + 39, H, 3, 11, "linear")
    h = np.random.RandomState(4).standard_normal((F, n)).astype(np.float32)
    u = np.random.RandomState(5).random_sample(40)
    up.prev_causal_outputs = "untouched"
    with pytest.raises(Exception, match="cover fewer samples.*holds %d feature columns.*takes %d" % (n - 1, n)):
        up.generate(40, u, local=h[:, :n - 1], local_phase=11)
    assert up.prev_causal_outputs == "untouched"
    assert up.generate(40, u, local=h, local_phase=11).shape[0] == 40


# ---- 7. scoring and the command line ---------------------------------------------------------------------------------------------
def test_scoring_with_the_layer():
    """The mean of token_nll is the training loss of the same window (1e-5 relative), and score() does not change with
    batch_size or with a chunk_width of another multiple of the hop beyond rounding in exact arithmetic -- the bars of
    test_locally_conditioned_scoring; one coarse column short raises before any work."""
    up, _, _ = _pair(3, "linear", twin=False)
    d = _data()
    n = coarse_frames_needed(T, H, 3, 5, "linear")
    ft = dev(d["h"][:, :, :n])
    want = float(default_loss(up, d["idx"], d["tgt"], local=ft, local_phase=5).detach())
    rows = up.token_nll(d["idx"], d["tgt"], local=ft, local_phase=5)
    assert abs(float(to_np(rows).astype(np.float64).mean()) - want) <= 1e-5 * abs(want)
    rs = np.random.RandomState(51)
    toks = rs.randint(0, 256, (200,)).astype(np.int32)
    n = coarse_frames_needed(200, H, 3, 0, "linear")
    assert n == 18                                                             # 51 fine columns (50 + 1 linear): 17 pairs
    f = rs.standard_normal((F, n)).astype(np.float32)
    up.gemm_precision = "fp32"
    a = up.score(toks, chunk_width=48, batch_size=2, local=f)
    b = up.score(toks, chunk_width=96, batch_size=8, local=f)
    c = up.score(toks, chunk_width=204, batch_size=1, local=f)                 # one piece
    assert a.shape == (200,)
    assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()) and float((a - c).abs().max()) <= 1e-5 * float(a.abs().max())
    assert float((a - up.score(toks, chunk_width=48, batch_size=2, local=-f)).abs().max()) > 1e-3
    with pytest.raises(Exception, match="holds 17 feature columns.*takes 18"):
        up.score(toks, chunk_width=48, local=f[:, :17])
    with pytest.raises(Exception, match="chunk_width % local_hop == 0"):
        up.score(toks, chunk_width=52, local=f)                                # a multiple of H' = 4, not of H


def test_cli_train_generate_evaluate_with_local_upsample(tmp_path):
    """wavs -> features -> ``train --local-upsample 4`` (replayed steps, then resumed op by op on sample-aligned crops) ->
    generation from features (batched decoder and host loop) -> scores, at hop 64 (H' = 16)."""
    import json
    from scipy.io import wavfile
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import features as cli_features
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import local as cli_local
    from wavenet_amd.train_audio import train as cli_train
    wav, feat, model = tmp_path / "wav", tmp_path / "feat", tmp_path / "model"
    wav.mkdir()
    model.mkdir()
    sr = 8000
    t = np.arange(sr // 2) / sr
    for name, hz in (("a.wav", 220), ("b.wav", 330)):
        wavfile.write(str(wav / name), sr, (0.5 * np.sin(2 * np.pi * hz * t) * 32767).astype(np.int16))
    cli_features.main(["-w", str(wav), "-o", str(feat), "--hop", "64", "--mels", "12", "--win", "256"])
    fa = np.load(str(feat / "a.npy"))
    cfg = {"quantization_steps": 256, "sampling_rate": sr, "causal_conv_channels": [32], "residual_conv_channels": [32] * 4,
           "residual_num_blocks": 2, "softmax_conv_channels": [64, 256], "optimizer": "adam"}
    (model / "wavenet.json").write_text(json.dumps(cfg))
    common = ["-w", str(wav), "-m", str(model), "--seed", "1"]
    loop = ["--lr", "0.003", "--batch-size", "4", "--train-width", "256", "--repeat", "15", "--max-epoch", "2"]
    l1 = cli_train.main(common + loop + ["--local-dir", str(feat), "--local-hop", "64", "--local-interp", "linear",
                                         "--local-upsample", "4"])
    assert json.loads((model / "local.json").read_text()) == {"channels": 12, "hop": 64, "interp": "linear", "upsample": 4}
    with np.load(str(model / "wavenet.model.npz")) as z:
        assert list(z.files)[-1] == KEY and z[KEY].shape == (48, 24, 1, 1)
        assert np.abs(z[KEY].reshape(48, 24) - LU.initial_weight(4, 12)).max() > 1e-4
    l2 = cli_train.main(common + loop + ["--local-dir", str(feat), "--no-graph", "--local-crop", "sample"])     # resumed: U from local.json
    assert np.isfinite(l1) and np.isfinite(l2) and l2 < l1, (l1, l2)
    with pytest.raises(SystemExit, match="same value"):
        cli_train.main(common + loop + ["--local-dir", str(feat), "--local-upsample", "2"])
    out = str(tmp_path / "gen")
    short = str(tmp_path / "short.npy")
    np.save(short, fa[:, :4])
    fn, one = cli_generate.main(["-m", str(model), "-o", out, "--fast", "--seed", "2", "--local", short])
    assert one.shape == (4 * 64 - 32 + 1,) and one.min() >= 0 and one.max() < 256       # n columns still give n * hop samples
    fns, tokens = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.02", "--fast", "--seed", "2", "--utterances", "2",
                                     "--local", short, "--local", str(feat / "b.npy")])
    assert len(fns) == 2 and tokens.shape == (2, int(sr * 0.02) - 1)
    fn2, slow = cli_generate.main(["-m", str(model), "-o", out, "-s", "0.003", "--seed", "2", "--local", short])
    assert slow.shape == (int(sr * 0.003) - 1,) and slow[0] == one[0]
    with pytest.raises(SystemExit, match="the features cover"):
        cli_generate.main(["-m", str(model), "-o", out, "-s", "0.5", "--fast", "--local", short])
    table = cli_evaluate.main(["-w", str(wav), "-m", str(model), "--local-dir", str(feat)])
    assert [r["file"] for r in table["files"]] == ["a.wav", "b.wav"]
    assert all(np.isfinite(r["nats_per_sample"]) and r["samples"] > 0 for r in table["files"])
