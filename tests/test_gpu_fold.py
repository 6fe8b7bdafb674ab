"""GPU: folded decoding -- one utterance as overlapping segments of ONE ``generate_batch`` call, joined on the device.

Everything here is equality.  A segment of ``generate_folded`` is an utterance of a ragged batched call, so its row must be what
``generate()`` gives for that segment alone -- its slice of the utterance's uniforms, its columns and phase, the utterance's window
where it starts at 0 and silence elsewhere -- tokens and ``chosen``, bit for bit; the uniforms are keyed by position, so segment 0
is the start of the sequential chain and a plan of one segment is ``generate()``; and the device's unfold is ``fold.unfold``.

Shapes: two utterances of 83 and 200 samples, body 37, overlap 8, phase 3, warm-up 11 and -- clamping segment 1's warm-up, which
then takes the utterance's own window -- 50."""
import json

import numpy as np
import pytest
import torch

from gpu_util import to_np
from test_gpu_copy_synthesis import HOP as CS_HOP, RATE as CS_RATE, WIN as CS_WIN, setup          # noqa: F401  (the fixture)
from test_gpu_ragged_generation import NINE, spy
from wavenet_amd import FasterWaveNet, Params, _lib, data, fold, metrics, sampling
from wavenet_amd.faster_wavenet import silence_window
from wavenet_amd.wavenet import coarse_frames_needed

pytestmark = pytest.mark.gpu

Q, FEATS = 256, 5
# the any-shape decoder: 2 x 3 layers, 8 / 8 / 16 channels
TINY = dict(quantization_steps=Q, causal_conv_channels=[8], residual_conv_channels=[8] * 3, residual_num_blocks=2,
            softmax_conv_channels=[16, Q])
LENGTHS, BODY, OVERLAP, PHASE = [83, 200], 37, 8, 3
MODELS = {                                  # name: (shape, constructor keywords)
    "repeat": (TINY, dict(local_hop=5)),
    "linear": (TINY, dict(local_hop=5, local_interp="linear")),
    "hop6-U2": (TINY, dict(local_hop=6, local_upsample=2)),
    "speaker": (TINY, dict(local_hop=5, condition_classes=3, condition_channels=4)),
    "config4": (NINE, dict(local_hop=5)),
}
_NETS, _RUNS = {}, {}


def _net(name):
    """The model of a case, built once: seeded weights, the conditioning weights drawn anew so that none of them is a start value."""
    if name not in _NETS:
        shape, kw = MODELS[name]
        net = FasterWaveNet(Params(shape), seed=1234, local_channels=FEATS, **kw)
        rs = np.random.RandomState(7)
        sd = net.state_dict()
        for k in sorted(sd):
            if "condition" in k:
                sd[k] = (0.5 * rs.standard_normal(np.shape(sd[k]))).astype(np.float32)
        net.load_state_dict(sd)
        net.to_gpu()
        assert net._nine_workgroup_shape(_lib.default_exec_flags()) == (name == "config4")
        _NETS[name] = net
    return _NETS[name]


def _inputs(net, name):
    rs = np.random.RandomState(5)
    W = net.input_width
    prompts = rs.randint(0, Q, (2, W)).astype(np.int32)
    us = [rs.random_sample(n) for n in LENGTHS]
    hs = [rs.standard_normal((FEATS, coarse_frames_needed(W + n - 1, net.local_hop, net.local_upsample, PHASE, net.local_interp)))
          .astype(np.float32) for n in LENGTHS]                     # exactly what generate(n, ...) itself asks for
    kw = dict(temperature=[1.0, 0.8], top_k=[0, 20], top_p=[1.0, 0.9])
    if name == "speaker":
        kw["condition"] = [2, 0]
    return prompts, us, hs, kw


def _one(kw, i):
    return {k: v[i] for k, v in kw.items()}


def _run(name, warmup):
    """The folded call of a case and the whole-utterance ``generate`` calls it is held against, computed once and not changed."""
    if (name, warmup) not in _RUNS:
        net = _net(name)
        prompts, us, hs, kw = _inputs(net, name)
        with spy(net) as s:
            pcm, chosen, segs = net.generate_folded(LENGTHS, us, BODY, OVERLAP, warmup, initial_tokens=prompts, local=hs,
                                                    local_phase=PHASE, return_chosen=True, return_segments=True, **kw)
        assert s.calls == 0                                             # one batched call, not a loop over generate()
        whole = [net.generate(LENGTHS[i], us[i], initial_tokens=prompts[i], local=hs[i], local_phase=PHASE, **_one(kw, i))
                 for i in range(2)]
        _RUNS[(name, warmup)] = (pcm, chosen, segs, whole)
    return _RUNS[(name, warmup)]


CASES = [(m, w) for m in MODELS for w in (11, 50)]


@pytest.mark.parametrize("name,warmup", CASES)
def test_every_segment_is_its_own_generate_call(name, warmup):
    net = _net(name)
    prompts, us, hs, kw = _inputs(net, name)
    pcm, chosen, segs, _ = _run(name, warmup)
    W, silence = net.input_width, silence_window(Q, net.input_width)
    for i, (plan, rows, ch) in enumerate(segs):
        assert plan == fold.fold_plan(LENGTHS[i], BODY, OVERLAP, warmup) and len(plan.segments) == (3, 6)[i]
        if warmup == 50:
            assert plan.segments[1].s == 0 and plan.segments[2].s > 0               # the clamp
        for u, g in enumerate(plan.segments):
            first, count, ph = fold.segment_columns(g.s, g.e, W, PHASE, net.local_hop, net.local_interp, net.local_upsample)
            want, want_ch = net.generate(g.e - g.s, us[i][g.s:g.e], initial_tokens=prompts[i] if g.s == 0 else silence,
                                         local=hs[i][:, first:first + count], local_phase=ph, return_chosen=True, **_one(kw, i))
            assert rows[u].dtype == torch.int32 and rows[u].is_cuda and torch.equal(rows[u], want), (i, u)
            assert torch.equal(ch[u], want_ch), (i, u)


@pytest.mark.parametrize("name,warmup", CASES)
def test_segment_0_is_the_chain_and_the_device_unfold_is_the_rule(name, warmup):
    pcm, chosen, segs, whole = _run(name, warmup)
    table = data.pcm_table(Q)
    distinct = 0
    for i, (plan, rows, ch) in enumerate(segs):
        assert torch.equal(rows[0][:BODY], whole[i][:BODY]), i                   # uniforms keyed by position: the chain's start
        host = [to_np(r) for r in rows]
        assert pcm[i].dtype == torch.int16 and pcm[i].is_cuda and pcm[i].shape == (LENGTHS[i],)
        assert np.array_equal(to_np(pcm[i]), fold.unfold(host, plan, table)), i
        assert np.array_equal(to_np(chosen[i]), fold.gather_owner([to_np(c) for c in ch], plan)), i
        distinct += len(plan.segments) - 1 - fold.identical_seams(host, plan)
        own = fold.owner(plan)
        inside = np.ones(LENGTHS[i], bool)
        for g in plan.segments[:-1]:
            inside[g.b:g.b + OVERLAP] = False
        assert np.array_equal(to_np(pcm[i])[inside], table[fold.gather_owner(host, plan)][inside])
        assert own[0] == 0 and own[-1] == len(plan.segments) - 1
    print("%s, warm-up %d: %d of %d seams differ between their two sides" % (name, warmup, distinct, sum(len(s[0].segments) - 1 for s in segs)))


@pytest.mark.parametrize("n,B,O,W", [(83, 37, 8, 11), (200, 37, 8, 50), (64, 8, 8, 0), (4100, 1000, 257, 300), (50, 60, 5, 5), (41, 5, 0, 2)])
def test_the_device_unfold_on_rows_whose_seams_all_differ(n, B, O, W):
    """Random token rows (what decoded segments agree on is the model's business): every seam is a cross-fade of two different
    signals, ties and both rims of the table included, and the device's result is ``fold.unfold``'s, bit for bit."""
    net = _net("repeat")
    table = data.pcm_table(Q)
    plan = fold.fold_plan(n, B, O, W)
    rs = np.random.RandomState(n)
    host = [rs.randint(0, Q, (g.e - g.s,)).astype(np.int32) for g in plan.segments]
    for r in host:
        r[::7], r[3::11] = 0, Q - 1
    want = fold.unfold(host, plan, table)
    got = net._unfold([torch.as_tensor(r).to(net.device) for r in host], plan, table)
    assert got.dtype == torch.int16 and np.array_equal(to_np(got), want)
    assert fold.identical_seams(host, plan) == (len(host) - 1 if O == 0 else 0)
    if len(host) > 1 and O:
        assert not np.array_equal(want, table[fold.gather_owner(host, plan)])


@pytest.mark.parametrize("name", list(MODELS))
def test_a_plan_of_one_segment_is_generate_and_a_tile_changes_nothing(name):
    net = _net(name)
    prompts, us, hs, kw = _inputs(net, name)
    pcm, chosen, segs, whole = _run(name, 11)
    table = torch.as_tensor(data.pcm_table(Q)).to(net.device)
    one, one_ch = net.generate_folded(LENGTHS, us, 200, OVERLAP, 11, initial_tokens=prompts, local=hs, local_phase=PHASE,
                                      return_chosen=True, **kw)
    for i in range(2):
        assert torch.equal(one[i], table[whole[i].long()]), i
        want_ch = net.generate(LENGTHS[i], us[i], initial_tokens=prompts[i], local=hs[i], local_phase=PHASE, return_chosen=True,
                               **_one(kw, i))[1]
        assert torch.equal(one_ch[i], want_ch), i
    # one utterance, the scalar form: the tensors themselves come back
    solo = net.generate_folded(LENGTHS[0], us[0], 83, initial_tokens=prompts[0], local=hs[0], local_phase=PHASE, **_one(kw, 0))
    assert isinstance(solo, torch.Tensor) and torch.equal(solo, one[0])
    tiled = net.generate_folded(LENGTHS, us, BODY, OVERLAP, 11, initial_tokens=prompts, local=hs, local_phase=PHASE, tile=2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(tiled, pcm))
    auto = net.generate_folded(LENGTHS[1], us[1], "auto", 2, 3, initial_tokens=prompts[1], local=hs[1], local_phase=PHASE,
                               return_segments=True, **_one(kw, 1))
    assert auto[1][0].body == fold.auto_body(200, net.fold_capacity(), 2, 3) >= 20


# ---- the command ----------------------------------------------------------------------------------------------------------------------
def test_generate_fold_writes_the_methods_samples_and_without_a_seam_the_plain_commands_bytes(tmp_path):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import generate as cli_generate
    sr, hop = 8000, 5
    net = _net("repeat")
    W = net.input_width
    model = tmp_path / "model"
    model.mkdir()
    net.save(str(model))
    (model / "wavenet.json").write_text(json.dumps(dict(TINY, sampling_rate=sr)))
    (model / "local.json").write_text(json.dumps({"channels": FEATS, "hop": hop}))
    h = np.random.RandomState(3).standard_normal((FEATS, (W + 130) // hop)).astype(np.float32)
    np.save(str(tmp_path / "f.npy"), h)
    n = h.shape[1] * hop - W + 1                                          # what the features cover behind the window
    base = ["-m", str(model), "--fast", "--seed", "2", "--local", str(tmp_path / "f.npy"), "--top-k", "40"]
    plain, tokens = cli_generate.main(base + ["-o", str(tmp_path / "plain")])
    assert tokens.shape == (n,)
    same, signal = cli_generate.main(base + ["-o", str(tmp_path / "same"), "--fold", "1"])             # 8,000 samples >= n: no seam
    assert open(same, "rb").read() == open(plain, "rb").read() and np.array_equal(signal, data.pcm_table(Q)[tokens])
    report = tmp_path / "r.json"
    folded, signal = cli_generate.main(base + ["-o", str(tmp_path / "folded"), "--fold", str(37.0 / sr), "--fold-overlap", str(8.0 / sr),
                                               "--fold-warmup", str(11.0 / sr), "--report", str(report), "--tile", "2"])
    np.random.seed(2)
    u = np.random.random_sample(n)
    want, want_ch, (plan, rows, _) = net.generate_folded(n, u, 37, 8, 11, local=h, top_k=40, return_chosen=True, return_segments=True)
    rate, pcm = wavfile.read(folded)
    assert rate == sr and np.array_equal(pcm[:, 0], to_np(want)) and np.array_equal(pcm[:, 1], pcm[:, 0]) and np.array_equal(signal, pcm[:, 0])
    assert len(plan.segments) == -(-(n - 8) // 37) >= 3 and not np.array_equal(to_np(want), data.pcm_table(Q)[tokens])
    row = json.loads(report.read_text())["files"][0]
    assert row["fold"] == {"segments": len(plan.segments), "body": 37, "overlap": 8, "warmup": 11,
                           "identical_seams": fold.identical_seams([to_np(r) for r in rows], plan)}
    assert row["samples"] == n and row["nats_per_sample"] == sampling.chosen_nll(want_ch)


# ---- reading the cost of a fold ------------------------------------------------------------------------------------------------------------
def test_copy_synthesis_reads_its_figures_off_the_folded_signal_and_evaluate_prints_them(setup):
    """tests/test_gpu_copy_synthesis.py's checkpoint and recordings (684, 644 and 384 samples behind a window of 16; hop 16): bodies
    of 150 samples, the default overlap (one column) and warm-up (the window's width)."""
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    s = setup
    net, W, toks = s["net"], s["W"], s["tokens"]
    np.random.seed(3)
    u = [np.random.random_sample(t.size - W) for t in toks]
    kw = dict(temperature=0.9, top_k=40)
    rows = metrics.copy_synthesis(net, toks, s["feats"], None, u, s["mel"], s["pitch"], fold=(150, None, None), **kw)
    pcm, chosen, segs = net.generate_folded([t.size - W for t in toks], u, 150, initial_tokens=np.stack([t[:W] for t in toks]),
                                            local=list(s["feats"]), return_chosen=True, return_segments=True, **kw)
    table = data.pcm_table(256).astype(np.float32)
    k = metrics.first_free_column(W, CS_WIN, CS_HOP)
    for r, t, p, ch, (plan, seg_rows, _) in zip(rows, toks, pcm, chosen, segs):
        assert np.array_equal(r["emitted"], to_np(p)) and r["samples"] == t.size and r["nats_per_sample"] == sampling.chosen_nll(ch)
        assert r["fold"] == {"segments": -(-(t.size - W - 16) // 150), "body": 150, "overlap": 16, "warmup": 16,
                             "identical_seams": fold.identical_seams([to_np(x) for x in seg_rows], plan)} and r["fold"]["segments"] >= 3
        a, b = s["mel"].batch([table[t] / np.float32(32768.0), np.concatenate([table[t[:W]], to_np(p).astype(np.float32)]) / np.float32(32768.0)])
        assert r["log_mel_distance_db"] == metrics.log_mel_distance(a[:, k:], b[:, k:])[0] > 0.0
    # a plan of one segment is the unfolded run: its tokens' values, its likelihood
    plain = metrics.copy_synthesis(net, toks, s["feats"], None, u, s["mel"], s["pitch"], **kw)
    one = metrics.copy_synthesis(net, toks, s["feats"], None, u, s["mel"], s["pitch"], fold=(10 ** 6, None, None), **kw)
    for a, b in zip(plain, one):
        assert np.array_equal(data.pcm_table(256)[a["emitted"]], b["emitted"]) and a["nats_per_sample"] == b["nats_per_sample"]
        assert b["fold"]["segments"] == 1
    with pytest.raises(ValueError, match="fold= does not go with forced="):
        metrics.copy_synthesis(net, toks, s["feats"], None, u, s["mel"], s["pitch"], fold=(150, None, None), forced=[t[W:] for t in toks])
    got = cli_evaluate.main(["-w", str(s["wav"]), "-m", str(s["model"]), "--copy-synthesis", "--seed", "3", "--fold", str(150.0 / CS_RATE),
                             "--temperature", "0.9", "--top-k", "40"])
    for g, r in zip(got["files"], rows):
        assert g["fold"] == r["fold"] and all(g[key] == r[key] for key in ("log_mel_distance_db", "vuv_error", "nats_per_sample"))
