"""The probability of each emitted token without a GPU: the descriptor flag in the header and the binding (and an ABI that did
not move), ``sampling.chosen_nll`` / ``sampling.pick_best`` on hand-made rows, the command line's refusals, and the row order of
``--best-of`` candidates in the one ``generate_batch`` call."""
import json
import math
import os
import re

import numpy as np
import pytest

from wavenet_amd import Params, _lib, sampling
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate
from wavenet_amd.train_audio.train import input_width_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"residual_conv_channels": [8, 8, 8], "residual_num_blocks": 2, "causal_conv_channels": [8],
         "softmax_conv_channels": [16, 256]}


def _header():
    return open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()


def _fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
            for part in decl.split(",")]


def test_the_header_defines_the_bit_as_256_and_the_binding_agrees():
    hdr = _header()
    assert re.findall(r"^#define\s+WN_DECODER_TRACE_CHOSEN\s+(\d+)u", hdr, flags=re.M) == ["256"]
    assert _lib.WN_DECODER_TRACE_CHOSEN == 256
    # free in both flag words: no other WN_EXEC_* / WN_DECODER_* flag bit has the value
    others = {k: v for k, v in vars(_lib).items() if re.match(r"WN_(EXEC|DECODER)_", k) and k not in
              ("WN_DECODER_TRACE_CHOSEN", "WN_DECODER_BATCH_MAX_ANY")}
    assert others and all(isinstance(v, int) and not (v & 256) for v in others.values()), others


def test_the_abi_did_not_move():
    hdr = _header()
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 69
    assert _lib.ABI_VERSION == 5 == int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1))
    assert _fields(hdr, "WnExec") == [f[0] for f in _lib.WnExec._fields_] == \
        ["precision", "flags", "ws", "ws_bytes", "fwd_t1_min_blocks", "reserved", "plan"]
    assert _fields(hdr, "WnStackDesc") == [f[0] for f in _lib.WnStackDesc._fields_] == \
        ["n_layers", "Cr", "Cs", "fw", "cd", "dilation", "Wf", "bf", "Wg", "bg", "Wp", "bp", "Ws", "bs", "bias_phase_tab",
         "bias_interp", "bias_hop", "bias_phase", "bias_frame_stride"]
    assert _fields(hdr, "WnDecoderDesc") == [f[0] for f in _lib.WnDecoderDesc._fields_] == \
        ["Q", "fw_causal", "n_causal", "fw", "n_blocks", "n_layers", "Cr", "Cs", "n_head", "causal_channels", "cd",
         "head_channels", "causal_W", "causal_b", "Wf", "bf", "Wg", "bg", "Wp", "bp", "Ws", "bs", "head_W", "head_b", "head_act",
         "flags", "step_limit", "frame_interp", "frame_bias", "n_frames", "frame_hop", "frame_phase", "frame_stride"]


def test_chosen_nll_on_hand_made_rows():
    p = np.array([0.5, 0.25, 1.0, 0.125], dtype=np.float32)
    want = (math.log(2.0) + math.log(4.0) + 0.0 + math.log(8.0)) / 4.0
    got = sampling.chosen_nll(p)
    assert isinstance(got, float) and got == want
    # float64 arithmetic on the float32 values: 1 - 2^-24 has a logarithm that float32 arithmetic would round to 0
    tiny = np.array([np.float32(1.0) - np.float32(2.0 ** -24)], dtype=np.float32)
    assert sampling.chosen_nll(tiny) == -math.log(1.0 - 2.0 ** -24) > 0.0
    assert sampling.chosen_nll(np.array([0.5, 0.0, 0.5], dtype=np.float32)) == math.inf        # a 0.0 was drawn
    assert sampling.chosen_nll(np.zeros((0,), np.float32)) == 0.0
    import torch
    assert sampling.chosen_nll(torch.tensor([0.5, 0.25, 1.0, 0.125])) == want


def test_pick_best_on_hand_made_rows():
    assert sampling.pick_best([3.0, 1.5, 2.0]) == 1
    assert sampling.pick_best([2.0, 1.0, 1.0, 4.0]) == 1                   # a tie: the lowest index
    assert sampling.pick_best([math.inf, 5.0]) == 1
    assert sampling.pick_best([math.inf, math.inf]) == 0
    assert sampling.pick_best([math.nan, 7.0, math.nan, 6.0]) == 3         # NaN never wins
    assert sampling.pick_best([math.nan, math.inf]) == 1
    assert sampling.pick_best([4.0]) == 0
    with pytest.raises(ValueError):
        sampling.pick_best([])


def test_the_flags_parse_and_their_absence_changes_nothing():
    a = cli_args.parse([])
    assert a.report is None and a.best_of == 1 and "report" not in vars(a) and "best_of" not in vars(a)
    a = cli_args.parse(["--fast", "--best-of", "4", "--report", "r.json"])
    assert a.best_of == 4 and a.report == "r.json"
    text = cli_args.build_parser().format_help()
    assert "--best-of" in text and "--report" in text and "not a quality score" in " ".join(text.split())


def test_the_command_line_refuses_before_a_model_is_built(tmp_path, monkeypatch):
    def no_model(*a, **kw):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli_generate._model, "build", no_model)
    monkeypatch.setattr(cli_generate._model, "load_params", no_model)
    m = str(tmp_path / "model")
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(["-m", m, "--best-of", "2"])
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(["-m", m, "--report", str(tmp_path / "r.json")])
    with pytest.raises(SystemExit, match="K >= 1, got 0"):
        cli_generate.main(["-m", m, "--fast", "--best-of", "0"])
    with pytest.raises(SystemExit, match="K >= 1, got -3"):
        cli_generate.main(["-m", m, "--best-of", "-3"])
    assert not os.path.exists(m) and not os.path.exists(str(tmp_path / "r.json"))


class _Recorder(object):
    """Stands in for a FasterWaveNet: ``generate_batch`` records its arguments and answers row r with tokens that are all
    ``r`` and probabilities that are all ``probs[r]``."""

    def __init__(self, probs):
        self.probs, self.calls = probs, []

    def generate_batch(self, n_samples, uniforms, **kw):
        self.calls.append((n_samples, np.array(uniforms), kw))
        rows = len(uniforms)
        assert rows == len(self.probs)
        tokens = np.stack([np.full((n_samples,), r, dtype=np.int32) for r in range(rows)])
        chosen = np.stack([np.full((n_samples,), self.probs[r], dtype=np.float32) for r in range(rows)])
        return tokens, chosen

    def generate(self, *a, **kw):
        raise AssertionError("--best-of goes through generate_batch")


def test_best_of_candidates_are_rows_u_times_k_plus_c_of_one_generate_batch_call(tmp_path):
    N, K, n = 2, 3, 7                                   # 8 samples a second for 1 second: n = 8 - 1
    params = Params(SMALL)
    # utterance 0: candidate 2 is the likeliest; utterance 1: candidates 0 and 1 tie, the lower index is kept
    net = _Recorder([0.25, 0.125, 0.5, 0.5, 0.5, 0.25])
    report = str(tmp_path / "report.json")
    np.random.seed(5)
    files, tokens = cli_generate.generate_utterances(net, params, [None] * N, sampling_rate=8, generate_sec=1.0, fast=True,
                                                     output_dir=str(tmp_path / "out"), temperature=0.9, top_k=7, top_p=0.8,
                                                     conditions=[4, 9], best_of=K, report=report)
    assert len(net.calls) == 1                          # all N * K candidates in the same call
    got_n, u, kw = net.calls[0]
    assert got_n == n and u.shape == (N * K, n)
    assert np.array_equal(u, np.random.RandomState(5).random_sample((N * K, n)))
    assert kw["condition"] == [4, 4, 4, 9, 9, 9] and kw["return_chosen"] is True
    assert (kw["temperature"], kw["top_k"], kw["top_p"]) == (0.9, 7, 0.8)
    prompts = np.asarray(kw["initial_tokens"])
    assert prompts.shape == (N * K, input_width_of(params)) and (prompts == 127).all()
    # only the kept candidate is written, under the utterance's name
    assert [os.path.basename(f) for f in files] == ["generated_000.wav", "generated_001.wav"]
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["generated_000.wav", "generated_001.wav"]
    assert tokens.shape == (N, n) and (tokens[0] == 0 * K + 2).all() and (tokens[1] == 1 * K + 0).all()
    table = json.load(open(report))
    ln2, ln4, ln8 = math.log(2.0), math.log(4.0), math.log(8.0)
    assert table["files"] == [
        {"file": "generated_000.wav", "samples": n, "nats_per_sample": ln2, "bits_per_sample": 1.0,
         "candidates": [ln4, ln8, ln2], "kept": 2},
        {"file": "generated_001.wav", "samples": n, "nats_per_sample": ln2, "bits_per_sample": 1.0,
         "candidates": [ln2, ln2, ln4], "kept": 0}]
    assert table["total"] == {"samples": 2 * n, "nats_per_sample": ln2, "bits_per_sample": 1.0}
    for row in table["files"]:
        assert row["kept"] == sampling.pick_best(row["candidates"])


def test_the_single_utterance_mode_with_k_candidates_draws_k_rows_and_goes_through_generate_batch(tmp_path):
    K, n = 2, 7
    net = _Recorder([0.5, 1.0])
    np.random.seed(8)
    fn, tokens = cli_generate.generate_audio(net, Params(SMALL), sampling_rate=8, generate_sec=1.0, fast=True,
                                             output_dir=str(tmp_path / "out"), best_of=K, report=str(tmp_path / "r.json"))
    (got_n, u, kw), = net.calls
    assert got_n == n and np.array_equal(u, np.random.RandomState(8).random_sample((K, n)))
    assert os.path.basename(fn) == "generated.wav" and (tokens == 1).all()
    table = json.load(open(str(tmp_path / "r.json")))
    assert table["files"] == [{"file": "generated.wav", "samples": n, "nats_per_sample": 0.0, "bits_per_sample": 0.0,
                               "candidates": [math.log(2.0), 0.0], "kept": 1}]
