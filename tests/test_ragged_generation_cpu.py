"""A length per utterance without a GPU: the descriptor field in the header and the binding, the function that deals
utterances to launches, the argument errors of ``generate_batch``'s sequence form (raised before any device work, so on a model
that was never moved to a device), and the argument handling of ``generate --local-dir``."""
import json
import os
import re

import numpy as np
import pytest

import local_cond_ref as LR
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd.faster_wavenet import deal_launches
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the header and the binding ----------------------------------------------------------------------------------------------
def test_header_and_binding_declare_step_limit_ahead_of_the_local_conditioning_group():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    body = re.search(r"typedef struct WnDecoderDesc \{(.*?)\} WnDecoderDesc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
              for part in decl.strip().split(",")]
    tail = ["step_limit", "frame_interp", "frame_bias", "n_frames", "frame_hop", "frame_phase", "frame_stride"]
    assert fields[-7:] == tail
    assert [f[0] for f in _lib.WnDecoderDesc._fields_][-7:] == tail
    assert fields == [f[0] for f in _lib.WnDecoderDesc._fields_]
    assert _lib.WnDecoderDesc().step_limit == 0
    assert re.findall(r"^#define\s+WN_ABI_VERSION\s+(\d+)", hdr, flags=re.M) == ["5"]
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))) == 69
    assert len(re.findall(r"^#define\s+WN_EXEC_\w+\s+\d+u", hdr, flags=re.M)) == 6


# ---- dealing utterances to launches --------------------------------------------------------------------------------------------
def _check_deal(lengths, limit, want):
    got = deal_launches(lengths, limit)
    assert got == want
    # every utterance once, no launch over the limit, a launch's n its longest utterance's, handles longest first
    assert sorted(i for _, idx in got for i in idx) == list(range(len(lengths)))
    restored = [None] * len(lengths)
    for n, idx in got:
        assert 1 <= len(idx) <= limit
        assert n == max(lengths[i] for i in idx) == lengths[idx[0]]
        assert [lengths[i] for i in idx] == sorted((lengths[i] for i in idx), reverse=True)
        for i in idx:
            restored[i] = lengths[i]                                  # a result written back by index is in the caller's order
    assert restored == list(lengths)
    # launches are longest first as a whole
    assert [n for n, _ in got] == sorted((n for n, _ in got), reverse=True)


def test_dealing_sorts_longest_first_keeps_the_order_of_equals_and_cuts_at_the_limit():
    lengths = [5, 40, 3, 40, 17]
    _check_deal(lengths, 2, [(40, [1, 3]), (17, [4, 0]), (3, [2])])
    _check_deal(lengths, 1, [(40, [1]), (40, [3]), (17, [4]), (5, [0]), (3, [2])])
    _check_deal(lengths, 5, [(40, [1, 3, 4, 0, 2])])
    _check_deal(lengths, 1024, [(40, [1, 3, 4, 0, 2])])
    # equal lengths: the caller's order, cut into runs of `limit` -- the launches of the int call
    _check_deal([9] * 7, 3, [(9, [0, 1, 2]), (9, [3, 4, 5]), (9, [6])])
    assert deal_launches([], 4) == []
    with pytest.raises(ValueError):
        deal_launches([3], 0)


# ---- generate_batch: the sequence form's argument errors -----------------------------------------------------------------------
def test_ragged_argument_errors_name_the_utterance_before_any_device_work():
    p = R.make_params(**LR.TINY)
    net = FasterWaveNet(Params(p), seed=0)                                # never moved to a device
    u = np.random.RandomState(1).random_sample((3, 12))
    with pytest.raises(Exception, match=r"2 lengths for 3 utterances \(utterance 2"):
        net.generate_batch([4, 5], u)
    with pytest.raises(Exception, match=r"4 lengths for 3 utterances \(utterance 3"):
        net.generate_batch([4, 5, 6, 7], u)
    for bad in (0, -3, 2.5, "7", True):
        with pytest.raises(Exception, match="utterance 1 must be a positive integer"):
            net.generate_batch([4, bad, 6], u)
    with pytest.raises(Exception, match="utterance 2 has 12 uniforms for its 13 samples"):
        net.generate_batch([4, 12, 13], u)
    with pytest.raises(Exception, match="utterance 1 has 3 uniforms for its 5 samples"):
        net.generate_batch([4, 5, 6], [u[0], u[1, :3], u[2]])
    # features that do not cover an utterance: the check runs per utterance, with that utterance's own length
    hop = 5
    loc = FasterWaveNet(Params(p), seed=0, local_channels=LR.FEATS, local_hop=hop)
    W = loc.input_width
    h = np.random.RandomState(2).standard_normal((LR.FEATS, LR.frames_needed(W + 7 - 1, hop))).astype(np.float32)
    covered = h.shape[1] * hop - W + 1                                    # samples these columns cover
    assert 7 <= covered < 12
    with pytest.raises(Exception, match=r"utterance 2: generate_batch: the features cover fewer samples"):
        loc.generate_batch([3, covered, covered + 1], u, local=h)
    with pytest.raises(Exception, match=r"utterance 1: generate_batch: the features cover fewer samples"):
        loc.generate_batch([3, 12, 12], u, local=[h, h[:, :-1], h[:, :-1]])
    # the int call keeps its own messages
    with pytest.raises(Exception, match=r"^uniforms must be \(N, >= n_samples\)$"):
        net.generate_batch(13, u)
    with pytest.raises(Exception, match="^generate_batch: the features cover fewer samples"):
        loc.generate_batch(12, u, local=h)


# ---- generate --local-dir: argument handling -----------------------------------------------------------------------------------
def test_generate_local_dir_argument_handling(tmp_path):
    with pytest.raises(SystemExit):                                       # mutually exclusive with --local
        cli_args.parse(["--fast", "--local-dir", "feat", "--local", "a.npy"])
    a = cli_args.parse(["--fast", "--local-dir", "feat"])
    assert a.local_dir == "feat" and a.local is None and a.fast
    model, feat, empty = tmp_path / "m", tmp_path / "feat", tmp_path / "empty"
    for d in (model, feat, empty):
        d.mkdir()
    (model / "wavenet.json").write_text(json.dumps(dict(LR.TINY, sampling_rate=8192)))
    np.save(str(feat / "a.npy"), np.zeros((5, 40), np.float32))
    (empty / "notes.txt").write_text("no features here")
    common = ["-g", "-1", "-m", str(model), "-o", str(tmp_path / "out")]
    # every one of these stops before the model is built (-g -1 would stop the build with another message)
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(common + ["--local-dir", str(feat)])
    with pytest.raises(SystemExit, match="not locally conditioned"):      # no local.json
        cli_generate.main(common + ["--fast", "--local-dir", str(feat)])
    (model / "local.json").write_text(json.dumps({"channels": 5, "hop": 12}))
    with pytest.raises(SystemExit, match="no .npy feature file"):
        cli_generate.main(common + ["--fast", "--local-dir", str(empty)])
    with pytest.raises(SystemExit, match="--speaker do not go with it"):
        cli_generate.main(common + ["--fast", "--local-dir", str(feat), "--utterances", "2"])
    np.save(str(feat / "b.npy"), np.zeros((5, 1), np.float32))            # 12 samples of features: shorter than the window
    with pytest.raises(SystemExit, match=r"b\.npy cover 12 samples, fewer than the 16 of the window"):
        cli_generate.main(common + ["--fast", "--local-dir", str(feat)])
    os.remove(str(feat / "b.npy"))
    # what the job is, without a model: names sorted, a length per file (-s caps it), linear mode's extra column
    np.save(str(feat / "0_short.npy"), np.zeros((5, 2), np.float32))
    args = cli_args.parse(common + ["--fast", "--local-dir", str(feat)])
    names, feats, lengths, cids = cli_generate.directory_job(args, False)
    assert names == ["0_short", "a"] and lengths == [2 * 12 - 16 + 1, 40 * 12 - 16 + 1] and cids is None
    assert [f.shape for f in feats] == [(5, 2), (5, 40)]
    args = cli_args.parse(common + ["--fast", "--local-dir", str(feat), "-s", "0.0078125"])  # 1 / 128 s at 8,192 Hz: 63 samples
    assert cli_generate.directory_job(args, True)[2] == [9, 63]
    (model / "local.json").write_text(json.dumps({"channels": 5, "hop": 12, "interp": "linear"}))
    names, feats, lengths, cids = cli_generate.directory_job(args, False)
    assert [f.shape for f in feats] == [(5, 3), (5, 41)] and lengths == [9, 465]
    # a speaker-conditioned checkpoint labels every file by its name; an unknown label stops with the existing message
    (model / "speakers.json").write_text(json.dumps({"speakers": ["a", "p225"], "condition_channels": 4}))
    with pytest.raises(SystemExit, match="unknown speaker '0'"):
        cli_generate.directory_job(args, False)
    os.remove(str(feat / "0_short.npy"))
    np.save(str(feat / "p225_001.npy"), np.zeros((5, 3), np.float32))
    assert cli_generate.directory_job(args, False)[3] == [0, 1]
