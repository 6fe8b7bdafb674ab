"""The host side of crops across the corpus: the draw rule against the per-file rule, the refusals that need no GPU, the ABI's
names, and the flag."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import corpus_ref as R
from wavenet_amd import Corpus, _corpus, _lib
from wavenet_amd.corpus import columns_per_crop
from wavenet_amd.train_audio.train import _Crops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IW, TW, HOP, F = 9, 16, 16, 3
# hi = len - TW - 1: 17 -> no window; 18 -> exactly one (sample); 26 -> none on a column border (r = 9), 27 -> exactly one;
# 61, 257 and 700 are no multiples of the hop
LENGTHS = [61, 17, 18, 64, 26, 27, 257, 700]


def _files(lengths, q=256, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, q, size=n).astype(np.int32) for n in lengths]


def _features(lengths, surplus=(0, 2), seed=1):
    rs = np.random.RandomState(seed)
    return [rs.randn(F, -(-n // HOP) + surplus[i % len(surplus)]).astype(np.float32) for i, n in enumerate(lengths)]


def _corpus_on_host(lengths=LENGTHS, with_features=True, **kw):
    return Corpus(_files(lengths), IW, 256, "cpu", features=_features(lengths) if with_features else None, hop=HOP, **kw)


class _Every(object):
    """An rng whose one randint call returns every g of [0, total) once."""
    calls = 0

    def randint(self, low, high, size=None):
        assert low == 0 and size == high
        self.calls += 1
        return np.arange(high)


@pytest.mark.parametrize("crop,with_features", [("sample", True), ("frame", True), ("frame", False)])
def test_draw_indices_is_a_bijection_onto_the_starts_the_per_file_rule_allows(crop, with_features):
    c = _corpus_on_host(with_features=with_features)
    per_file = [R.legal_starts(n, IW, TW, HOP if with_features else 0, crop) for n in LENGTHS]
    counts = c.windows(TW, crop)
    assert counts.tolist() == [len(s) for s in per_file]
    assert counts[1] == 0 and (counts[2] == 1 if crop == "sample" or not with_features else counts[4] == 0 and counts[5] == 1)
    total, rng = int(counts.sum()), _Every()
    files, starts = c.draw_indices(total, TW, crop, rng=rng)
    assert rng.calls == 1
    got = list(zip(files.tolist(), starts.tolist()))
    want = [(f, s) for f, ss in enumerate(per_file) for s in ss]
    assert len(set(got)) == len(got) == total and got == want         # every allowed pair exactly once (in file order)
    c.check_draws(files, starts, TW)                                  # ... and gather takes every one of them


def test_a_corpus_without_any_window_refuses_the_draw():
    c = _corpus_on_host([17, 5], with_features=False)
    assert c.windows(TW).tolist() == [0, 0]
    with pytest.raises(Exception, match="too short"):
        c.draw_indices(4, TW)


@pytest.mark.parametrize("crop,interp,U", [("sample", "repeat", 1), ("frame", "repeat", 1), ("sample", "linear", 1),
                                           ("frame", "linear", 4), ("sample", "repeat", 4), (None, None, 1)])
def test_one_file_under_one_seed_draws_the_crops_of_the_per_file_loop(monkeypatch, crop, interp, U):
    """The same np.random.randint call, argument for argument, the same starts, the same column count -- and the crops
    themselves: ``_Crops`` (run on the host here) against the reference at the corpus' starts."""
    from wavenet_amd.train_audio import local as L
    from wavenet_amd.wavenet import coarse_frames_needed
    n, B = 257, 6
    tok, feats = _files([n])[0], _features([n], surplus=(2,))[0]
    calls, real = [], np.random.randint

    def randint(*a, **kw):
        calls.append((a, kw, real(*a, **kw)))
        return calls[-1][2]

    monkeypatch.setattr(np.random, "randint", randint)
    fkw, n_cols = {}, None
    if crop is not None:
        ext, shift = L.padded(L.with_extra_column(feats, interp, U), IW, HOP)
        fkw = dict(features=ext, hop=HOP, shift=shift, extra_column=interp == "linear", crop=crop)
        if U > 1:
            fkw["columns"] = coarse_frames_needed(IW + TW, HOP, U, None if crop == "sample" else 0, interp)
    crops = _Crops(np.concatenate([np.full((IW,), 127, dtype=np.int32), tok]), IW, TW, "cpu", **fkw)
    np.random.seed(11)
    drawn = crops.draw(B)
    c = Corpus([tok], IW, 256, "cpu", features=None if crop is None else [feats], hop=HOP)
    if crop is not None:
        n_cols = columns_per_crop(IW, TW, HOP, crop, interp, U)
        assert n_cols == crops.fcol.numel()
    np.random.seed(11)
    files, starts = c.draw_indices(B, TW, crop or "sample")
    (a0, k0, r0), (a1, k1, r1) = calls
    assert a0 == a1 and k0 == k1 and np.array_equal(r0, r1)            # the very call
    assert files.tolist() == [0] * B
    x, tgt, local, _, phases = R.of_corpus(c, files, starts, TW, n_cols, interp or "repeat", U)
    assert np.array_equal(drawn[0].numpy(), x) and np.array_equal(drawn[1].numpy(), tgt)
    if crop is not None:
        assert np.array_equal(drawn[2].numpy(), local)
        assert np.array_equal(c.phases(starts), phases)
        assert np.array_equal(drawn[3], phases) if crop == "sample" else not phases.any()


def test_gather_refuses_bad_draws_by_crop_before_any_device_work():
    c = _corpus_on_host()
    ok_f, ok_s = np.array([0, 3, 6]), np.array([0, 5, 239])
    for files, starts, word in [([0, 8, 6], ok_s, "crop 1 names file 8"), ([0, -1, 6], ok_s, "crop 1 names file -1"),
                                (ok_f, [0, 5, 240], "crop 2 starts at 240; file 6 allows starts 0 .. 239"),
                                (ok_f, [-1, 5, 2], "crop 0 starts at -1"),
                                ([0, 1, 6], ok_s, "crop 1 names file 1, which is left out: its 17 tokens")]:
        with pytest.raises(ValueError, match=word):
            c.gather(np.asarray(files), np.asarray(starts), TW, 3)
    with pytest.raises(ValueError, match="n_cols = None"):
        c.gather(ok_f, ok_s, TW)
    with pytest.raises(ValueError, match="integer arrays"):
        c.gather(ok_f, ok_s.astype(np.float32), TW, 3)
    assert c.launches == 0
    with pytest.raises(ValueError, match="lives on cpu"):              # (a good draw gets as far as the device, and no further)
        c.gather(ok_f, ok_s, TW, 3)


def test_the_constructor_refuses_what_it_cannot_pack():
    tok = _files([61, 64])
    with pytest.raises(ValueError, match="file 1 holds a token outside"):
        Corpus([tok[0], tok[1] + 200], IW, 256, "cpu")
    with pytest.raises(ValueError, match=r"features of file 1 have shape \(3, 3\); its 64 tokens need \(3, >= 4\)"):
        Corpus(tok, IW, 256, "cpu", features=[np.zeros((F, 4), np.float32), np.zeros((F, 3), np.float32)], hop=HOP)
    with pytest.raises(ValueError, match="1 class ids for 2 files"):
        Corpus(tok, IW, 256, "cpu", classes=[0])
    assert Corpus(tok, IW, 256, "cpu").tokens.dtype == np.uint8 and Corpus(tok, IW, 300, "cpu").tokens.dtype == np.int32
    assert Corpus(tok, IW, 256, "cpu").file_offset.tolist() == [0, 61]


def test_wn_corpus_gather_refuses_null_and_bad_shapes_without_a_gpu():
    lib = _corpus.lib()
    EARG = _corpus.WNC_EARG

    def desc(**kw):
        d = dict(tokens=64, file_offset=64, file_len=64, file_class=None, features=None, col_offset=None, col_count=None,
                 total_cols=0, n_files=2, token_bytes=1, F=0, hop=0, input_width=IW, silence=127, pad_cols=0, shift=0)
        d.update(kw)
        return C.byref(_corpus.WnCorpusDesc(**d))

    feat = dict(features=64, col_offset=64, col_count=64, total_cols=9, F=F, hop=HOP, pad_cols=1, shift=7)
    assert lib.wn_corpus_gather(None, 64, 2, TW, 0, 64, 64, None, None, None) == EARG and b"NULL" in lib.wn_corpus_last_error()
    for args in [(None, 2, TW, 0, 64, 64), (64, 2, TW, 0, None, 64), (64, 2, TW, 0, 64, None)]:
        assert lib.wn_corpus_gather(desc(), *args, None, None, None) == EARG and b"NULL" in lib.wn_corpus_last_error()
    for d, args, word in [(desc(tokens=None), (2, TW, 0), b"NULL tokens"), (desc(file_len=None), (2, TW, 0), b"NULL tokens"),
                          (desc(token_bytes=2), (2, TW, 0), b"token_bytes = 2"), (desc(token_bytes=0), (2, TW, 0), b"token_bytes = 0"),
                          (desc(), (0, TW, 0), b"B = 0"), (desc(), (-3, TW, 0), b"B = -3"), (desc(), (2, 0, 0), b"target_width = 0"),
                          (desc(n_files=0), (2, TW, 0), b"n_files = 0"), (desc(silence=256), (2, TW, 0), b"silence = 256"),
                          (desc(**feat), (2, TW, 0), b"n_cols = 0"), (desc(**feat), (2, TW, -1), b"n_cols = -1"),
                          (desc(**dict(feat, col_count=None)), (2, TW, 3), b"NULL col_offset"),
                          (desc(**dict(feat, hop=0)), (2, TW, 3), b"hop = 0"), (desc(**dict(feat, F=0)), (2, TW, 3), b"F = 0"),
                          (desc(**dict(feat, shift=6)), (2, TW, 3), b"shift = 6")]:
        assert lib.wn_corpus_gather(d, 64, *args, 64, 64, 64, None, None) == EARG, word
        assert word in lib.wn_corpus_last_error(), (word, lib.wn_corpus_last_error())
    assert lib.wn_corpus_gather(desc(**feat), 64, 2, TW, 3, 64, 64, None, None, None) == EARG       # features and no `local`
    assert b"NULL col_offset, col_count or local" in lib.wn_corpus_last_error()
    with pytest.raises(_lib.WaveNetHipError, match="n_cols = 0"):
        _corpus.check(lib.wn_corpus_gather(desc(**feat), 64, 2, TW, 0, 64, 64, 64, None, None))


def test_header_map_and_binding_name_the_same_three_functions():
    hdr = open(os.path.join(ROOT, "include", "wavenet_corpus.h")).read()
    declared = set(re.findall(r"\b(wn_corpus_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_corpus.EXPORTS) == {"wn_corpus_abi_version", "wn_corpus_last_error", "wn_corpus_gather"}
    assert "wn_corpus*" in open(os.path.join(ROOT, "wavenet_amd", "csrc", "corpus_exports.map")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _corpus.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in nm.splitlines() if ln.strip()} == declared
    assert _corpus.lib().wn_corpus_abi_version() == _corpus.ABI_VERSION == int(re.search(r"#define WN_CORPUS_ABI_VERSION (\d+)", hdr).group(1))
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct WnCorpusDesc \{(.*?)\} WnCorpusDesc;", hdr, re.S).group(1), flags=re.S)
    fields = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert fields == [f[0] for f in _corpus.WnCorpusDesc._fields_]
    assert C.sizeof(_corpus.WnCorpusDesc) == 7 * 8 + 8 + 8 * 4
    assert "getenv" not in open(os.path.join(ROOT, "wavenet_amd", "csrc", "corpus.hip")).read()


def test_parse_accepts_corpus_with_the_flags_it_works_with_and_is_unchanged_without():
    from wavenet_amd.train_audio import args as cli_args
    combos = [["--speaker-prefix", "--condition-channels", "4"], ["--local-dir", "d", "--local-hop", "16"],
              ["--local-mel", "--mels", "8", "--win", "64", "--local-interp", "linear", "--local-crop", "sample"],
              ["--local-mel", "--local-upsample", "4", "--local-crop", "frame"], ["--ema-decay", "0.999", "--valid-wav-dir", "v"],
              ["--storage", "bf16"], ["--no-graph"], []]
    for argv in combos:
        without, with_flag = cli_args.parse(argv), cli_args.parse(argv + ["--corpus"])
        assert with_flag.corpus is True and without.corpus is False and "corpus" not in vars(without)
        assert dict(vars(with_flag), corpus=None) == dict(vars(without), corpus=None)
    assert vars(cli_args.parse([])) == {k: v for k, v in vars(cli_args.parse(["--corpus"])).items() if k != "corpus"}


def test_train_checks_the_flag_before_a_model_is_built(tmp_path):
    from wavenet_amd.train_audio import train as cli_train
    (tmp_path / "wav").mkdir()
    with pytest.raises(SystemExit, match="train --corpus: no .wav file in"):
        cli_train.main(["-w", str(tmp_path / "wav"), "-m", str(tmp_path / "model"), "--corpus"])
    with pytest.raises(SystemExit, match="--repeat must be at least 1, got 2, 500 and 0"):
        cli_train.main(["-w", str(tmp_path / "wav"), "-m", str(tmp_path / "model"), "--corpus", "--repeat", "0", "--batch-size", "2"])
    assert not (tmp_path / "model").exists()
