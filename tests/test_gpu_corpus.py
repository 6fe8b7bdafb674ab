"""Crops across the corpus on the device: ``wn_corpus_gather`` against tests/corpus_ref.py bit for bit, ``train --corpus`` on one
file against the per-file run, several files that really mix, and the call inside a captured graph."""
import json

import numpy as np
import pytest
import torch

import corpus_ref as R
from gpu_util import to_np
from test_gpu_logmel import CFG, LOOP, MEL
from wavenet_amd import Corpus, _corpus, _lib
from wavenet_amd.corpus import columns_per_crop

pytestmark = pytest.mark.gpu

IW, TW, HOP, F = 9, 16, 16, 3
LENGTHS = [61, 64, 257, 700, 1001]
# (file, start); a start is legal in [0, len - TW - 1).  shift = 7, pad_cols = 1:
DRAWS = [(0, 0),        # starts in the silence pad; first = 0 < pad_cols
         (2, 4),        # straddles pad and file
         (0, 43), (1, 46), (2, 239), (3, 682), (4, 983),      # the last legal start of every file; (0, 43): columns 2, 3, 4 of 4
         (1, 9), (3, 25),                                     # on a column border (frame mode's starts)
         (4, 500), (3, 8), (2, 10), (4, 1), (1, 20)]
MODES = [("sample", "repeat", 1), ("frame", "repeat", 1), ("sample", "linear", 1), ("sample", "repeat", 4), ("frame", "linear", 4)]
GUARD, INT_FILL, FLOAT_FILL = 64, -7, 12345.0


def _corpus_of(q, classes=True, features=True):
    rs = np.random.RandomState(q)
    tokens = [rs.randint(0, q, size=n).astype(np.int32) for n in LENGTHS]
    feats = [rs.randn(F, -(-n // HOP) + (0, 2)[i % 2]).astype(np.float32) for i, n in enumerate(LENGTHS)] if features else None
    return Corpus(tokens, IW, q, "cuda", features=feats, hop=HOP, classes=[3, 0, 2, 2, 1] if classes else None)


_CORPORA = {}


def corpus(q, **kw):
    key = (q,) + tuple(sorted(kw.items()))
    if key not in _CORPORA:
        _CORPORA[key] = _corpus_of(q, **kw)
    return _CORPORA[key]


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def _raw_gather(c, draws, n_cols):
    """The raw ABI on outputs that sit between guard words; -> the four outputs, after checking that the guards are untouched."""
    B = len(draws)
    table = torch.as_tensor(np.asarray(draws, dtype=np.int32)).cuda()
    bufs = {"x": _guarded(B * (IW + TW), torch.int32, INT_FILL), "tgt": _guarded(B * TW, torch.int32, INT_FILL),
            "local": _guarded(B * c.F * n_cols, torch.float32, FLOAT_FILL) if c.features is not None else (None, None),
            "cond": _guarded(B, torch.int64, INT_FILL) if c.file_class is not None else (None, None)}
    rc = _corpus.lib().wn_corpus_gather(c.desc, _lib.ptr(table), B, TW, n_cols, *[_lib.ptr(bufs[k][1]) for k in ("x", "tgt", "local", "cond")],
                                        _lib.stream_ptr())
    _corpus.check(rc)
    torch.cuda.synchronize()
    out = {}
    for k, (buf, inner) in bufs.items():
        if buf is None:
            out[k] = None
            continue
        fill = FLOAT_FILL if k == "local" else INT_FILL
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + inner.numel():] == fill).all()), "written outside " + k
        out[k] = to_np(inner)
    return out["x"].reshape(B, IW + TW), out["tgt"].reshape(B, TW), \
        None if out["local"] is None else out["local"].reshape(B, c.F, n_cols), out["cond"]


def _same(got, want):
    if want is None:
        return got is None
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8),
                                                                                  np.ascontiguousarray(want).view(np.uint8))


@pytest.mark.parametrize("q", [256, 300])
@pytest.mark.parametrize("crop,interp,U", MODES)
def test_the_gather_is_the_reference_bit_for_bit_and_writes_its_outputs_only(q, crop, interp, U):
    c = corpus(q)
    assert c.tokens.dtype == (np.uint8 if q == 256 else np.int32) and c.desc.token_bytes == c.tokens.dtype.itemsize
    assert c.file_offset.tolist() == [0, 61, 125, 382, 1082]                       # unaligned file starts
    n_cols = columns_per_crop(IW, TW, HOP, crop, interp, U)
    for draws in (DRAWS[:7], DRAWS[7:], DRAWS[:1], DRAWS[2:3], DRAWS[6:7]):          # B = 7 twice, B = 1 three times
        files, starts = [d[0] for d in draws], [d[1] for d in draws]
        c.check_draws(np.asarray(files), np.asarray(starts), TW)                   # the draws are legal ones
        want = R.of_corpus(c, files, starts, TW, n_cols, interp, U)
        got = _raw_gather(c, draws, n_cols)
        for name, g, w in zip(("x", "tgt", "local", "condition"), got, want):
            assert w is not None and _same(g, w), (name, draws)
        assert INT_FILL not in want[0] and INT_FILL not in want[1] and FLOAT_FILL not in want[2]      # equal: every element written
    # the Python face: the same arrays, the phases from the host
    files, starts = np.array([d[0] for d in DRAWS]), np.array([d[1] for d in DRAWS])
    before = c.launches
    x, tgt, local, cond, phases = c.gather(files, starts, TW, n_cols)
    want = R.of_corpus(c, files, starts, TW, n_cols, interp, U)
    assert c.launches == before + 1
    assert all(_same(to_np(g), w) for g, w in zip((x, tgt, local, cond), want)) and _same(phases, want[4])
    assert phases.tolist() == [(s + 7) % HOP for s in starts]


@pytest.mark.parametrize("q", [256, 300])
def test_a_corpus_without_features_or_classes_writes_tokens_only(q):
    c = corpus(q, classes=False, features=False)
    got = _raw_gather(c, DRAWS[:7], 0)
    want = R.of_corpus(c, [d[0] for d in DRAWS[:7]], [d[1] for d in DRAWS[:7]], TW)
    assert _same(got[0], want[0]) and _same(got[1], want[1]) and got[2] is None and got[3] is None and want[2] is None
    x, tgt, local, cond, phases = c.gather(np.array([4]), np.array([983]), TW)
    assert local is None and cond is None and phases is None and _same(to_np(x), R.of_corpus(c, [4], [983], TW)[0])


def test_a_window_longer_than_one_workgroups_chunk():
    """input_width + target_width + 1 = 1,034 window positions and 3 x 67 feature cells: two chunks per crop, the second one
    holding the window's tail, the targets' tail and every feature cell."""
    rs = np.random.RandomState(5)
    lengths = [1100, 2100]
    c = Corpus([rs.randint(0, 256, size=n) for n in lengths], IW, 256, "cuda", hop=HOP, classes=[1, 0],
               features=[rs.randn(F, -(-n // HOP)).astype(np.float32) for n in lengths])
    tw, n_cols = 1024, 67
    files, starts = np.array([1, 1, 0]), np.array([0, 2100 - tw - 2, 1100 - tw - 2])
    x, tgt, local, cond, _ = c.gather(files, starts, tw, n_cols)
    want = R.of_corpus(c, files, starts, tw, n_cols)
    assert all(_same(to_np(g), w) for g, w in zip((x, tgt, local, cond), want))


def test_the_call_is_capturable_and_a_replay_follows_the_refilled_draw_table():
    c = corpus(256)
    B, n_cols = 7, 3
    table = torch.as_tensor(np.asarray(DRAWS[:B], dtype=np.int32)).cuda()
    x = torch.full((B, IW + TW), INT_FILL, dtype=torch.int32, device="cuda")
    tgt = torch.full((B, TW), INT_FILL, dtype=torch.int32, device="cuda")
    local = torch.full((B, F, n_cols), FLOAT_FILL, dtype=torch.float32, device="cuda")
    cond = torch.full((B,), INT_FILL, dtype=torch.int64, device="cuda")

    def call():
        _corpus.check(_corpus.lib().wn_corpus_gather(c.desc, _lib.ptr(table), B, TW, n_cols, _lib.ptr(x), _lib.ptr(tgt), _lib.ptr(local),
                                                     _lib.ptr(cond), _lib.stream_ptr()))

    call()                                                                         # (the kernel's code is loaded before the capture)
    x.fill_(INT_FILL)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    torch.cuda.synchronize()
    assert int(x[0, 0]) == INT_FILL                                                # captured, not run
    for draws in (DRAWS[:B], DRAWS[B:2 * B]):
        table.copy_(torch.as_tensor(np.asarray(draws, dtype=np.int32)))
        g.replay()
        torch.cuda.synchronize()
        want = R.of_corpus(c, [d[0] for d in draws], [d[1] for d in draws], TW, n_cols)
        assert all(_same(to_np(got), w) for got, w in zip((x, tgt, local, cond), want)), draws


# ---- train --corpus ----------------------------------------------------------------------------------------------------------------
def _write_wav(path, n, seed):
    """A tone of its own pitch under noise of its own seed: no two files alike, nothing silent to trim."""
    from scipy.io import wavfile
    rs = np.random.RandomState(seed)
    t = np.arange(n) / 8000.0
    x = 0.4 * np.sin(2 * np.pi * (150 + 90 * seed) * t) + 0.1 * rs.randn(n) + 0.05
    wavfile.write(str(path), 8000, np.round(np.clip(x, -1, 1) * 32767).astype(np.int16))


def _train(tmp, name, wav, extra, loop=LOOP):
    from wavenet_amd.train_audio import train as cli_train
    model = tmp / name
    model.mkdir()
    (model / "wavenet.json").write_text(json.dumps(CFG))
    cli_train.main(["-w", str(wav), "-m", str(model)] + loop + extra)
    with np.load(str(model / "wavenet.model.npz")) as z:
        return model, {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def one_file(tmp_path_factory):
    from wavenet_amd.train_audio import features as cli_features
    tmp = tmp_path_factory.mktemp("corpus_one")
    wav = tmp / "wav"
    wav.mkdir()
    _write_wav(wav / "f.wav", 3000, 1)
    cli_features.main(["-w", str(wav), "-o", str(tmp / "feat"), "--hop", "16", "--mels", "8", "--win", "64", "--device"])
    return dict(wav=wav, feat=tmp / "feat")


@pytest.mark.parametrize("case", ["plain", "speaker", "mel", "mel_linear_sample", "dir_upsample", "no_graph"])
def test_with_one_file_the_corpus_run_ends_with_the_per_file_runs_weights(one_file, tmp_path, case):
    extra = {"plain": [], "no_graph": ["--no-graph", "--local-mel"] + MEL + ["--local-crop", "sample"], "speaker": ["--speaker-prefix", "--condition-channels", "4"], "mel": ["--local-mel"] + MEL,
             "mel_linear_sample": ["--local-mel"] + MEL + ["--local-interp", "linear", "--local-crop", "sample"],
             "dir_upsample": ["--local-dir", str(one_file["feat"]), "--local-hop", "16", "--local-upsample", "4"]}[case]
    model_a, wa = _train(tmp_path, "per_file", one_file["wav"], extra)
    model_b, wb = _train(tmp_path, "corpus", one_file["wav"], extra + ["--corpus"])
    assert sorted(wa) == sorted(wb)
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
    for name in ("local.json", "speakers.json"):                                   # the flag is a property of the run
        assert (model_a / name).exists() == (model_b / name).exists()
        if (model_a / name).exists():
            assert (model_a / name).read_bytes() == (model_b / name).read_bytes()
    assert sorted(p.name for p in model_a.iterdir()) == sorted(p.name for p in model_b.iterdir())


def test_several_files_mix_in_a_batch_and_the_kernels_arrays_are_what_trained(tmp_path, monkeypatch):
    wav = tmp_path / "wav"
    wav.mkdir()
    names = ["p1_a.wav", "p1_b.wav", "p2_a.wav", "p2_b.wav"]
    for i, (name, n) in enumerate(zip(names, (1500, 3000, 2200, 1800))):
        _write_wav(wav / name, n, i + 2)
    loop = ["--seed", "1", "--lr", "0.003", "--batch-size", "4", "--train-width", "48", "--repeat", "3", "--max-epoch", "2"]
    extra = ["--speaker-prefix", "--condition-channels", "4", "--local-mel"] + MEL + ["--local-crop", "sample", "--corpus"]
    real = Corpus.gather
    seen = []

    def recording(self, files, starts, target_width, n_cols=None):
        out = real(self, files, starts, target_width, n_cols)
        seen.append((np.array(files), np.array(starts), to_np(out[3]), self.file_class.copy()))
        return out

    monkeypatch.setattr(Corpus, "gather", recording)
    _, wa = _train(tmp_path, "kernel", wav, extra, loop)
    first = list(seen)
    assert len(first) == 4 * 3                                                     # len(files) x --repeat updates
    assert first[0][3].tolist() == [0, 0, 1, 1]
    for files, starts, cond, classes in first:
        assert files.shape == (4,) and np.array_equal(cond, classes[files])        # each crop carries its own file's speaker
    assert any(len(set(cond.tolist())) == 2 for _, _, cond, _ in first)           # a batch held crops of both speakers
    assert len({f for files, _, _, _ in first for f in files.tolist()}) > 2

    def from_reference(self, files, starts, target_width, n_cols=None):
        files, starts = self.check_draws(files, starts, target_width)
        seen.append((files, starts))
        x, tgt, local, cond, phases = R.of_corpus(self, files, starts, target_width, n_cols)
        return tuple(torch.as_tensor(a).cuda() for a in (x, tgt, local, cond)) + (phases,)

    del seen[:]
    monkeypatch.setattr(Corpus, "gather", from_reference)
    _, wb = _train(tmp_path, "reference", wav, extra, loop)
    assert len(seen) == len(first) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(first, seen))
    assert sorted(wa) == sorted(wb) and "global_condition_embed/W" in wa and "local_condition_projection/W" in wa
    for k in wa:
        assert np.array_equal(wa[k], wb[k]), k
