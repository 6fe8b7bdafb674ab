"""``--gpus N`` without a GPU: the flag, the refusals made before anything is launched, the launcher's command line, and the
arithmetic that lets N equally seeded ranks cover one global draw and one sorted table."""
import ast
import builtins
import importlib.util
import os
import sys

import numpy as np
import pytest

from wavenet_amd import Corpus
from wavenet_amd.dp import DataParallel
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import evaluate as cli_evaluate
from wavenet_amd.train_audio import generate as cli_generate
from wavenet_amd.train_audio import launch
from wavenet_amd.train_audio import train as cli_train
from wavenet_amd.train_audio.train import _Crops

IW, TW, HOP, F = 9, 16, 16, 3
LENGTHS = [61, 17, 18, 64, 257, 700]                 # (17 holds no window: the draw leaves it out)


def test_the_flag_is_absent_from_a_namespace_that_did_not_give_it():
    plain = cli_args.parse(["-w", "wav"])
    assert "gpus" not in vars(plain) and plain.gpus == 1 and cli_args.Args.gpus == 1
    assert vars(cli_args.parse(["--gpus", "4"]))["gpus"] == 4
    assert "gpus" not in vars(cli_evaluate.build_parser().parse_args([]))
    assert cli_evaluate.build_parser().parse_args(["--gpus", "2"]).gpus == 2


@pytest.fixture
def nothing_starts(monkeypatch):
    """A refusal comes before a launch and before a model: either one fails the test."""
    def never(*a, **k):
        raise AssertionError("the command line went on past the check")
    monkeypatch.setattr(launch, "run", never)
    monkeypatch.setattr(cli_train._model, "build", never)
    monkeypatch.delenv("WORLD_SIZE", raising=False)


@pytest.mark.parametrize("main", [cli_train.main, cli_evaluate.main], ids=["train", "evaluate"])
@pytest.mark.parametrize("n", [0, 9, -1])
def test_gpus_outside_1_to_8_is_refused_naming_the_value(nothing_starts, capsys, main, n):
    with pytest.raises(SystemExit) as e:
        main(["--gpus", str(n)])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--gpus" in err and "1 .. 8" in err and "got %d" % n in err


def test_a_batch_that_does_not_divide_by_the_ranks_is_refused_before_launch(nothing_starts):
    with pytest.raises(SystemExit) as e:
        cli_train.main(["--gpus", "2", "--batch-size", "3"])
    assert "--batch-size 3" in str(e.value.code) and "--gpus 2" in str(e.value.code)
    assert launch.check_batch(16, 8) == 2
    with pytest.raises(ValueError, match="--batch-size 16 .* --gpus 3"):
        launch.check_batch(16, 3)


def test_world_size_different_from_gpus_stops_before_a_model_is_built(nothing_starts, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "3")
    with pytest.raises(SystemExit) as e:
        cli_train.main(["--gpus", "2", "--batch-size", "4"])
    assert "--gpus 2" in str(e.value.code) and "WORLD_SIZE=3" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        cli_train.main(["--batch-size", "4"])                         # no flag inside a launcher's world of three
    assert "--gpus 1" in str(e.value.code) and "WORLD_SIZE=3" in str(e.value.code)


def test_generate_and_copy_synthesis_refuse_the_flag(nothing_starts, monkeypatch):
    with pytest.raises(SystemExit) as e:
        cli_generate.main(["--gpus", "2"])
    assert "--gpus 2" in str(e.value.code) and "generate" in str(e.value.code)
    monkeypatch.setattr(cli_evaluate, "copy_synthesis_job", lambda args: {})
    with pytest.raises(SystemExit) as e:
        cli_evaluate.main(["--gpus", "2", "--copy-synthesis"])
    assert "--gpus 2" in str(e.value.code) and "--copy-synthesis" in str(e.value.code)


def test_the_parent_hands_its_own_arguments_to_the_launcher_and_its_exit_code_on(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    seen = []
    monkeypatch.setattr(launch, "run", lambda module, argv, n: seen.append((module, list(argv), n)) or 3)
    argv = ["--gpus", "2", "--batch-size", "4", "-w", "somewhere"]
    with pytest.raises(SystemExit) as e:
        cli_train.main(argv)
    assert e.value.code == 3 and seen == [("wavenet_amd.train_audio.train", argv, 2)]
    del seen[:]
    with pytest.raises(SystemExit) as e:
        cli_evaluate.main(["--gpus", "5", "--json", "t.json"])
    assert e.value.code == 3 and seen == [("wavenet_amd.train_audio.evaluate", ["--gpus", "5", "--json", "t.json"], 5)]


def test_launch_command_is_the_expected_list():
    got = launch.command("wavenet_amd.train_audio.train", ["--gpus", "2", "-w", "wav", "--seed", 1], 2, 29511)
    assert got == [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                   "--master-port", "29511", "-m", "wavenet_amd.train_audio.train", "--gpus", "2", "-w", "wav", "--seed", "1"]
    with pytest.raises(ValueError, match="got 9"):
        launch.command("m", [], 9, 1)
    assert "retry" not in " ".join(got) and not any(a.startswith("--max-restarts") for a in got)


def test_the_ranks_environment_is_the_benchmarks():
    env = launch.environment({"A": "b"})
    assert env == {"A": "b", "HSA_ENABLE_IPC_MODE_LEGACY": "0", "OMP_NUM_THREADS": "8"}
    assert launch.environment({"OMP_NUM_THREADS": "16"})["OMP_NUM_THREADS"] == "16"       # what is set stays


def test_launch_imports_no_torch_until_a_rank_joins(monkeypatch):
    """The parent's half -- the checks, the command, the environment -- runs with ``import torch`` made to fail: the module has
    no such import at its top level, so importing it cannot create any ``torch.cuda`` state."""
    path = launch.__file__
    tree = ast.parse(open(path).read())
    top = [n for n in tree.body if isinstance(n, (ast.Import, ast.ImportFrom))]
    names = {a.name.split(".")[0] for n in top if isinstance(n, ast.Import) for a in n.names} | \
            {(n.module or "").split(".")[0] for n in top if isinstance(n, ast.ImportFrom)}
    assert "torch" not in names and "wavenet_amd" not in names and all(n.level == 0 for n in top if isinstance(n, ast.ImportFrom))
    real = builtins.__import__

    def no_torch(name, *a, **k):
        if name == "torch" or name.startswith("torch."):
            raise AssertionError("import %s" % name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_torch)
    spec = importlib.util.spec_from_file_location("launch_alone", path)
    alone = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(alone)
    assert alone.command("m", ["x"], 8, 1)[-3:] == ["-m", "m", "x"] and alone.check_gpus(1) == 1
    assert alone.check_batch(8, 4) == 2 and "OMP_NUM_THREADS" in alone.environment({})
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert not alone.in_rank()


def _corpus_on_host(with_features=True):
    rs = np.random.RandomState(0)
    files = [rs.randint(0, 256, size=n).astype(np.int32) for n in LENGTHS]
    feats = [rs.randn(F, -(-n // HOP)).astype(np.float32) for n in LENGTHS] if with_features else None
    return Corpus(files, IW, 256, "cpu", features=feats, hop=HOP)


@pytest.mark.parametrize("crop", ["sample", "frame"])
def test_equally_seeded_generators_give_equal_pairs(crop):
    c = _corpus_on_host()
    a = c.draw_indices(12, TW, crop, rng=np.random.RandomState(7))
    b = c.draw_indices(12, TW, crop, rng=np.random.RandomState(7))
    other = c.draw_indices(12, TW, crop, rng=np.random.RandomState(8))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], other[1])


def _rank(rank, world):
    dp = object.__new__(DataParallel)                  # the arithmetic alone: no process group
    dp.rank, dp.world = rank, world
    return dp


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_the_ranks_shards_partition_the_global_draw(world):
    """``Corpus.draw(..., shard=)`` under equally seeded generators: every rank makes the one global ``randint`` call, keeps all
    its pairs in ``last_draw`` and hands its own [lo, hi) of them to the gather; the shards are ``dp.shard``'s and, put end to
    end, are the draw of a single process."""
    batch = 24
    whole = _corpus_on_host()
    seen = []
    whole.gather = lambda files, starts, tw, n_cols=None: seen.append((files, starts))
    whole.draw(batch, TW, "sample", 3, rng=np.random.RandomState(5))
    (files, starts), = seen
    assert files.size == batch and np.array_equal(whole.last_draw[0], files) and np.array_equal(whole.last_draw[1], starts)
    parts, edges = [], []
    for r in range(world):
        c = _corpus_on_host()
        got = []
        c.gather = lambda files, starts, tw, n_cols=None: got.append((files, starts))
        rng = np.random.RandomState(5)
        shard = _rank(r, world).shard(batch)
        assert shard == (r * batch // world, (r + 1) * batch // world)
        c.draw(batch, TW, "sample", 3, rng=rng, shard=shard)
        assert np.array_equal(c.last_draw[0], files) and np.array_equal(c.last_draw[1], starts)        # the GLOBAL pairs
        parts.append(got[0])
        edges.append(shard)
    assert edges[0][0] == 0 and edges[-1][1] == batch and all(a[1] == b[0] for a, b in zip(edges, edges[1:]))
    assert np.array_equal(np.concatenate([p[0] for p in parts]), files)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), starts)
    with pytest.raises(ValueError, match="not divisible"):
        _rank(0, 5).shard(batch)
    with pytest.raises(ValueError, match="shard"):
        whole.draw(batch, TW, "sample", 3, rng=np.random.RandomState(5), shard=(20, 25))


def test_a_sharded_draw_consumes_the_generator_as_the_whole_draw_does():
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    whole, part = _corpus_on_host(), _corpus_on_host()
    whole.gather = part.gather = lambda *args, **kw: None
    for _ in range(3):
        whole.draw(8, TW, "frame", 2, rng=a)
        part.draw(8, TW, "frame", 2, rng=b, shard=(4, 8))
    assert np.array_equal(whole.last_draw[1], part.last_draw[1]) and a.randint(1 << 30) == b.randint(1 << 30)


@pytest.mark.parametrize("kind", ["plain", "sample", "frame"])
def test_the_per_file_sampler_shards_the_same_way(kind):
    """``_Crops.draw(batch, shard=)`` on the host: the same global starts in ``last_draw``, and rows lo .. hi - 1 of everything
    the unsharded draw returns -- tokens, targets, feature columns and phases."""
    rs = np.random.RandomState(2)
    sig = rs.randint(0, 256, size=900).astype(np.int32)
    kw = {} if kind == "plain" else dict(features=rs.randn(F, 900 // HOP + 2).astype(np.float32), hop=HOP, shift=7, crop=kind)
    np.random.seed(11)
    whole = _Crops(sig, IW, TW, "cpu", **kw)
    full = whole.draw(8)
    assert whole.last_draw.shape == (8,)
    for lo, hi in ((0, 4), (4, 8), (6, 8)):
        np.random.seed(11)
        part = _Crops(sig, IW, TW, "cpu", **kw)
        got = part.draw(8, shard=(lo, hi))
        assert np.array_equal(part.last_draw, whole.last_draw) and len(got) == len(full)
        for g, f in zip(got, full):
            assert np.array_equal(np.asarray(g), np.asarray(f)[lo:hi])


@pytest.mark.parametrize("n_files", [1, 3, 4, 7])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_strided_file_shards_restore_the_sorted_list_and_the_table(world, n_files):
    """``files[r::w]`` over r is the sorted list again (w above the file count included: those ranks hold nothing), and the
    table formed from the merged rows is the unsharded one to the last bit, on rows whose products do not sum exactly."""
    files = sorted("p%03d_%d.wav" % (i * 37 % 11, i) for i in range(n_files))
    rs = np.random.RandomState(n_files)
    rows = [dict(file=fn, samples=int(rs.randint(1, 10 ** 6)), nats_per_sample=float(rs.rand() * 5 + 1e-3),
                 bits_per_sample=float(rs.rand())) for fn in files]
    per_rank = [rows[r::world] for r in range(world)]
    assert sum(len(p) for p in per_rank) == n_files and (world <= n_files or per_rank[-1] == [])
    assert [r["file"] for r in cli_evaluate.merge_rows(per_rank)] == files
    assert [r["file"] for r in cli_evaluate.merge_rows(per_rank[::-1])] == files          # whatever order the ranks answer in
    want = cli_evaluate.table_of(rows)
    got = cli_evaluate.table_of(cli_evaluate.merge_rows(per_rank))
    assert got == want and got["files"] == rows
    nats = 0.0
    for r in rows:
        nats += r["nats_per_sample"] * r["samples"]
    assert want["total"]["samples"] == sum(r["samples"] for r in rows)
    assert want["total"]["nats_per_sample"] == nats / want["total"]["samples"]               # as evaluate_dir always formed it


def test_join_in_a_world_of_one_joins_nothing(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    args = cli_args.parse(["-g", "3"])
    assert launch.join(args) == (0, 1) and args.gpu_device == 3
    assert launch.shared_seed(None, 0, 1) is None and launch.shared_seed(4, 0, 1) == 4
    assert launch.build_in_turn(lambda: "built", 0, 1) == "built"
    launch.leave(1)
