"""``train --gpus N`` and ``evaluate --gpus N``: two ranks sharing cuda:0 over gloo (the hook WAVENET_DP_SHARE_GPU=1, the
rehearsal of tests/test_gpu_dp.py) against one process with the same seed, the same files and the same GLOBAL batch.  Every
child process runs under a time limit.  The self-arming case at the end runs one rank per device over RCCL where a node has
two devices.

The largest differences seen go to dp_cli.json in the directory that WAVENET_HIP_RECORD_DIR names (unset: no record is written;
profiles/dp_cli.json holds a committed copy under "largest_weight_difference")."""
import hashlib
import json
import os
import re
import signal
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVER = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 5,
            residual_num_blocks=2, softmax_conv_channels=[256, 256])           # tests/test_gpu_dp.py's OVER
SR, TW, BATCH, UPDATES = 8000, 150, 4, 3
F, HOP, WIN = 8, 16, 64
MEL = ["--local-mel", "--mels", str(F), "--win", str(WIN), "--local-hop", str(HOP)]
FILES = (("p1_a.wav", 3000), ("p1_b.wav", 4200), ("p2_a.wav", 2500))
ATOL = 2e-5                                                                    # test_two_ranks_on_one_gpu_follow_the_global_batch_step's
LIMIT = 300                                                                    # seconds a child process may take
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    where = os.environ.get("WAVENET_HIP_RECORD_DIR")
    if RECORD and where:
        os.makedirs(where, exist_ok=True)
        path, whole = os.path.join(where, "dp_cli.json"), {}
        if os.path.isfile(path):                              # tools/time_dp_cli.py keeps its "timing" in the same file
            with open(path) as f:
                whole = json.load(f)
        whole.update({"largest_weight_difference": RECORD, "bound": ATOL})
        with open(path, "w") as f:
            f.write(json.dumps(whole, indent=1, sort_keys=True) + "\n")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _write_wavs(where, files=FILES):
    from scipy.io import wavfile
    from wavenet_amd import data
    where.mkdir()
    clips = data.synthetic_waveform(len(files), max(n for _, n in files), SR)
    for (name, n), clip in zip(files, clips):
        wavfile.write(str(where / name), SR, np.round(clip[:n] * 32767).astype(np.int16))
    return where


@pytest.fixture(scope="module")
def wav(tmp_path_factory):
    return _write_wavs(tmp_path_factory.mktemp("dp_cli") / "wav")


# ---- 1. function level: train_corpus / train_audio on a data-parallel network ---------------------------------------------------------
def _net(case, seed):
    from wavenet_amd import Params, WaveNet
    kw = dict(condition_classes=2, condition_channels=4, local_channels=F, local_hop=HOP) if case == "conditioned" else {}
    net = WaveNet(Params(dict(OVER, sampling_rate=SR)), seed=seed, **kw)
    net.speakers = ["p1", "p2"] if kw else None
    net.local, net.local_mel = ((F, HOP), {"win": WIN}) if kw else (None, None)
    net.to_gpu()
    net.update_laerning_rate(0.01)
    net.optimizer.eps = 1e-3                                  # see test_train_step_graph_replay_equals_eager_steps
    return net


def _updates(net, case, wav_dir):
    """UPDATES updates from numpy seed 5 -> (every global draw made, the summed loss)."""
    from wavenet_amd.train_audio import train as T
    names = [n for n, _ in FILES]
    draws, state = [], {}
    np.random.seed(5)
    if case == "per_file":
        real = T._Crops.draw

        def spy(self, n, **kw):
            out = real(self, n, **kw)
            draws.append(np.array(self.last_draw))
            return out
        T._Crops.draw = spy
        try:
            loss = sum(T.train_audio(net, net.params, os.path.join(wav_dir, fn), batch_size=BATCH, train_width=TW, repeat=rep,
                                     state=state) for fn, rep in ((names[0], UPDATES - 1), (names[1], 1)))
        finally:
            T._Crops.draw = real
        return draws, loss
    crop = "sample" if case == "conditioned" else "frame"
    corpus = T.load_corpus(net, net.params, wav_dir, names, local_mel=net.local_mel)
    real = corpus.draw_indices

    def spy(*a, **k):
        out = real(*a, **k)
        draws.append(np.stack(out))
        return out
    corpus.draw_indices = spy
    loss = T.train_corpus(net, net.params, corpus, batch_size=BATCH, train_width=TW, repeat=UPDATES, state=state, local_crop=crop)
    assert np.array_equal(np.stack(corpus.last_draw), draws[-1]) and draws[-1].shape == (2, BATCH)
    assert corpus.launches == UPDATES
    return draws, loss


def _worker(rank, world, port, tmp, case, wav_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        net = _net(case, 100 + rank)                          # every rank starts elsewhere: the broadcast fixes that
        dp = net.enable_data_parallel()
        assert dp.shard(BATCH) == (rank * BATCH // world, (rank + 1) * BATCH // world)
        draws, loss = _updates(net, case, wav_dir)
        torch.cuda.synchronize()
        got = net._arena.detach().cpu().numpy()
        seen = [None] * world
        dist.all_gather_object(seen, {"draws": draws, "loss": loss, "sha": hashlib.sha256(got.tobytes()).hexdigest()})
        assert len(draws) == UPDATES
        for other in seen:                                    # the same global draws, the same loss, bit-equal arenas
            assert all(np.array_equal(a, b) for a, b in zip(other["draws"], draws)) and len(other["draws"]) == UPDATES
            assert other["loss"] == loss and other["sha"] == seen[0]["sha"]
        if rank == 0:
            ref = _net(case, 100)
            start = ref._arena.detach().cpu().numpy().copy()
            ref_draws, ref_loss = _updates(ref, case, wav_dir)
            torch.cuda.synchronize()
            want = ref._arena.detach().cpu().numpy()
            assert all(np.array_equal(a, b) for a, b in zip(ref_draws, draws)) and len(ref_draws) == UPDATES
            assert np.abs(want - start).max() > 1e-3                   # the weights did move
            worst = float(np.abs(got - want).max())
            print("%s: largest |two ranks - one process| = %.3e, losses %r / %r" % (case, worst, loss, ref_loss))
            with open(os.path.join(tmp, "worst"), "w") as f:
                f.write(repr(worst))
            np.testing.assert_allclose(got, want, atol=ATOL, rtol=0)
        open(os.path.join(tmp, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["unconditioned", "conditioned", "per_file"])
def test_two_ranks_train_the_global_batch_of_one_process(tmp_path, wav, case):
    """``train_corpus`` (unconditioned; speakers + log-mel features with a phase per crop) and ``train_audio`` (the per-file loop's
    ``_Crops``) on a data-parallel network, Adam at lr 0.01 and eps 1e-3, three updates: both ranks make the draws one process
    makes, end bit-equal, and rank 0 ends within 2e-5 of that process."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), case, str(wav)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")
    RECORD["function_" + case] = float((tmp_path / "worst").read_text())


# ---- 2. the command line ---------------------------------------------------------------------------------------------------------
def _model_dir(where, optimizer="sgd"):
    where.mkdir()
    (where / "wavenet.json").write_text(json.dumps(dict(OVER, sampling_rate=SR, optimizer=optimizer)))
    return where


def _ranks(module, argv, share_gpu=True):
    """``python -m module argv`` as a child under a time limit -> (stdout, stderr); the exit status must be 0."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "WAVENET_DP_SHARE_GPU"):
        env.pop(k, None)
    if share_gpu:
        env["WAVENET_DP_SHARE_GPU"] = "1"
    # a session of its own: at the time limit the launcher AND its ranks are ended, not the direct child alone
    child = subprocess.Popen([sys.executable, "-m", module] + [str(a) for a in argv], env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, text=True, cwd=ROOT, start_new_session=True)
    try:
        out, err = child.communicate(timeout=LIMIT)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.communicate()
        raise
    assert child.returncode == 0, out[-2000:] + err[-4000:]
    return out, err


def _lines(out, model):
    """What a run printed, line by line (progress lines end in a carriage return), the model directory and the figures of the
    epoch lines taken out: those differ between the runs compared.  The first thing a command prints is "loading .../wavenet.json";
    what stands before it is gloo's own word on its connections, written by its C++ side as the ranks join."""
    out = out[out.index("loading "):].replace(str(model), "MODEL")
    out = re.sub(r"(epoch: \d+ - )\S+( loss - )\d+( min)", r"\1L\2M\3", out)
    out = re.sub(r"(held-out (?:ema )?weights: )\S+( nats/sample  )\S+", r"\1N\2B", out)
    return [ln for ln in re.split(r"[\r\n]+", out.replace("\033[2K", "")) if ln.strip()]


def _weights(model):
    with np.load(str(model / "wavenet.model.npz")) as z:
        return {k: z[k] for k in z.files}


def _largest(a, b):
    assert sorted(a) == sorted(b)
    return max(float(np.abs(a[k] - b[k]).max()) for k in a)


def _compare_with_one_process(tmp, wav_dir, gpus, extra, capsys, share_gpu=True, batch=BATCH, resume=True):
    """``train --gpus`` in a child against ``train`` in this process: exit status, files, lines, weights; then both once more,
    resumed.  Returns the largest weight difference of the two comparisons."""
    from wavenet_amd.train_audio import train as cli_train
    loop = ["-w", wav_dir, "--seed", "1", "--lr", "0.01", "--batch-size", batch, "--train-width", TW, "--repeat", "1",
            "--max-epoch", "2"] + extra
    from wavenet_amd import Params, WaveNet
    many, one = _model_dir(tmp / "many"), _model_dir(tmp / "one")
    # what both commands start from: model.build seeds the network with --seed
    worst, before = [], WaveNet(Params(json.loads((one / "wavenet.json").read_text())), seed=1).state_dict()
    for run in range(2 if resume else 1):
        out, _ = _ranks("wavenet_amd.train_audio.train", loop + ["-m", many, "--gpus", gpus], share_gpu)
        capsys.readouterr()
        cli_train.main([str(a) for a in loop + ["-m", one]])
        want = capsys.readouterr().out
        # every line once: what N ranks print is what one process prints (its progress, "loading", corpus and epoch lines)
        assert _lines(out, many) == _lines(want, one), (out, want)
        assert len(re.findall(r"epoch: 1 - ", out)) == 1 and out.count("loading p1_a.wav") == 1
        assert ("wavenet.model.npz" in out) == (run == 1)                           # the second invocation resumes ...
        # every checkpoint file once: the directory holds what one process leaves, and nothing of another rank's
        assert sorted(p.name for p in many.iterdir()) == sorted(p.name for p in one.iterdir())
        assert json.loads((many / "wavenet.json").read_text()) == json.loads((one / "wavenet.json").read_text())
        got, ref = _weights(many), _weights(one)
        worst.append(_largest(got, ref))
        print("run %d: largest |%s ranks - one process| = %.3e" % (run, gpus, worst[-1]))
        for k in got:
            np.testing.assert_allclose(got[k], ref[k], atol=ATOL, rtol=0, err_msg=k)
        # ... and trains on from there.  The weights did move, in every invocation: three SGD steps of lr 0.01 under a clipped
        # gradient move a weight by up to 3e-2; agreement to 2e-5 says something only where the movement is well above it
        moved = _largest(got, before)
        print("run %d: the weights moved by %.3e" % (run, moved))
        assert moved > 1e-4
        before = got
    return max(worst)


def test_train_gpus_2_corpus_ends_with_the_weights_of_the_plain_command(tmp_path, wav, capsys):
    """Plain SGD (Adam at eps 1e-8 turns rounding noise into sign flips and cannot be compared), three updates per invocation."""
    RECORD["train_corpus"] = _compare_with_one_process(tmp_path, wav, 2, ["--corpus"], capsys)


def test_train_gpus_2_per_file_loop_ends_with_the_weights_of_the_plain_command(tmp_path, wav, capsys):
    RECORD["train_per_file"] = _compare_with_one_process(tmp_path, wav, 2, [], capsys, resume=False)


def _save_worker(rank, world, port, tmp, wav_dir):
    """One rank of ``train --gpus 2``, started as a launcher starts it, with ``WaveNet.save`` counted per rank."""
    from wavenet_amd import WaveNet
    from wavenet_amd.train_audio import train as cli_train
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      WAVENET_DP_SHARE_GPU="1")
    real, calls = WaveNet.save, []

    def counted(self, model_dir="./"):
        calls.append(model_dir)
        return real(self, model_dir)
    WaveNet.save = counted
    model = os.path.join(tmp, "model")
    cli_train.main(["-w", wav_dir, "-m", model, "--seed", "1", "--lr", "0.01", "--batch-size", str(BATCH), "--train-width", str(TW),
                    "--repeat", "1", "--max-epoch", "2", "--corpus", "--gpus", str(world)])
    with open(os.path.join(tmp, "saves%d" % rank), "w") as f:
        json.dump(calls, f)


def test_rank_0_alone_writes_the_checkpoints(tmp_path, wav):
    """Both ranks run ``train.main`` to its end; rank 0 calls ``net.save`` once per file and once per epoch, rank 1 never."""
    import torch.multiprocessing as mp
    _model_dir(tmp_path / "model")
    mp.spawn(_save_worker, args=(2, _free_port(), str(tmp_path), str(wav)), nprocs=2, join=True)
    saves = [json.loads((tmp_path / ("saves%d" % r)).read_text()) for r in (0, 1)]
    assert saves[0] == [str(tmp_path / "model")] * (len(FILES) + 1) and saves[1] == []
    assert (tmp_path / "model" / "wavenet.model.npz").exists()


# ---- 3. evaluate --gpus 2, and train --valid-wav-dir ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory, wav):
    """A checkpoint: three updates of the plain command."""
    from wavenet_amd.train_audio import train as cli_train
    model = _model_dir(tmp_path_factory.mktemp("dp_cli_model") / "model")
    cli_train.main(["-w", str(wav), "-m", str(model), "--seed", "1", "--lr", "0.01", "--batch-size", "4", "--train-width", str(TW),
                    "--repeat", "1", "--max-epoch", "2", "--corpus"])
    return model


@pytest.mark.parametrize("n_files", [3, 1])
def test_evaluate_gpus_2_writes_the_table_of_one_process_byte_for_byte(tmp_path, wav, trained, capsys, n_files):
    """Three files: shards of two and one.  One file: a rank with nothing."""
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    held = wav if n_files == 3 else _write_wavs(tmp_path / "held", FILES[1:2])
    argv = ["-w", held, "-m", trained, "--chunk-width", "700", "--batch-size", "2"]
    out, _ = _ranks("wavenet_amd.train_audio.evaluate", argv + ["--gpus", "2", "--json", tmp_path / "a.json"])
    capsys.readouterr()
    table = cli_evaluate.main([str(a) for a in argv + ["--json", tmp_path / "b.json"]])
    want = capsys.readouterr().out
    assert (tmp_path / "a.json").read_bytes() == (tmp_path / "b.json").read_bytes()
    assert [r["file"] for r in table["files"]] == sorted(n for n, _ in (FILES if n_files == 3 else FILES[1:2]))
    assert _lines(out, trained) == _lines(want, trained) and out.count("total ") == 1


def test_train_valid_wav_dir_under_two_ranks_prints_one_held_out_line_per_epoch(tmp_path, wav):
    """Two training files, epochs 1 and 2 (--max-epoch 3), three held-out files, with a weight average: per epoch one line for the
    weights and one for the averaged ones, the held-out files scored by the two ranks in turn."""
    few = _write_wavs(tmp_path / "few", FILES[:2])
    model = _model_dir(tmp_path / "model")
    out, _ = _ranks("wavenet_amd.train_audio.train",
                    ["-w", few, "-m", model, "--seed", "1", "--lr", "0.01", "--batch-size", BATCH, "--train-width", TW, "--repeat", "1",
                     "--max-epoch", "3", "--corpus", "--gpus", "2", "--valid-wav-dir", wav, "--ema-decay", "0.9"])
    for epoch in (1, 2):
        assert len(re.findall(r"epoch: %d - held-out weights: \S+ nats/sample" % epoch, out)) == 1
        assert len(re.findall(r"epoch: %d - held-out ema weights: \S+ nats/sample" % epoch, out)) == 1
        assert len(re.findall(r"epoch: %d - \S+ loss" % epoch, out)) == 1
    samples = set(re.findall(r"\((\d+) samples\)", out))
    assert len(samples) == 1 and int(samples.pop()) > 3 * 2000                    # all three files, whichever rank scored them
    assert (model / "wavenet.ema.npz").exists()


# ---- 4. one rank per device over RCCL: arms itself on a node with two devices -----------------------------------------------------
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs: arms itself on a multi-GPU node")
def test_train_gpus_n_over_rccl_one_rank_per_device(tmp_path, wav, capsys):
    """``train --gpus min(device_count, 8) --corpus`` with no hook: backend "nccl", rank r on device r, two clips per rank; the
    assertions of the two-rank rehearsal above."""
    world = min(torch.cuda.device_count(), 8)
    RECORD["train_corpus_rccl_%d" % world] = _compare_with_one_process(tmp_path, wav, world, ["--corpus"], capsys, share_gpu=False,
                                                                     batch=2 * world)
