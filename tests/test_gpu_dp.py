"""config 3 stand-in on one GPU: two ranks share cuda:0 over gloo and train data-parallel with the two-graph step
(forward/backward graph -> all-reduce of the flat gradient arena -> optimiser graph, wavenet_amd/graph.py); the weights
must follow the single-process step on the concatenated batch (mean of shard gradients == gradient of
the global batch, then identical hooks + Adam on every rank; train_audio/train.py:58-80 is the step)."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OVER = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 5,
            residual_num_blocks=2, softmax_conv_channels=[256, 256])
CFG2 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10,
            residual_num_blocks=4, softmax_conv_channels=[256, 256])          # BASELINE configs[2]'s stack: 614,656 floats
STEPS = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batches(iw, B_PER, EXTRA):
    rs = np.random.RandomState(3)
    T = iw + EXTRA
    return [(rs.randint(0, 256, (2 * B_PER, T)).astype(np.int32), rs.randint(0, 256, (2 * B_PER, EXTRA)).astype(np.int32))
            for _ in range(STEPS)]


def _worker(rank, world, port, tmp, use_graph, over, B_PER, EXTRA):
    import torch.distributed as dist
    from oracle import wavenet_ref as R
    from wavenet_amd import Params, TrainStepGraph, WaveNet
    from wavenet_amd.graph import default_loss
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = R.make_params(**over)
        w = R.init_weights(p, 11)
        net = WaveNet(Params(p), seed=100 + rank)
        if rank == 0:
            net.load_state_dict(w)
        net.to_gpu()
        net.update_laerning_rate(0.01)
        net.optimizer.eps = 1e-3                 # see test_train_step_graph_replay_equals_eager_steps
        net.optimizer.t = 5 if rank == 0 else 0  # a resumed rank 0: the optimiser clock must travel with the weights
        dp = net.enable_data_parallel()
        assert net.optimizer.t == 5
        iw = net.input_width
        lo, hi = dp.shard(2 * B_PER)
        batches = _batches(iw, B_PER, EXTRA)
        dev = lambda a: torch.as_tensor(a).cuda()
        if use_graph:
            g = TrainStepGraph(net, dev(batches[0][0][lo:hi]), dev(batches[0][1][lo:hi]))
            assert g._g2 is not None and net.optimizer.t == 5
        for x, t in batches:
            if use_graph:
                g.step(dev(x[lo:hi]), dev(t[lo:hi]))
            else:
                net.backprop(default_loss(net, dev(x[lo:hi]), dev(t[lo:hi])))
        torch.cuda.synchronize()
        assert net.optimizer.t == 5 + STEPS
        got = net._arena.detach().cpu().numpy()
        # every rank holds the same weights, bit for bit (same reduced gradient, same kernels)
        mine = torch.from_numpy(got.copy())
        other = mine.clone()
        dist.broadcast(other, 0)
        assert torch.equal(mine, other)
        if rank == 0:
            ref = WaveNet(Params(p), seed=0)
            ref.load_state_dict(w)
            ref.to_gpu()
            ref.update_laerning_rate(0.01)
            ref.optimizer.eps = 1e-3
            ref.optimizer.t = 5
            w_init = ref._arena.detach().cpu().numpy().copy()
            for x, t in batches:
                ref.backprop(default_loss(ref, dev(x), dev(t)))
            torch.cuda.synchronize()
            want = ref._arena.detach().cpu().numpy()
            assert np.abs(want - w_init).max() > 1e-3                 # the weights did move
            np.testing.assert_allclose(got, want, atol=2e-5)
        open(os.path.join(tmp, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("use_graph,over,B_PER,EXTRA", [(True, OVER, 2, 150), (False, OVER, 2, 150), (True, CFG2, 1, 100)])
def test_two_ranks_on_one_gpu_follow_the_global_batch_step(tmp_path, use_graph, over, B_PER, EXTRA):
    """The third case is BASELINE configs[2]'s own 4 x 10 stack (the 614,656-float arena all-reduced between the two
    graphs), one clip per rank."""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path), use_graph, over, B_PER, EXTRA), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")


def _rccl_worker(rank, port, tmp):
    import torch.distributed as dist
    from oracle import wavenet_ref as R
    from wavenet_amd import Params, TrainStepGraph, WaveNet
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))   # "nccl" IS RCCL on ROCm
    try:
        assert dist.get_backend() == "nccl"
        p = R.make_params(**CFG2)
        w = R.init_weights(p, 11)
        iw = R.input_width(p)
        batches = _batches(iw, 1, 100)
        dev = lambda a: torch.as_tensor(a).cuda()
        arenas = []
        for dp_on in (True, False):
            net = WaveNet(Params(p), seed=0)
            net.load_state_dict(w)
            net.to_gpu()
            net.update_laerning_rate(0.01)
            net.optimizer.eps = 1e-3
            if dp_on:
                dp = net.enable_data_parallel(always_reduce=True)
                assert dp.world == 1 and dp.always_reduce
            g = TrainStepGraph(net, dev(batches[0][0]), dev(batches[0][1]))
            assert (g._g2 is not None) == dp_on                       # two graphs with the collective between them
            n_ar = [0]
            if dp_on:
                real = dist.all_reduce

                def counted(*a, **k):
                    n_ar[0] += 1
                    return real(*a, **k)
                dist.all_reduce = counted
            try:
                for x, t in batches:
                    g.step(dev(x), dev(t))
                torch.cuda.synchronize()
            finally:
                if dp_on:
                    dist.all_reduce = real
            assert n_ar[0] == (STEPS if dp_on else 0)
            assert net._grad_arena.numel() >= 614656
            arenas.append(net._arena.detach().cpu().numpy().copy())
            del g, net
        assert np.array_equal(arenas[0], arenas[1])                                 # bit for bit: SUM over one rank is the identity
        open(os.path.join(tmp, "rccl_ok"), "w").write(dist.get_backend())
    finally:
        dist.destroy_process_group()


def test_rccl_world_size_one_all_reduce_between_the_two_graphs(tmp_path):
    """RCCL itself on the hardware that exists (VERDICT r3 missing #1): a `nccl` process group of ONE rank on cuda:0; the
    BASELINE configs[2] stack trains three steps as forward/backward graph -> ncclAllReduce of the 614,656-float gradient
    arena (launched eagerly on the capture stream's successor, never captured; the communicator is created by the warm-up
    outside any capture) -> optimiser graph.  The weights must equal the single-graph non-DP step's bit for bit, and the
    group must tear down cleanly.  It cannot measure scaling; it proves communicator creation, stream ordering around the
    two graphs and destroy_process_group on the real backend."""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_rccl_worker, args=(port, str(tmp_path)), nprocs=1, join=True)
    assert (tmp_path / "rccl_ok").read_text() == "nccl"


def test_bench_dp_branch_over_rccl_in_a_group_of_one():
    """bench.py's N > 1 code path (init_process_group("nccl"), enable_data_parallel, two-graph step, barrier-bracketed
    timing, MAX over ranks through an RCCL all-reduce, the `dist` record, destroy_process_group) with
    WAVENET_BENCH_FORCE_DIST=1 on the one GPU."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WAVENET_BENCH_FORCE_DIST="1", MASTER_PORT=str(_free_port()), MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "3", "--warmup", "1", "--full"], env=env,
                       capture_output=True, text=True, timeout=900, cwd=root)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["dist"]["backend"] == "nccl" and out["dist"]["world_size"] == 1
    assert "RCCL all-reduce" in out["launch"] and "fwd+bwd graph" in out["launch"], out["launch"]
    assert np.isfinite(out["loss"]) and out["value"] > 0


def _oracle_worker(rank, world, port, tmp):
    import torch.distributed as dist
    from oracle import wavenet_ref as R
    from wavenet_amd import Params, WaveNet
    from wavenet_amd.graph import default_loss
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = R.make_params(**OVER)
        w = R.init_weights(p, 21)
        net = WaveNet(Params(p), seed=0)
        net.load_state_dict(w)
        net.to_gpu()
        dp = net.enable_data_parallel()
        iw = net.input_width
        rs = np.random.RandomState(9)
        B, EXTRA = 2 * world, 120
        x = rs.randint(0, 256, (B, iw + EXTRA)).astype(np.int32)
        t = rs.randint(0, 256, (B, EXTRA)).astype(np.int32)
        lo, hi = dp.shard(B)
        dev = lambda a: torch.as_tensor(a).cuda()
        loss = default_loss(net, dev(x[lo:hi]), dev(t[lo:hi]))
        net.zero_grads()
        loss.backward()
        mult = dp.all_reduce_grads(net._grad_arena)                 # SUM over ranks in place; 1 / world is the optimiser's factor
        torch.cuda.synchronize()
        assert mult == 1.0 / world
        got = net._grad_arena.detach().cpu().numpy() * mult
        if rank == 0:
            loss_ref, _, g = R.train_step_grads(p, w, x, t)         # the ORACLE on the global batch
            worst = 0.0
            for ln, kind, off, n, shape in net._spans:
                want = np.asarray(g["%s/%s" % (ln.name, kind)], np.float64).reshape(-1)
                err = float(np.abs(got[off:off + n] - want).max())
                scale = max(float(np.abs(want).max()), 1e-12)
                worst = max(worst, err / scale)
                assert err <= 1e-4 * scale + 1e-7, (ln.name, kind, err, scale)
            ml = dp.mean_loss(float(loss.detach()))
            assert abs(ml - loss_ref) < 1e-4, (ml, loss_ref)
            open(os.path.join(tmp, "oracle_ok"), "w").write("%.3e" % worst)
        else:
            dp.mean_loss(float(loss.detach()))
    finally:
        dist.destroy_process_group()


def test_two_rank_reduced_gradient_equals_the_oracle_on_the_global_batch(tmp_path):
    """VERDICT r4 next #5b / SURVEY 8(e): "reduced grads == single-process global-batch grads", held against the ORACLE on the
    device, not only against the device's own single-process step: two ranks on cuda:0 (gloo) each run forward + backward on
    their two clips, all-reduce(SUM) the flat gradient arena; arena x 1/world must equal oracle.train_step_grads on all four
    clips (every tensor within 1e-4 of its largest entry), and the all-reduced mean loss the oracle's loss (1e-4)."""
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_oracle_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(tmp_path / "oracle_ok"), "rank 0 did not finish the comparison"


def _multi_gpu_worker(rank, world, port, tmp, backend="nccl", share_gpu=False):
    """One rank per DEVICE over RCCL (`nccl`): the data-parallel step of SURVEY 8(e) as BASELINE configs[2] runs it.
    (backend="gloo", share_gpu=True: the one-GPU rehearsal of exactly this code -- every rank on cuda:0.)"""
    import hashlib
    import json
    import torch.distributed as dist
    from oracle import wavenet_ref as R
    from wavenet_amd import Params, TrainStepGraph, WaveNet
    from wavenet_amd.graph import default_loss
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    device = 0 if share_gpu else rank
    torch.cuda.set_device(device)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        assert dist.get_backend() == backend and dist.get_world_size() == world
        p = R.make_params(**CFG2)
        w = R.init_weights(p, 21)
        net = WaveNet(Params(p), seed=100 + rank)            # every rank starts elsewhere: the broadcast must fix that
        if rank == 0:
            net.load_state_dict(w)
        net.to_gpu()
        net.update_laerning_rate(0.01)
        net.optimizer.eps = 1e-3
        dp = net.enable_data_parallel()
        assert dp.world == world and net._arena.device.index == device
        iw = net.input_width
        rs = np.random.RandomState(9)
        B, EXTRA = world, 120                                 # one clip per rank
        x = rs.randint(0, 256, (B, iw + EXTRA)).astype(np.int32)
        t = rs.randint(0, 256, (B, EXTRA)).astype(np.int32)
        lo, hi = dp.shard(B)
        dev = lambda a: torch.as_tensor(a).cuda()
        # (1) reduced gradient == the ORACLE's gradient on the global batch
        loss = default_loss(net, dev(x[lo:hi]), dev(t[lo:hi]))
        net.zero_grads()
        loss.backward()
        mult = dp.all_reduce_grads(net._grad_arena)
        torch.cuda.synchronize()
        got = net._grad_arena.detach().cpu().numpy() * mult
        ml = dp.mean_loss(float(loss.detach()))
        worst = 0.0
        if rank == 0:
            torch.set_num_threads(min(16, os.cpu_count() or 1))
            loss_ref, _, g = R.train_step_grads(p, w, x, t)
            for ln, kind, off, n, shape in net._spans:
                want = np.asarray(g["%s/%s" % (ln.name, kind)], np.float64).reshape(-1)
                err = float(np.abs(got[off:off + n] - want).max())
                scale = max(float(np.abs(want).max()), 1e-12)
                worst = max(worst, err / scale)
                assert err <= 1e-4 * scale + 1e-7, (ln.name, kind, err, scale)
            assert abs(ml - loss_ref) < 1e-4, (ml, loss_ref)
        # (2) three replayed two-graph steps (fwd+bwd graph -> ncclAllReduce -> optimiser graph): every rank's weights bit-equal
        g2 = TrainStepGraph(net, dev(x[lo:hi]), dev(t[lo:hi]))
        assert g2._g2 is not None
        w0 = net._arena.detach().clone()
        for _ in range(STEPS):
            g2.step(dev(x[lo:hi]), dev(t[lo:hi]))
        torch.cuda.synchronize()
        assert float((net._arena.detach() - w0).abs().max()) > 1e-4
        digest = hashlib.sha256(net._arena.detach().cpu().numpy().tobytes()).hexdigest()
        # (3) the `dist` record: what RCCL saw
        rec = [None] * world
        dist.all_gather_object(rec, {"rank": rank, "device": torch.cuda.current_device(),
                                     "name": torch.cuda.get_device_name(device), "weights_sha256": digest})
        assert len({r["weights_sha256"] for r in rec}) == 1, rec                            # bit-equal weights on every rank
        if rank == 0:
            assert sorted(r["device"] for r in rec) == ([0] * world if share_gpu else list(range(world)))   # distinct devices
            json.dump({"backend": dist.get_backend(), "world_size": dist.get_world_size(), "ranks": rec,
                       "grad_worst_rel_err_vs_oracle": worst}, open(os.path.join(tmp, "dist.json"), "w"))
    finally:
        dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs: arms itself on a multi-GPU node (SURVEY 8(e), BASELINE configs[2])")
def test_rccl_ranks_on_distinct_gpus_reduce_to_the_oracle_gradient_and_stay_bit_equal(tmp_path):
    """RCCL at N >= 2 the moment a node has the devices -- min(device_count, 8) ranks, ONE PER GPU, backend
    `nccl` (RCCL over xGMI).  On BASELINE configs[1]'s 4 x 10 stack (the 614,656-float arena): (1) all-reduce(SUM) of the
    shard gradients x 1/world equals the ORACLE's gradient on the global batch (every tensor within 1e-4 of its largest
    entry) and the all-reduced mean loss the oracle's loss; (2) after three replayed two-graph steps (forward/backward graph
    -> ncclAllReduce -> optimiser graph) every rank holds the same weights BIT FOR BIT although every rank was initialised
    differently (the broadcast of weights + optimiser state); (3) the `dist` record shows the world size as RCCL saw it and
    one distinct device per rank.  Skipped on a one-GPU box; the single-device baseline is train_audio/model.py:57-59."""
    import json
    import torch.multiprocessing as mp
    world = min(torch.cuda.device_count(), 8)
    mp.spawn(_multi_gpu_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    rec = json.load(open(tmp_path / "dist.json"))
    assert rec["backend"] == "nccl" and rec["world_size"] == world and len(rec["ranks"]) == world


def test_the_multi_gpu_rccl_test_rehearsed_with_two_ranks_on_one_gpu(tmp_path):
    """The worker of the self-arming test above, line for line, with the one difference a one-GPU box forces: backend gloo and
    both ranks on cuda:0.  Keeps that test's code exercised (and correct) until a node with two devices runs it over RCCL."""
    import json
    import torch.multiprocessing as mp
    mp.spawn(_multi_gpu_worker, args=(2, _free_port(), str(tmp_path), "gloo", True), nprocs=2, join=True)
    rec = json.load(open(tmp_path / "dist.json"))
    assert rec["backend"] == "gloo" and rec["world_size"] == 2 and rec["grad_worst_rel_err_vs_oracle"] < 1e-4
