"""The exponential moving average of the weights on the GPU: rule 6 of wn_rule_step through the raw C ABI, then
WaveNet.enable_ema through backprop, TrainStepGraph, data parallelism, ema_weights() and the train / evaluate / generate
commands."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:                                            # the two-rank worker below runs this file as a program
        sys.path.insert(0, _p)

import json                                                           # noqa: E402

import numpy as np                                                    # noqa: E402
import pytest                                                         # noqa: E402
import torch                                                          # noqa: E402

from oracle import wavenet_ref as R                                   # noqa: E402
from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, WaveNet, _lib, data      # noqa: E402
from wavenet_amd.ema import ema_decay_at                              # noqa: E402
from wavenet_amd.graph import default_loss                            # noqa: E402
from gpu_util import build, dev, to_np                                # noqa: E402

pytestmark = pytest.mark.gpu

EMA = _lib.WN_RULE_EMA
U = 2.0 ** -24                                                        # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------
# the raw C ABI
# ---------------------------------------------------------------------------------------------
def rule_step(rule, p, g, s1=None, s2=None, lr=0.0, lr_dev=None, hyper=0.0, eps=0.0, wd=0.0, sqnorm=None, clip=0.0, gmult=1.0,
              n=None):
    ptr = _lib.ptr
    return _lib.lib().wn_rule_step(rule, ptr(p), ptr(g), ptr(s1), ptr(s2), p.numel() if n is None else n, float(lr), ptr(lr_dev),
                                   hyper, eps, wd, ptr(sqnorm), clip, gmult, _lib.stream_ptr())


def restate(e, w, r):
    """(float64 e + float64(r) (w - e), the bound 2 * 2^-24 * max(|e|, |w|, |e_new|) per element): one rounding of the
    difference and one of the result -- or of the two terms of (e - r e) + r w, which are no larger."""
    e64, w64 = e.astype(np.float64), w.astype(np.float64)
    new = e64 + float(np.float32(r)) * (w64 - e64)
    return new, 2 * U * np.maximum(np.maximum(np.abs(e64), np.abs(w64)), np.abs(new))


_GUARD = 8                                                            # floats around each array that no launch may touch


def _arrays(n, off_e, off_w, seed=0):
    """e and w as n-float views that start ``off`` floats past a 16-byte boundary, inside buffers with sentinels around them."""
    rs = np.random.RandomState(seed + n)
    he, hw = rs.standard_normal(n).astype(np.float32), rs.standard_normal(n).astype(np.float32)
    be = torch.full((n + 2 * _GUARD,), 777.0, device="cuda")
    bw = torch.full((n + 2 * _GUARD,), 555.0, device="cuda")
    assert be.data_ptr() % 16 == 0 and bw.data_ptr() % 16 == 0
    e, w = be[_GUARD + off_e:_GUARD + off_e + n], bw[_GUARD + off_w:_GUARD + off_w + n]
    e.copy_(torch.from_numpy(he))
    w.copy_(torch.from_numpy(hw))
    assert e.data_ptr() % 16 == 4 * off_e and w.data_ptr() % 16 == 4 * off_w

    def untouched():
        b, c = to_np(be), to_np(bw)
        return (np.all(b[:_GUARD + off_e] == 777.0) and np.all(b[_GUARD + off_e + n:] == 777.0) and
                np.all(c[:_GUARD + off_w] == 555.0) and np.all(c[_GUARD + off_w + n:] == 555.0) and
                np.array_equal(c[_GUARD + off_w:_GUARD + off_w + n], hw))
    return he, hw, e, w, untouched


# 1, 3: below one float4; 4: exactly one; 5, 1027: the tails; 524,289: one element past one grid of 2048 x 256 threads;
# 614,656: BASELINE config 2's arena
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 524289, 614656])
@pytest.mark.parametrize("off_e,off_w", [(0, 0), (1, 0), (0, 1)])
def test_one_step_against_a_float64_restatement(n, off_e, off_w):
    for r in (np.float32(0.1), np.float32(0.9), np.float32(1.0 - 0.9999)):
        he, hw, e, w, untouched = _arrays(n, off_e, off_w)
        assert rule_step(EMA, e, w, lr=r) == 0, _lib.lib().wn_last_error()
        torch.cuda.synchronize()
        want, bound = restate(he, hw, r)
        err = np.abs(to_np(e).astype(np.float64) - want)
        worst = float((err / bound).max())
        print("n=%d offsets (%d, %d) r=%.6g: max err / bound = %.3f" % (n, off_e, off_w, r, worst))
        assert np.all(err <= bound), worst
        assert untouched()                                            # w read only, nothing outside the n floats written


@pytest.mark.parametrize("n,off", [(5, 0), (1027, 1), (614656, 0)])
def test_rate_by_value_and_through_device_memory_are_bit_identical(n, off):
    r = np.float32(1.0 - ema_decay_at(3, 0.9999, True))
    he, hw, e1, w1, _ = _arrays(n, off, 0)
    _, _, e2, w2, _ = _arrays(n, off, 0)
    rd = torch.full((1,), float(r), device="cuda")
    assert rule_step(EMA, e1, w1, lr=r) == 0
    assert rule_step(EMA, e2, w2, lr=123.0, lr_dev=rd) == 0            # `lr` is ignored, whatever it holds
    assert torch.equal(e1, e2) and not np.array_equal(to_np(e1), he)


@pytest.mark.parametrize("n,off_e,off_w", [(3, 0, 0), (1027, 0, 0), (1027, 1, 0), (1027, 0, 1), (524289, 0, 0)])
def test_rate_zero_keeps_the_average_and_rate_one_copies_the_weights(n, off_e, off_w):
    he, hw, e, w, untouched = _arrays(n, off_e, off_w)
    assert rule_step(EMA, e, w, lr=0.0) == 0
    assert np.array_equal(to_np(e).view(np.uint32), he.view(np.uint32))
    assert rule_step(EMA, e, w, lr=1.0) == 0
    assert np.array_equal(to_np(e).view(np.uint32), hw.view(np.uint32))
    assert untouched()


@pytest.mark.parametrize("n,off", [(1027, 0), (1027, 1)])
def test_a_non_finite_norm_skips_and_a_large_one_does_not_scale(n, off):
    he, hw, e, w, _ = _arrays(n, off, 0)
    nrm = torch.zeros((_lib.SQNORM_WORDS,), device="cuda")
    for bad in (float("inf"), float("nan")):
        nrm[0] = bad
        assert rule_step(EMA, e, w, lr=0.25, sqnorm=nrm, clip=1.0) == 0
        assert np.array_equal(to_np(e).view(np.uint32), he.view(np.uint32))
    nrm[0] = 1e6                                                      # norm 1000, far above clip: an optimiser would scale by 1e-3
    assert rule_step(EMA, e, w, lr=0.25, sqnorm=nrm, clip=1.0) == 0
    want, bound = restate(he, hw, 0.25)
    assert np.all(np.abs(to_np(e).astype(np.float64) - want) <= bound)
    # clip <= 0: the word is not read at all, as for every rule
    nrm[0] = float("nan")
    h2 = to_np(e).copy()
    assert rule_step(EMA, e, w, lr=0.25, sqnorm=nrm, clip=0.0) == 0
    want, bound = restate(h2, hw, 0.25)
    assert np.all(np.abs(to_np(e).astype(np.float64) - want) <= bound) and not np.array_equal(to_np(e), h2)


def test_refusals_come_before_any_device_work():
    he, hw, e, w, untouched = _arrays(64, 0, 0)
    E = _lib.WN_EARG
    assert rule_step(EMA, e, w, lr=0.1, wd=1e-3) == E
    assert rule_step(EMA, e, w, lr=0.1, gmult=0.5) == E
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        assert rule_step(EMA, e, w, lr=bad) == E, bad
    assert b"[0, 1]" in _lib.lib().wn_last_error()
    s = torch.zeros((64,), device="cuda")
    assert rule_step(7, e, w, s1=s, s2=s, lr=0.1) == E
    assert rule_step(-1, e, w, s1=s, s2=s, lr=0.1) == E
    assert rule_step(EMA, e, w, lr=0.1, n=0) == E
    torch.cuda.synchronize()
    assert np.array_equal(to_np(e), he) and untouched()
    assert rule_step(EMA, e, w, s1=None, s2=None, lr=0.1) == 0        # no state arrays: accepted
    assert rule_step(5, e, w, s1=None, lr=0.1) == E                   # ... by this rule only
    assert not np.array_equal(to_np(e), he)


@pytest.mark.parametrize("rule,name,eps", [(0, "sgd", 0.0), (1, "momentumsgd", 0.0), (2, "adagrad", 1e-8), (3, "adadelta", 1e-6),
                                           (4, "nesterov", 0.0), (5, "rmsprop", 1e-8)])
def test_rules_zero_to_five_still_reach_their_own_kernels(rule, name, eps):
    """The routing switch: each optimiser rule twice on identical inputs -- equal to each other bit for bit -- and against the
    oracle's restatement of the Chainer rule, two steps, at the existing rule test's tolerance."""
    n, lr, hyper = 1027, 0.01, 0.8
    rs = np.random.RandomState(rule)
    P = (rs.standard_normal(n) * 0.1).astype(np.float32)
    S1, S2 = np.zeros_like(P), np.zeros_like(P)
    runs = [[dev(P.copy()), dev(S1.copy()), dev(S2.copy())] for _ in range(2)]
    for _ in range(2):
        g = (rs.standard_normal(n) * 0.02).astype(np.float32)
        for p, s1, s2 in runs:
            assert rule_step(rule, p, dev(g), s1=s1, s2=s2, lr=lr, hyper=hyper, eps=eps) == 0
        R.rule_step_ref(name, P, g, S1, S2, lr, hyper)
        for a, b in zip(*runs):
            assert torch.equal(a, b)
        np.testing.assert_allclose(to_np(runs[0][0]), P, rtol=0, atol=3e-6)
        if rule != 0:
            np.testing.assert_allclose(to_np(runs[0][1]), S1, rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------------------------
# the Python face
# ---------------------------------------------------------------------------------------------
TINY = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 3, residual_num_blocks=2,
            softmax_conv_channels=[64, 256])
B, TW = 2, 64


def _net(seed=7, ema=None, cls=WaveNet):
    p, w, net = build(TINY, seed=seed, cls=cls)                       # gradient clipping 1.0: the skip guard is armed
    net.update_laerning_rate(0.01)
    if ema is not None:
        net.enable_ema(*ema)
    return net


def _batches(net, k, seed=0):
    rs = np.random.RandomState(seed)
    T = net.input_width + TW
    return [(dev(rs.randint(0, 256, (B, T)).astype(np.int32)), dev(rs.randint(0, 256, (B, TW)).astype(np.int32)))
            for _ in range(k)]


def _follow(net, step, batches, decay, warmup):
    """Run ``step`` on every batch; after each, advance a float64 host average from the weights read back.  Returns the
    largest |device - host| and the bound k * 2^-23 * max|w| (two roundings of 2^-24 max per step)."""
    host = to_np(net._ema_arena).astype(np.float64)
    w0 = to_np(net._arena).copy()
    wmax = 0.0
    for t, (x, tgt) in enumerate(batches):
        step(x, tgt)
        w = to_np(net._arena).astype(np.float64)
        r = float(np.float32(1.0 - ema_decay_at(t, decay, warmup)))    # the rate the kernel is handed
        host += r * (w - host)
        wmax = max(wmax, float(np.abs(w).max()), float(np.abs(host).max()))
    got = to_np(net._ema_arena)
    assert np.abs(to_np(net._arena) - w0).max() > 1e-3                # the weights moved,
    assert not np.array_equal(got, w0) and not np.array_equal(got, to_np(net._arena))   # and the average lags behind them
    return float(np.abs(got.astype(np.float64) - host).max()), len(batches) * 2.0 ** -23 * wmax


def test_eager_steps_follow_the_schedule():
    net = _net(ema=(0.9, True))
    assert net._ema_arena.is_cuda and torch.equal(net._ema_arena, net._arena)
    err, bound = _follow(net, lambda x, t: net.backprop(default_loss(net, x, t)), _batches(net, 6), 0.9, True)
    print("eager: max |device - host| = %.3g, bound %.3g" % (err, bound))
    assert err <= bound and net._ema_t == 6 and net.last_update_applied()


def test_enable_before_to_gpu_moves_the_average_with_the_weights():
    p = R.make_params(**TINY)
    net = WaveNet(Params(p), seed=3)
    net.enable_ema(0.5, warmup=False)
    net.to_gpu()
    net.update_laerning_rate(0.01)
    assert net._ema_arena.device == net._arena.device and net._ema_arena.data_ptr() != net._arena.data_ptr()
    w0 = to_np(net._arena).astype(np.float64)
    x, t = _batches(net, 1)[0]
    net.backprop(default_loss(net, x, t))
    want = w0 + 0.5 * (to_np(net._arena).astype(np.float64) - w0)
    assert np.abs(to_np(net._ema_arena) - want).max() <= 2.0 ** -23 * np.abs(w0).max()


def test_a_skipped_optimiser_step_is_a_skipped_averaging_step():
    net = _net(ema=(0.9, True))
    x, t = _batches(net, 1)[0]
    net.backprop(default_loss(net, x, t))
    w, e = net._arena.clone(), net._ema_arena.clone()
    assert not torch.equal(w, e)

    def void_loss():                                                  # a gradient that is no gradient: NaN in one tensor of the arena
        return net.causal_conv_layers[0].W.sum() * float("nan")

    net.backprop(void_loss)
    assert not net.last_update_applied()
    assert torch.equal(net._arena, w) and torch.equal(net._ema_arena, e)
    assert net._ema_t == 2                                            # the host clock advances all the same, like Adam's t


def test_graph_steps_follow_the_schedule_and_add_exactly_one_kernel_node():
    net = _net(ema=(0.9, True))
    batches = _batches(net, 6)
    net._ema_arena.mul_(0.75)                                         # an average that is not the weights: a warm-up trace would show
    net._ema_t = 0
    e0, w0 = net._ema_arena.clone(), net._arena.clone()
    g = TrainStepGraph(net, *batches[0], keep_graph=True)
    assert torch.equal(net._ema_arena, e0) and torch.equal(net._arena, w0) and net._ema_t == 0 and net.optimizer.t == 0
    err, bound = _follow(net, lambda x, t: g.step(x, t), batches, 0.9, True)
    print("graph: max |device - host| = %.3g, bound %.3g" % (err, bound))
    assert err <= bound and net._ema_t == 6
    off = _net()
    g_off = TrainStepGraph(off, *batches[0], keep_graph=True)
    assert g.node_counts()["kernel"] == g_off.node_counts()["kernel"] + 1
    # what was captured by value cannot change under the graph
    net.disable_ema()
    with pytest.raises(_lib.WaveNetHipError, match="captured"):
        g.step()
    off.enable_ema(0.9)
    with pytest.raises(_lib.WaveNetHipError, match="captured"):
        g_off.step()


def test_the_average_does_not_perturb_training():
    a, b = _net(seed=5), _net(seed=5, ema=(0.9999, True))
    batches = _batches(a, 5)
    ga, gb = TrainStepGraph(a, *batches[0]), TrainStepGraph(b, *batches[0])
    for x, t in batches:
        ga.step(x, t)
        gb.step(x, t)
    torch.cuda.synchronize()
    assert torch.equal(a._arena, b._arena) and torch.equal(a.optimizer.m, b.optimizer.m)
    assert torch.equal(a.optimizer.v, b.optimizer.v) and a.optimizer.t == b.optimizer.t == 5
    assert not torch.equal(b._ema_arena, b._arena)


def test_ema_weights_swaps_in_the_average_and_back():
    net = _net(ema=(0.9, True), cls=FasterWaveNet)
    for x, t in _batches(net, 3):
        net.backprop(default_loss(net, x, t))
    w, e = net._arena.clone(), net._ema_arena.clone()
    pw, pe = net._arena.data_ptr(), net._ema_arena.data_ptr()
    avg = net.ema_state_dict()
    u = np.random.RandomState(9).random_sample(8)
    raw_tokens = to_np(net.generate(8, u))                            # the decoder handle now holds the raw weights
    with net.ema_weights():
        assert (net._arena.data_ptr(), net._ema_arena.data_ptr()) == (pw, pe)
        sd = net.state_dict()
        assert all(np.array_equal(sd[k], avg[k]) for k in sd)
        with pytest.raises(_lib.WaveNetHipError, match="ema_weights"):
            net.backprop(default_loss(net, *_batches(net, 1)[0]))
        inside = to_np(net.generate(8, u))
    assert torch.equal(net._arena, w) and torch.equal(net._ema_arena, e)
    other = _net(seed=11, cls=FasterWaveNet)
    other.load_state_dict(avg)                                        # the average as a second model's weights
    assert np.array_equal(inside, to_np(other.generate(8, u)))
    assert np.array_equal(to_np(net.generate(8, u)), raw_tokens)      # and the first model decodes with its own again
    g = TrainStepGraph(net, *_batches(net, 1)[0])
    with net.ema_weights():
        with pytest.raises(_lib.WaveNetHipError, match="ema_weights"):
            g.step()


# ---------------------------------------------------------------------------------------------
# two ranks on cuda:0 over gloo (the worker runs this file as a program, one process per rank)
# ---------------------------------------------------------------------------------------------
DP_STEPS = 3


def _dp_worker(rank, world, port, tmp):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = R.make_params(**TINY)
        net = WaveNet(Params(p), seed=100 + rank)
        if rank == 0:
            net.load_state_dict(R.init_weights(p, 11))
            net.enable_ema(0.9, warmup=True)
            net._ema_arena.mul_(0.5)                                   # a resumed rank 0: average, clock and numbers must travel
            net._ema_t = 4
        else:
            net.enable_ema(0.5, warmup=False)
        net.to_gpu()
        net.update_laerning_rate(0.01)
        dp = net.enable_data_parallel()
        assert (net._ema_t, net._ema_decay, net._ema_warmup) == (4, 0.9, True)

        def same_everywhere(t):
            other = t.clone()
            dist.broadcast(other, 0)
            return torch.equal(t, other)

        assert same_everywhere(net._ema_arena) and not torch.equal(net._ema_arena, net._arena)
        rs = np.random.RandomState(3)
        T = net.input_width + TW
        batches = [(rs.randint(0, 256, (2 * B, T)).astype(np.int32), rs.randint(0, 256, (2 * B, TW)).astype(np.int32))
                   for _ in range(DP_STEPS)]
        lo, hi = dp.shard(2 * B)
        g = TrainStepGraph(net, dev(batches[0][0][lo:hi]), dev(batches[0][1][lo:hi]), keep_graph=True)
        assert g._g2 is not None and net._ema_t == 4
        e0 = net._ema_arena.clone()
        for x, t in batches:
            g.step(dev(x[lo:hi]), dev(t[lo:hi]))
        torch.cuda.synchronize()
        assert net._ema_t == 4 + DP_STEPS and not torch.equal(net._ema_arena, e0)
        assert same_everywhere(net._arena) and same_everywhere(net._ema_arena)
        # a rank whose average differs (rank 0 here: it is the source) brings every rank to its own
        if rank == 0:
            net._ema_arena.add_(0.25)
            net._ema_t = 17
        assert same_everywhere(net._ema_arena) == (rank == 0)
        dp.broadcast_weights(0)
        assert same_everywhere(net._ema_arena) and net._ema_t == 17
        open(os.path.join(tmp, "ok%d" % rank), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_keep_the_same_average(tmp_path):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "--dp-worker", str(rank),
                               "2", str(port), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rank in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], "\n".join(outs)
    assert os.path.exists(tmp_path / "ok0") and os.path.exists(tmp_path / "ok1")


# ---------------------------------------------------------------------------------------------
# the commands, end to end
# ---------------------------------------------------------------------------------------------
def test_train_evaluate_generate_with_the_average(tmp_path, capsys):
    from scipy.io import wavfile
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    from wavenet_amd.train_audio import generate as cli_generate
    from wavenet_amd.train_audio import train as cli_train
    wav, held, model, out = (str(tmp_path / d) for d in ("wav", "held", "model", "out"))
    for d in (wav, held, model):
        os.makedirs(d)
    sr = 8000
    wave = data.synthetic_waveform(2, 2 * sr, sr)                     # two seconds each: one to train on, one held out
    wavfile.write(os.path.join(wav, "a.wav"), sr, (wave[0] * 32767).astype(np.int16))
    wavfile.write(os.path.join(held, "b.wav"), sr, (wave[1] * 32767).astype(np.int16))
    cfg = Params(dict(TINY, sampling_rate=sr)).to_dict()
    with open(os.path.join(model, "wavenet.json"), "w") as f:
        json.dump(cfg, f)
    cli_train.main(["-w", wav, "-m", model, "--ema-decay", "0.9", "--valid-wav-dir", held, "--max-epoch", "2", "--repeat", "5",
                    "--batch-size", "2", "--train-width", "32", "--seed", "1"])
    printed = capsys.readouterr().out
    assert os.path.isfile(os.path.join(model, "wavenet.ema.npz"))
    lines = [ln for ln in printed.splitlines() if "held-out" in ln]
    assert len(lines) == 2 and "held-out weights:" in lines[0] and "held-out ema weights:" in lines[1], printed
    with np.load(os.path.join(model, "wavenet.ema.npz")) as z:
        assert int(z["ema/t"]) == 5 and float(z["ema/decay"]) == 0.9 and bool(z["ema/warmup"])
    # evaluate --ema == evaluate_dir under ema_weights() on the reloaded net
    table = cli_evaluate.main(["-w", held, "-m", model, "--ema"])
    net = WaveNet(Params(cfg), seed=0)
    net.enable_ema(0.9)
    net.load(model)
    net.to_gpu()
    assert net._ema_t == 5 and not torch.equal(net._arena, net._ema_arena)
    raw = cli_evaluate.evaluate_dir(net, net.params, held, verbose=False)
    with net.ema_weights():
        want = cli_evaluate.evaluate_dir(net, net.params, held, verbose=False)
    assert table == want and table["total"]["samples"] > 10000
    assert table["total"]["nats_per_sample"] != raw["total"]["nats_per_sample"]
    assert ("%.6f" % want["total"]["nats_per_sample"]) in lines[1] and ("%.6f" % raw["total"]["nats_per_sample"]) in lines[0]
    # generate --fast --ema
    fn, tokens = cli_generate.main(["-m", model, "-o", out, "--fast", "--ema", "-s", "0.01", "--seed", "2"])
    assert os.path.isfile(fn) and tokens.shape == (int(sr * 0.01) - 1,)
    # a checkpoint without the file
    os.remove(os.path.join(model, "wavenet.ema.npz"))
    with pytest.raises(SystemExit, match="no averaged weights"):
        cli_evaluate.main(["-w", held, "-m", model, "--ema"])
    with pytest.raises(SystemExit, match="no averaged weights"):
        cli_generate.main(["-m", model, "-o", out, "--fast", "--ema", "-s", "0.01"])


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--dp-worker":
        _dp_worker(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
