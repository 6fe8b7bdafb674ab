"""The exponential moving average of the weights without a GPU: the schedule, the checkpoint files, the command-line flags,
and the ABI it arrived through (rule 6 of wn_rule_step: no new export)."""
import os
import re

import numpy as np
import pytest

from wavenet_amd import Params, WaveNet, _lib
from wavenet_amd.ema import ema_decay_at, ema_rate_at
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import evaluate as cli_evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TINY = {"quantization_steps": 256, "residual_conv_channels": [8, 8], "residual_num_blocks": 1, "causal_conv_channels": [8],
         "softmax_conv_channels": [16, 256]}


def test_schedule_warms_up_from_one_tenth_and_stays_at_decay():
    assert ema_decay_at(0, 0.9999, True) == 0.1                       # (1 + 0) / (10 + 0): TensorFlow's num_updates rule
    assert ema_decay_at(1, 0.9999, True) == 2.0 / 11.0
    # (1 + t) / (10 + t) = decay at t = (10 decay - 1) / (1 - decay): 81/90, 8991/9000, 89991/90000
    for decay, reached in ((0.9, 80), (0.999, 8990), (0.9999, 89990)):
        d = [ema_decay_at(t, decay, True) for t in range(100000 if decay > 0.999 else 10000)]
        assert all(b >= a for a, b in zip(d, d[1:]))                  # monotone
        first = next(t for t in range(len(d)) if (1.0 + t) / (10.0 + t) >= decay)
        assert first == reached                                       # decay from there on, the ramp before it
        assert all(x == decay for x in d[first:]) and all(x < decay for x in d[:first])
        assert all(d[t] == (1.0 + t) / (10.0 + t) for t in range(first))
    assert [ema_decay_at(t, 0.97, False) for t in (0, 1, 10, 10 ** 6)] == [0.97] * 4
    # what the kernel gets: 1 - decay_t in float64, rounded to fp32 once
    r = ema_rate_at(3, 0.9999, True)
    assert isinstance(r, np.float32) and r == np.float32(1.0 - 4.0 / 13.0)
    assert ema_rate_at(10 ** 6, 0.9999, True) == np.float32(1.0 - 0.9999)
    with pytest.raises(ValueError):
        ema_decay_at(-1, 0.9)


def test_enable_disable_and_reconfigure_keep_the_average():
    net = WaveNet(Params(_TINY), seed=0)
    assert not net.ema_enabled
    with pytest.raises(Exception, match="enable_ema"):
        with net.ema_weights():
            pass
    net.enable_ema()
    assert net.ema_enabled and net._ema_t == 0 and (net._ema_decay, net._ema_warmup) == (0.9999, True)
    assert net._ema_arena.data_ptr() != net._arena.data_ptr() and np.array_equal(net._ema_arena.numpy(), net._arena.numpy())
    net._ema_arena += 0.5
    net._ema_t = 7
    keep = net._ema_arena.numpy().copy()
    net.enable_ema(0.99, warmup=False)                                # other numbers: the average and its clock stay
    assert (net._ema_decay, net._ema_warmup, net._ema_t) == (0.99, False, 7) and np.array_equal(net._ema_arena.numpy(), keep)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            net.enable_ema(bad)
    net.disable_ema()
    assert not net.ema_enabled and net._ema_arena is None


def test_ema_weights_swaps_contents_not_pointers_on_the_host():
    net = WaveNet(Params(_TINY), seed=0)
    net.enable_ema(0.9)
    net._ema_arena.mul_(0.5)
    w, e = net._arena.numpy().copy(), net._ema_arena.numpy().copy()
    pw, pe = net._arena.data_ptr(), net._ema_arena.data_ptr()
    raw = net.state_dict()
    with net.ema_weights():
        assert (net._arena.data_ptr(), net._ema_arena.data_ptr()) == (pw, pe)
        assert np.array_equal(net._arena.numpy(), e) and np.array_equal(net._ema_arena.numpy(), w)
        inside = net.state_dict()
        avg = net.ema_state_dict()                                    # the average, wherever it sits just now
        for k in raw:
            assert np.array_equal(inside[k], avg[k]) and np.array_equal(inside[k], raw[k] * np.float32(0.5))
        with pytest.raises(Exception, match="ema_weights"):
            net.backprop(None)
        with pytest.raises(Exception, match="nest"):
            with net.ema_weights():
                pass
        with pytest.raises(Exception, match="ema_weights"):
            net.save("unused")
    assert np.array_equal(net._arena.numpy(), w) and np.array_equal(net._ema_arena.numpy(), e)
    with pytest.raises(RuntimeError, match="boom"):                   # an exception inside still puts the weights back
        with net.ema_weights():
            raise RuntimeError("boom")
    assert np.array_equal(net._arena.numpy(), w) and not net._ema_swapped


def test_checkpoint_round_trip_of_the_average(tmp_path, capsys):
    d = str(tmp_path / "m")
    a = WaveNet(Params(_TINY), seed=0)
    a.enable_ema(0.95, warmup=False)
    a._ema_arena += torch_randn_like(a._ema_arena, 3)
    a._ema_t = 41
    a.save(d)
    assert os.path.isfile(os.path.join(d, "wavenet.ema.npz"))
    sd = a.ema_state_dict()
    assert set(sd) == set(a.state_dict()) | {"ema/t", "ema/decay", "ema/warmup"}
    b = WaveNet(Params(_TINY), seed=1)
    b.enable_ema()                                                    # other numbers: the file's win
    b.load(d)
    assert np.array_equal(b._arena.numpy(), a._arena.numpy()) and np.array_equal(b._ema_arena.numpy(), a._ema_arena.numpy())
    assert (b._ema_t, b._ema_decay, b._ema_warmup) == (41, 0.95, False)
    assert not np.array_equal(b._ema_arena.numpy(), b._arena.numpy())
    # weights="ema": the average as the model's weights, no average kept
    c = WaveNet(Params(_TINY), seed=2)
    c.load(d, weights="ema")
    got = c.state_dict()
    for k in got:
        assert np.array_equal(got[k], sd[k])
    assert not c.ema_enabled
    with pytest.raises(ValueError):
        c.load(d, weights="both")
    capsys.readouterr()
    # enabled, but the checkpoint has no average: it starts again from the weights just loaded, and says so
    os.remove(os.path.join(d, "wavenet.ema.npz"))
    e = WaveNet(Params(_TINY), seed=3)
    e.enable_ema(0.9)
    e._ema_t = 9
    e.load(d)
    assert e._ema_t == 0 and np.array_equal(e._ema_arena.numpy(), a._arena.numpy())
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if "wavenet.ema.npz" in ln]) == 1 and "starts again" in out
    with pytest.raises(FileNotFoundError, match="no averaged weights"):
        c.load(d, weights="ema")


def test_without_the_average_save_and_load_are_what_they_were(tmp_path, capsys):
    d = str(tmp_path / "m")
    a = WaveNet(Params(_TINY), seed=0)
    a.save(d)
    assert "wavenet.ema.npz" not in os.listdir(d)
    # a stray file (of another model, even) is ignored
    np.savez(os.path.join(d, "wavenet.ema.npz"), **{"ema/t": np.array(3), "junk": np.zeros(2)})
    b = WaveNet(Params(_TINY), seed=1)
    b.load(d)
    assert not b.ema_enabled and np.array_equal(b._arena.numpy(), a._arena.numpy())
    assert "wavenet.ema.npz" not in capsys.readouterr().out
    b.save(d)
    with np.load(os.path.join(d, "wavenet.ema.npz")) as z:
        assert sorted(z.files) == ["ema/t", "junk"]                   # not rewritten either


def torch_randn_like(t, seed):
    import torch
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(t.shape).astype(np.float32))


def test_new_flags_parse_and_default_to_off():
    a = cli_args.parse([])
    assert (a.ema_decay, a.valid_wav_dir, a.ema) == (0.0, None, False)
    a = cli_args.parse(["--ema-decay", "0.999", "--valid-wav-dir", "held_out", "--ema"])
    assert (a.ema_decay, a.valid_wav_dir, a.ema) == (0.999, "held_out", True)
    for bad in ("1.0", "-0.5", "nan"):
        with pytest.raises(SystemExit):
            cli_args.parse(["--ema-decay", bad])
    ap = cli_evaluate.build_parser()
    assert ap.parse_args(["--ema"]).ema is True
    # off = absent: train_audio.model.build reads both with a default, and what a command line without them parses to is
    # what it parsed to before they existed
    off = ap.parse_args([])
    assert getattr(off, "ema", False) is False and getattr(off, "ema_decay", 0.0) == 0.0
    assert not {"ema", "ema_decay", "valid_wav_dir"} & (set(vars(off)) | set(vars(cli_args.parse([]))))


def test_rule_six_arrived_without_a_new_export():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))) == 69 == len(_lib.EXPORTS)
    assert int(re.search(r"\bWN_RULE_EMA\s*=\s*(\d+)", hdr).group(1)) == 6 == _lib.WN_RULE_EMA
    assert int(re.search(r"\bWN_RULE_RMSPROP\s*=\s*(\d+)", hdr).group(1)) == 5
