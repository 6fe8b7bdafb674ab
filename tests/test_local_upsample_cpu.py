"""The learned upsampling layer ahead of the local projection (``local_upsample``), everything that needs no GPU: the
constructor, the arena, the initial weight, the column counts, the float64 restatement of layer + alignment
(tests/local_upsample_ref.py), ``local.json``, the command line and the checkpoint messages."""
import json
import os

import numpy as np
import pytest
import torch

import local_cond_ref as LR
import local_interp_ref as LI
import local_upsample_ref as LU
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, WaveNet
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import local as cli_local
from wavenet_amd.train_audio import model as cli_model
from wavenet_amd.wavenet import coarse_frames_needed, frames_needed

F, H, T = LU.FEATS, LU.HOP, LU.T
KEY = "local_condition_upsample/W"


def _net(cls=WaveNet, seed=3, **kw):
    return cls(Params(R.make_params(**LR.TINY)), seed=seed, **kw)


# ---- the constructor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [WaveNet, FasterWaveNet])
def test_constructor_refusals(cls):
    with pytest.raises(Exception, match="local_upsample must be >= 1"):
        _net(cls, local_channels=F, local_hop=H, local_upsample=0)
    with pytest.raises(Exception, match="local_upsample = 5 does not divide local_hop = 12"):
        _net(cls, local_channels=F, local_hop=H, local_upsample=5)
    with pytest.raises(Exception, match="local_upsample = 3 needs local conditioning"):
        _net(cls, local_upsample=3)
    with pytest.raises(Exception, match="local conditioning is not available with storage='bf16'"):
        _net(cls, local_channels=F, local_hop=H, local_upsample=3, storage="bf16")
    assert _net(cls, local_channels=F, local_hop=H).local_upsample == 1
    assert _net(cls).local_upsample == 1
    net = _net(cls, local_channels=F, local_hop=H, local_upsample=3)
    assert (net.local_upsample, net.local_hop, net.local_fine_hop) == (3, 12, 4)


def test_the_new_tensor_is_last_and_nothing_else_moves():
    plain, one, up = _net(local_channels=F, local_hop=H), _net(local_channels=F, local_hop=H, local_upsample=1), \
        _net(local_channels=F, local_hop=H, local_upsample=3, local_interp="linear")
    keys = list(up.state_dict())
    assert keys[:-1] == list(plain.state_dict()) == list(one.state_dict())
    assert keys[-2:] == ["local_condition_projection/W", KEY]
    assert torch.equal(one._arena, plain._arena) and one._spans[-1][0].name == "local_condition_projection"
    n = plain._arena.numel()
    assert up._arena.numel() == n + (3 * F * 2 * F + 63) // 64 * 64
    assert torch.equal(up._arena[:n], plain._arena)                           # every other tensor: the same-seed U = 1 model's
    a, b = up.state_dict(), plain.state_dict()
    assert all(np.array_equal(a[k], b[k]) for k in b)
    assert a[KEY].shape == (3 * F, 2 * F, 1, 1) and a[KEY].dtype == np.float32
    assert up.num_parameters == plain.num_parameters + 3 * F * 2 * F
    glob = _net(local_channels=F, local_hop=H, local_upsample=2, condition_classes=3, condition_channels=8)
    assert list(glob.state_dict())[-3:] == ["global_condition_projection/W", "local_condition_projection/W", KEY]
    # the optimiser, the gradient arena and the weight average are sized by the arena: they cover the new tensor
    assert up._grad_arena.numel() == up.optimizer.m.numel() == up._arena.numel()
    assert up.local_condition_upsample.W.grad.data_ptr() == up._grad_arena[up._spans[-1][2]:].data_ptr()


@pytest.mark.parametrize("U", [2, 3, 12])
def test_the_initial_weight_entry_by_entry(U):
    w = _net(local_channels=F, local_hop=H, local_upsample=U).state_dict()[KEY].reshape(U * F, 2 * F)
    for q in range(U):
        a = np.float32(q) / np.float32(U)
        for c in range(F):
            for col in range(2 * F):
                want = np.float32(1) - a if col == c else (a if col == F + c else np.float32(0))
                assert w[q * F + c, col] == want, (q, c, col)
    assert np.array_equal(w, LU.initial_weight(U, F))
    assert np.array_equal(w[:F], np.concatenate([np.eye(F), np.zeros((F, F))], axis=1))     # q = 0: the coarse column itself
    # no draw: two seeds, one weight
    assert np.array_equal(w, _net(seed=9, local_channels=F, local_hop=H, local_upsample=U).state_dict()[KEY].reshape(U * F, 2 * F))


# ---- column counts ---------------------------------------------------------------------------------------------------------
def test_coarse_frames_needed_on_hand_made_cases():
    # H = 12, U = 3: H' = 4; phase 5 -> c0 = 1, phase' = 1; 70 positions read ceil(71 / 4) = 18 fine columns (19 linear) from
    # fine column 1 on: fine columns 0 .. 18 (19) -> ceil(19 / 3) + 1 = ceil(20 / 3) + 1 = 8
    assert coarse_frames_needed(70, 12, 3, 5, "repeat") == 8 and coarse_frames_needed(70, 12, 3, 5, "linear") == 8
    assert coarse_frames_needed(70, 12, 3, 5) == 8                               # ("repeat" is the default)
    # U = 12: H' = 1; phase 11, one position: fine column 11 (and 12 in linear mode) -> 2 and 3 coarse columns
    assert coarse_frames_needed(1, 12, 12, 11, "repeat") == 2 and coarse_frames_needed(1, 12, 12, 11, "linear") == 3
    assert coarse_frames_needed(1, 12, 12, 0, "repeat") == 2                      # a pair, always
    # the last fine column of a pair: phase 8 -> c0 = 2; 4 positions at phase' 0 read 1 fine column: 3 fine columns, one pair
    assert coarse_frames_needed(4, 12, 3, 8, "repeat") == 2 and coarse_frames_needed(5, 12, 3, 8, "repeat") == 3
    # a phase per clip: c0 = U - 1 = 2, phase' = 3: ceil(73 / 4) = 19 (20) -> ceil(21 / 3) + 1 = 8, ceil(22 / 3) + 1 = 9
    assert coarse_frames_needed(70, 12, 3, None, "repeat") == 8 and coarse_frames_needed(70, 12, 3, None, "linear") == 9
    assert coarse_frames_needed(70, 12, 3, None, "linear") == max(coarse_frames_needed(70, 12, 3, p, "linear") for p in range(12))
    # U = 1 is frames_needed, and frames_needed is what it was
    for interp in ("repeat", "linear"):
        for ph in (0, 5, 11):
            assert coarse_frames_needed(70, 12, 1, ph, interp) == frames_needed(70, 12, ph, interp)
        assert coarse_frames_needed(70, 12, 1, None, interp) == frames_needed(70, 12, 11, interp)
    assert frames_needed(70, 12, 5) == 7 and frames_needed(70, 12, 5, "linear") == 8 and frames_needed(70, 12) == 6
    # the restatement of the reference file agrees everywhere
    for U in (2, 3, 4, 6, 12):
        for interp in ("repeat", "linear"):
            for Tn in (1, 2, 11, 12, 13, 70):
                for ph in list(range(12)) + [None]:
                    assert coarse_frames_needed(Tn, 12, U, ph, interp) == LU.coarse_needed(Tn, 12, U, ph, interp)
    with pytest.raises(Exception, match="divide"):
        coarse_frames_needed(70, 12, 5, 0)
    with pytest.raises(Exception, match="interp"):
        coarse_frames_needed(70, 12, 3, 0, "cubic")


def test_too_few_columns_raise_before_any_device_work_and_name_the_counts():
    net = _net(local_channels=F, local_hop=H, local_upsample=3, local_interp="linear")
    h = np.zeros((3, F, 8), np.float32)
    feats, ph = net._local_features(h, 3, T, 5)                              # (the check itself needs no device)
    assert tuple(feats.shape) == (3, F, 8) and ph == 5
    with pytest.raises(Exception, match=r"holds 7 feature columns at hop 12, but 70 positions at phase 5 read 19 fine columns at "
                                        r"hop 4 from fine column 1 on \(local_upsample = 3\), which takes 8"):
        net._local_features(h[:, :, :7], 3, T, 5)
    with pytest.raises(Exception, match=r"holds 8 feature columns.*which takes 9 \(a phase per clip"):
        net._local_features(h, 3, T, [0, 5, 11])
    assert net._local_features(np.zeros((3, F, 20), np.float32), 3, T, [0, 5, 11])[1].hop == 12      # surplus: fine; phases stay in [0, H)
    with pytest.raises(Exception, match=r"must lie in \[0, local_hop = 12\), got 12"):
        net._local_features(h, 3, T, 12)


# ---- layer + alignment in float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", LU.PHASES)
@pytest.mark.parametrize("U", [2, 3, 4, 12])
def test_at_the_initial_weight_the_layer_is_linear_interpolation_at_the_coarse_hop(U, phase):
    """The float64 restatement of layer + cut + interpolation at hop H' against plain linear interpolation at hop H, position by
    position, to 1e-12 -- with the initial weight in exact arithmetic, that is with the quotient q / U formed in float64.
    The model's own float32 weight is that one rounded: q / U is exact in float32 for U = 2 and 4, where it passes the same
    1e-12; for U = 3 and 12 the coefficient a = q / U is off by at most half a float32 ulp of a number below 1, 2^-25, and
    1 - a by that plus the subtraction's own rounding, 2^-24 together: a fine column moves by at most 3 * 2^-25 * max |h|, and
    interpolating between two fine columns is a convex combination of them.  The bound asserted is 4 * 2^-25 * max |h|."""
    rs = np.random.RandomState(U)
    n = LU.coarse_needed(T, H, U, phase, "linear")
    h = rs.standard_normal((2, F, n))
    want = LU.lerp(h, H, phase, T)
    assert n >= LI.frames_needed(T, H, phase)                               # (the plain reference reads no column that is not there)
    exact = LU.layer_then_lerp(LU.initial_weight(U, F, np.float64), h, H, U, phase, T)
    assert np.abs(exact - want).max() <= 1e-12
    model_w = _net(local_channels=F, local_hop=H, local_upsample=U).state_dict()[KEY]
    got = LU.layer_then_lerp(model_w, h, H, U, phase, T)
    bound = 1e-12 if U in (2, 4) else 4 * 2.0 ** -25 * np.abs(h).max()
    assert np.abs(got - want).max() <= bound, (np.abs(got - want).max(), bound)
    # a random weight is something else, and the restated gradient is the adjoint of the restated layer
    W = LU.random_weight(U, F)
    y = LU.upsample(W, h)
    assert np.abs(LU.layer_then_lerp(W, h, H, U, phase, T) - want).max() > 0.1
    dy = rs.standard_normal(y.shape)
    dW, dh = LU.upsample_grads(W, h, dy)
    eps = 1e-6
    dir_W, dir_h = rs.standard_normal(W.shape), rs.standard_normal(h.shape)
    num = ((LU.upsample(W + eps * dir_W, h + eps * dir_h) - LU.upsample(W - eps * dir_W, h - eps * dir_h)) * dy).sum() / (2 * eps)
    assert abs(num - ((dW * dir_W).sum() + (dh * dir_h).sum())) <= 1e-6 * max(1.0, abs(num))


# ---- local.json and the command line ---------------------------------------------------------------------------------------
def test_local_json_round_trip_and_the_resumed_run(tmp_path):
    old, one, up, lin = (str(tmp_path / k) for k in ("old", "one", "up", "lin"))
    assert cli_local.load_upsample(old) is None
    cli_local.ensure_config(old, 80, 256)
    cli_local.ensure_config(one, 80, 256, None, 1)
    raw = open(os.path.join(old, "local.json"), "rb").read()
    assert raw == open(os.path.join(one, "local.json"), "rb").read() == b'{"channels": 80, "hop": 256}'     # U = 1: the file it always was
    assert cli_local.load_upsample(old) == 1
    assert cli_local.ensure_config(up, 80, 256, upsample=4) == (80, 256)
    with open(os.path.join(up, "local.json")) as f:
        assert json.load(f) == {"channels": 80, "hop": 256, "upsample": 4}
    assert cli_local.ensure_config(lin, 80, 256, "linear", 16) == (80, 256)
    with open(os.path.join(lin, "local.json")) as f:
        assert json.load(f) == {"channels": 80, "hop": 256, "interp": "linear", "upsample": 16}
    assert cli_local.load_upsample(up) == 4 and cli_local.load_upsample(lin) == 16 and cli_local.load_interp(lin) == "linear"
    assert cli_local.load_config(up) == (80, 256) and cli_local.load_interp(up) == "repeat"
    # resumed runs: no flag keeps the file's value, the same value passes, another one stops and names both
    assert cli_local.ensure_config(up, 80, 256) == (80, 256) and cli_local.ensure_config(up, 80, 256, upsample=4) == (80, 256)
    with pytest.raises(SystemExit, match="trained with --local-upsample 4, the command line gives 2"):
        cli_local.ensure_config(up, 80, 256, upsample=2)
    with pytest.raises(SystemExit, match="trained with --local-upsample 1, the command line gives 4"):
        cli_local.ensure_config(old, 80, 256, upsample=4)
    with pytest.raises(SystemExit, match="trained with --local-upsample 4, the command line gives 1"):
        cli_local.ensure_config(up, 80, 256, upsample=1)
    assert open(os.path.join(old, "local.json"), "rb").read() == raw
    with pytest.raises(SystemExit, match="divide the hop 256"):
        cli_local.ensure_config(str(tmp_path / "bad"), 80, 256, upsample=3)
    (tmp_path / "up" / "local.json").write_text('{"channels": 80, "hop": 256, "upsample": 3}')
    with pytest.raises(Exception, match="upsample"):
        cli_local.load_upsample(up)
    # the drivers repeat the last column: once for linear interpolation, once more for the layer's pairs
    f = np.arange(8, dtype=np.float32).reshape(2, 4)
    assert cli_local.with_extra_column(f, "repeat", 1) is f and cli_local.with_extra_column(f, "repeat") is f
    assert cli_local.with_extra_column(f, "linear").shape == (2, 5)
    g = cli_local.with_extra_column(f, "repeat", 4)
    assert g.shape == (2, 5) and np.array_equal(g[:, 4], f[:, 3])
    g = cli_local.with_extra_column(f, "linear", 4)
    assert g.shape == (2, 6) and np.array_equal(g[:, :4], f) and np.array_equal(g[:, 4], f[:, 3]) and np.array_equal(g[:, 5], f[:, 3])
    # ... which is what n columns covering n * hop samples from phase 0 need
    for U in (2, 4, 12):
        for interp in ("repeat", "linear"):
            assert coarse_frames_needed(4 * 12, 12, U, 0, interp) == cli_local.with_extra_column(f, interp, U).shape[1]


def test_cli_local_upsample_argument(tmp_path):
    a = cli_args.parse([])
    assert a.local_upsample is None and "local_upsample" not in vars(a) and cli_args.Args.local_upsample is None
    assert cli_args.parse(["--local-dir", "feat", "--local-upsample", "4"]).local_upsample == 4
    for argv in (["--local-upsample", "4"], ["--local-dir", "feat", "--local-upsample", "0"]):
        with pytest.raises(SystemExit):
            cli_args.parse(argv)
    d, w, fd = tmp_path / "m", tmp_path / "wav", tmp_path / "feat"
    for x in (d, w, fd):
        x.mkdir()
    (d / "wavenet.json").write_text(json.dumps(dict(LR.TINY)))
    (w / "a.wav").write_bytes(b"")
    np.save(str(fd / "a.npy"), np.zeros((5, 40), np.float32))
    base = ["-g", "-1", "-m", str(d), "-w", str(w), "--local-dir", str(fd), "--local-hop", "12"]
    with pytest.raises(Exception, match="not supported"):                    # (no CPU mode: the build stops at the device)
        cli_model.build(cli_args.parse(base + ["--local-upsample", "3"]), train=True)
    assert cli_local.load_config(str(d)) == (5, 12) and cli_local.load_upsample(str(d)) == 3
    with pytest.raises(SystemExit, match="same value"):
        cli_model.build(cli_args.parse(base + ["--local-upsample", "4"]), train=True)
    with pytest.raises(Exception, match="not supported"):                    # no flag: the file's value
        cli_model.build(cli_args.parse(base), train=True)
    assert cli_local.load_upsample(str(d)) == 3
    # generate / evaluate read the value from the checkpoint: the model they build holds the layer
    built = {}
    keep = cli_model.WaveNet

    class Spy(keep):
        def __init__(self, *a, **k):
            built.update(k)
            super().__init__(*a, **k)
    cli_model.WaveNet = Spy
    try:
        with pytest.raises(Exception, match="not supported"):
            cli_model.build(cli_args.parse(["-g", "-1", "-m", str(d)]))
    finally:
        cli_model.WaveNet = keep
    assert built["local_upsample"] == 3 and built["local_hop"] == 12 and built["local_channels"] == 5


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_checkpoint_mismatches_name_both_values(tmp_path):
    one, three, four = (_net(local_channels=F, local_hop=H, local_upsample=U) for U in (1, 3, 4))
    plain = _net()
    with pytest.raises(Exception, match="checkpoint was trained with local_upsample = 3 .*model is built with local_upsample = 1"):
        one.load_state_dict(three.state_dict())
    with pytest.raises(Exception, match="checkpoint was trained with local_upsample = 1 .*model is built with local_upsample = 3"):
        three.load_state_dict(one.state_dict())
    with pytest.raises(Exception, match="checkpoint was trained with local_upsample = 4 .*model is built with local_upsample = 3"):
        three.load_state_dict(four.state_dict())
    with pytest.raises(Exception, match="locally conditioned .* and the model is not"):
        plain.load_state_dict(three.state_dict())
    sd = three.state_dict()
    sd[KEY] = sd[KEY] + 1
    three.load_state_dict(sd)
    assert np.array_equal(three.state_dict()[KEY], sd[KEY])
    # through the files
    three.enable_ema(0.5)
    three.save(str(tmp_path))
    again = _net(seed=5, local_channels=F, local_hop=H, local_upsample=3)
    again.enable_ema(0.5)
    again.load(str(tmp_path))
    assert np.array_equal(again.state_dict()[KEY], sd[KEY]) and np.array_equal(again.ema_state_dict()[KEY], sd[KEY])
    with pytest.raises(Exception, match="local_upsample = 3 .*local_upsample = 4"):
        four.load(str(tmp_path))
    with pytest.raises(Exception, match="local_upsample = 3 .*local_upsample = 1"):
        one.load(str(tmp_path), weights="ema")
