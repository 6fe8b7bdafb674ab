"""Local conditioning without a GPU: the CPU reference against the per-clip reference, the model's new link behind all
others, argument and checkpoint errors, the header's trailing fields, the log-mel features, local.json and the command line."""
import json
import os
import re

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, WaveNet, _lib, features
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import local as cli_local
from wavenet_amd.train_audio import model as cli_model
from wavenet_amd.wavenet import frames_needed, local_alignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_with_one_frame_per_clip_is_the_per_clip_reference_exactly():
    """hop >= T + phase: every position reads row 0 of its clip, and the reference must then BE cond_ref's per-clip one.  In
    float64 -- the precision both serve as targets in -- every layer's out, z, tanh, sigmoid and the skip sum are equal bit
    for bit.  (In float32 torch's convolution-with-bias and convolution-then-add round differently: there the two agree to
    float32 rounding, 4e-6, which is checked too.)"""
    p = R.make_params(**LR.TINY)
    w = R.init_weights(p, 1234)
    rs = np.random.RandomState(0)
    x = rs.standard_normal((LR.B, 32, 1, LR.T)).astype(np.float32)
    bias = (rs.standard_normal((LR.B, cond_ref.cond_rows(p)[1])) * 0.5).astype(np.float32)
    for hop, phase in ((LR.T, 0), (LR.T + 9, 9), (1000, 123)):
        a = cond_ref.stack_forward(p, w, x, bias)
        b = LR.stack_forward(p, w, x, bias[:, None, :], hop, phase)
        for l in range(6):
            for k in range(4):
                assert np.array_equal(a[0][l][k], b[0][l][k]), (hop, l, k)
        assert np.array_equal(a[1], b[1]) and a[2] == b[2]
    a = cond_ref.stack_forward(p, w, x, bias, dtype=torch.float32)
    b = LR.stack_forward(p, w, x, bias[:, None, :], LR.T, 0, dtype=torch.float32)
    assert max(np.abs(a[0][l][k] - b[0][l][k]).max() for l in range(6) for k in range(4)) <= 4e-6


def test_reference_reads_the_frame_of_each_position_and_nothing_below_the_zero_prefix():
    """A block that is zero except frame f changes the gates' pre-activations exactly on the positions of frame f that lie at
    or above the layer's zero prefix."""
    p = R.make_params(**LR.TINY)
    w = R.init_weights(p, 1234)
    net = LR.LocalRefWaveNet(p, w, dtype=torch.float64)
    n = LR.frames_needed(LR.T, LR.HOP, LR.PHASE)
    assert n == 7
    for f in (0, 3, 6):
        rows = torch.zeros((1, n, cond_ref.cond_rows(p)[1]), dtype=torch.float64)
        rows[0, f] = 1.0
        net.set_rows(rows, LR.HOP, LR.PHASE)
        for _, _, d, pre in net.layers():
            bf, bg = net.gate_bias(pre, d, LR.T)
            Z = R.conv_pad_and_prefix(LR.T, d, 2)[1]
            want = np.array([1.0 if (t + LR.PHASE) // LR.HOP == f and t >= Z else 0.0 for t in range(LR.T)])
            assert np.array_equal(bf[0, 0, 0].numpy(), want) and np.array_equal(bg[0, 5, 0].numpy(), want), (f, pre)


# ---- the model -------------------------------------------------------------------------------------------------------------
def test_the_new_link_sits_last_and_nothing_else_moves():
    p = Params(R.make_params(**LR.TINY))
    plain, glob = WaveNet(p, seed=5), WaveNet(p, seed=5, condition_classes=3, condition_channels=8)
    loc = WaveNet(p, seed=5, local_channels=5, local_hop=12)
    both = WaveNet(p, seed=5, condition_classes=3, condition_channels=8, local_channels=5, local_hop=12)
    for base, more in ((plain, loc), (glob, both)):
        n = base._arena.numel()
        assert [(ln.name, k, o, m) for ln, k, o, m, _ in base._spans] == [(ln.name, k, o, m) for ln, k, o, m, _ in more._spans[:-1]]
        assert torch.equal(base._arena, more._arena[:n])                    # same offsets, same seeded draws
        assert more.num_parameters == base.num_parameters + 384 * 5
        assert list(more.state_dict())[-1] == "local_condition_projection/W"
        assert more.state_dict()["local_condition_projection/W"].shape == (384, 5, 1, 1)
        assert [ln.name for ln in more.links()][-1] == "local_condition_projection"
    assert loc._cond_offsets == [(64 * l, 64 * l + 32) for l in range(6)] and loc._cond_rows == 384
    assert plain.local_channels == 0 and not any(k.startswith("local_condition") for k in plain.state_dict())
    assert set(FasterWaveNet(p, seed=0, local_channels=5, local_hop=12).state_dict()) == set(loc.state_dict())
    assert not any("local" in k for k in Params().to_dict())                # constructor arguments, not Params fields


def test_constructor_argument_and_checkpoint_errors():
    p = Params(R.make_params(**LR.TINY))
    for kw in (dict(local_channels=5), dict(local_hop=12), dict(local_channels=-1, local_hop=-1)):
        with pytest.raises(Exception, match="local_channels > 0 and local_hop > 0"):
            WaveNet(p, seed=0, **kw)
    pw = Params(R.make_params(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 2,
                              residual_num_blocks=1, softmax_conv_channels=[256, 256]))
    with pytest.raises(Exception, match="bf16"):
        WaveNet(pw, seed=0, storage="bf16", local_channels=5, local_hop=12)
    pb = Params(R.make_params(**dict(LR.TINY, residual_conv_dilation_no_bias=False)))
    with pytest.raises(Exception, match="residual_conv_dilation_no_bias"):
        WaveNet(pb, seed=0, local_channels=5, local_hop=12)
    plain, loc = WaveNet(p, seed=0), WaveNet(p, seed=0, local_channels=5, local_hop=12)
    with pytest.raises(Exception, match="checkpoint is locally conditioned"):
        plain.load_state_dict(loc.state_dict())
    with pytest.raises(Exception, match="model is locally conditioned and the checkpoint is not"):
        loc.load_state_dict(plain.state_dict())
    # local=: a locally conditioned model needs features, any other refuses them; shape, dtype, phase and count are checked
    h = np.zeros((3, 5, 7), np.float32)
    with pytest.raises(Exception, match="pass local="):
        loc._local_features(None, 3, 70)
    with pytest.raises(Exception, match="no local conditioning"):
        plain._local_features(h, 3, 70)
    with pytest.raises(Exception, match="no local conditioning"):
        plain._local_features(None, 3, 70, 2)
    assert plain._local_features(None, 3, 70) == (None, 0)
    with pytest.raises(Exception, match=r"local_phase= must lie in \[0, local_hop = 12\)"):
        loc._local_features(h, 3, 70, 12)
    with pytest.raises(Exception, match="must be float32 of shape"):
        loc._local_features(h[:, :4], 3, 70, 5)
    with pytest.raises(Exception, match="must be float32 of shape"):
        loc._local_features(torch.zeros((3, 5, 7), dtype=torch.float64), 3, 70, 5)
    with pytest.raises(Exception, match="holds 6 feature columns, but 70 positions at hop 12 and phase 5 read 7"):
        loc._local_features(h[:, :, :6], 3, 70, 5)
    f, ph = loc._local_features(np.zeros((3, 5, 9), np.float32), 3, 70, 5)   # surplus columns are ignored
    assert tuple(f.shape) == (3, 5, 9) and ph == 5


def test_checkpoint_files_round_trip_the_projection_on_the_host(tmp_path):
    p = Params(R.make_params(**LR.TINY))
    a = WaveNet(p, seed=1, local_channels=5, local_hop=12)
    a.save(str(tmp_path))
    b = WaveNet(p, seed=2, local_channels=5, local_hop=12)
    k = "local_condition_projection/W"
    assert not np.array_equal(a.state_dict()[k], b.state_dict()[k])
    b.load(str(tmp_path))
    for key, v in a.state_dict().items():
        assert np.array_equal(v, b.state_dict()[key]), key
    with pytest.raises(Exception, match="locally conditioned"):
        WaveNet(p, seed=2).load(str(tmp_path))


def test_alignment_helper():
    """s0 -> (first column, phase): position t of the clip reads column (s0 + t) // H."""
    assert local_alignment(0, 256) == (0, 0) and local_alignment(255, 256) == (0, 255) and local_alignment(256, 256) == (1, 0)
    assert local_alignment(1000, 12) == (83, 4)
    for s0 in (0, 5, 11, 12, 29):
        col, ph = local_alignment(s0, 12)
        for t in (0, 1, 6, 7, 40):
            assert col + (t + ph) // 12 == (s0 + t) // 12
    with pytest.raises(Exception):
        local_alignment(3, 0)
    with pytest.raises(Exception):
        local_alignment(-1, 12)
    assert frames_needed(70, 12, 5) == 7 and frames_needed(72, 12, 0) == 6 and frames_needed(1, 12, 11) == 1


# ---- the header ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_trailing_fields_which_default_to_zero():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()

    def fields(name):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip()
                for part in decl.strip().split(",")]
    assert fields("WnStackDesc")[-3:] == ["bias_hop", "bias_phase", "bias_frame_stride"]
    assert fields("WnDecoderDesc")[-5:] == ["frame_bias", "n_frames", "frame_hop", "frame_phase", "frame_stride"]
    assert fields("WnStackDesc") == [f[0] for f in _lib.WnStackDesc._fields_]
    assert fields("WnDecoderDesc") == [f[0] for f in _lib.WnDecoderDesc._fields_]
    d, e = _lib.WnStackDesc(), _lib.WnDecoderDesc()
    assert (d.bias_hop, d.bias_phase, d.bias_frame_stride) == (0, 0, 0)
    assert (e.frame_bias, e.n_frames, e.frame_hop, e.frame_phase, e.frame_stride) == (None, 0, 0, 0, 0)
    assert re.findall(r"^#define\s+WN_ABI_VERSION\s+(\d+)", hdr, flags=re.M) == ["5"]
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))) == 69
    assert len(re.findall(r"^#define\s+WN_EXEC_\w+\s+\d+u", hdr, flags=re.M)) == 6


def test_frame_geometry_is_refused_without_a_gpu():
    """The descriptor checks come before any device work: they answer on a machine without a device."""
    import ctypes
    lib = _lib.lib()
    L = 2
    w = (ctypes.c_void_p * L)(0x1000, 0x2000)          # never dereferenced: every call below is refused first
    cd, dil = (ctypes.c_int * L)(32, 32), (ctypes.c_int * L)(1, 2)
    p = 0x3000

    def call(hop, phase, stride, flags, reserved, T=64):
        d = _lib.WnStackDesc(n_layers=L, Cr=32, Cs=256, fw=2, cd=cd, dilation=dil, Wf=w, Wg=w, Wp=w, Ws=w, bf=w, bg=w,
                             bias_hop=hop, bias_phase=phase, bias_frame_stride=stride)
        ex = _lib.WnExec(precision=0, flags=flags, reserved=reserved)
        rc = lib.wn_stack_fwd(ctypes.byref(d), p, p + 64, p, None, None, None, 1, T, 0, 0, 0, ctypes.byref(ex), None)
        return rc, lib.wn_last_error()
    for args_, word in (((-1, 0, 64, 2, 640), b"bias_hop"), ((12, 12, 64, 2, 640), b"bias_phase"), ((12, 0, 31, 2, 640), b"bias_frame_stride"),
                        ((12, 0, 64, 2, 6 * 64 - 1), b"reserved"), ((12, 0, 64, 0, 640), b"without WN_EXEC_BIAS_PER_CLIP")):
        rc, msg = call(*args_)
        assert rc == _lib.WN_EARG and word in msg, (args_, msg)
    # the kernels form t + phase in 32 bits: a T and a phase whose sum does not fit are refused, not wrapped
    rc, msg = call(2 ** 31 - 1, 100, 64, 2, 2 ** 31 - 1, T=2 ** 31 - 50)
    assert rc == _lib.WN_EARG and b"does not fit 32 bits" in msg, msg


# ---- features --------------------------------------------------------------------------------------------------------------
def _log_mel_direct(x, rate, n_mels, hop, win):
    """The definition restated with a direct O(N^2) DFT and explicit loops."""
    x = np.asarray(x, np.float64)
    N = x.size
    half = win // 2
    padded = np.concatenate([x[1:half + 1][::-1], x, x[-half - 1:-1][::-1]])
    n = (N + hop - 1) // hop
    k = np.arange(half + 1)
    out = np.zeros((n_mels, n))
    pts = 700.0 * (10.0 ** (np.linspace(0.0, 2595.0 * np.log10(1.0 + rate / 2.0 / 700.0), n_mels + 2) / 2595.0) - 1.0)
    for f in range(n):
        seg = padded[f * hop:f * hop + win] * (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win))
        dft = np.exp(-2j * np.pi * np.outer(k, np.arange(win)) / win) @ seg
        mag = np.abs(dft)
        for i in range(n_mels):
            acc = 0.0
            for b in range(half + 1):
                fr = b * rate / win
                wgt = max(0.0, min((fr - pts[i]) / (pts[i + 1] - pts[i]), (pts[i + 2] - fr) / (pts[i + 2] - pts[i + 1])))
                acc += wgt * mag[b]
            out[i, f] = np.log(max(acc, 1e-5))
    return out


def test_log_mel_shape_rule_and_a_direct_dft_restatement():
    rs = np.random.RandomState(3)
    for N, hop, want in ((600, 256, 3), (512, 256, 2), (513, 256, 3), (600, 64, 10), (2000, 256, 8)):
        m = features.log_mel(rs.standard_normal(N), 8000, n_mels=80 if N == 2000 else 12, hop=hop, win=256 if N < 2000 else 1024)
        assert m.shape == (80 if N == 2000 else 12, want) and m.dtype == np.float32 and want == (N + hop - 1) // hop
    x = rs.standard_normal(600) * 0.1 + np.sin(np.arange(600) * 0.3)
    got = features.log_mel(x, 8000, n_mels=10, hop=100, win=128)
    want = _log_mel_direct(x, 8000, 10, 100, 128)
    assert got.shape == want.shape == (10, 6)
    # both are log values of order 1: 1e-5 relative to the largest entry, plus float32 storage of the result
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert features.log_mel(np.zeros(300), 8000, n_mels=4, hop=100, win=64).max() == np.float32(np.log(1e-5))   # the floor


# ---- local.json and the command line -----------------------------------------------------------------------------------------
def test_local_json_round_trip_and_a_resumed_run_must_find_the_same_values(tmp_path):
    d = str(tmp_path / "model")
    assert cli_local.load_config(d) is None
    assert cli_local.ensure_config(d, 80, 256) == (80, 256)
    with open(os.path.join(d, "local.json")) as f:
        assert json.load(f) == {"channels": 80, "hop": 256}
    assert cli_local.load_config(d) == (80, 256) and cli_local.ensure_config(d, 80, 256) == (80, 256)
    for ch, hop in ((40, 256), (80, 128)):
        with pytest.raises(SystemExit, match="same values"):
            cli_local.ensure_config(d, ch, hop)
    assert not os.path.exists(os.path.join(d, "wavenet.json"))
    (tmp_path / "model" / "local.json").write_text("{broken")
    with pytest.raises(Exception, match="could not load"):
        cli_local.load_config(d)
    with pytest.raises(SystemExit, match="give --local FILE.npy"):
        cli_local.require_match((80, 256), False, "generate", "--local FILE.npy")
    with pytest.raises(SystemExit, match="not locally conditioned"):
        cli_local.require_match(None, True, "generate", "--local FILE.npy")
    cli_local.require_match(None, False, "generate", "--local FILE.npy")
    # the silence training puts in front of a file reads column 0
    f = np.arange(12, dtype=np.float32).reshape(2, 6)
    ext, shift = cli_local.padded(f, 13, 4)
    assert ext.shape == (2, 10) and shift == 3 and np.array_equal(ext[:, :4], np.repeat(f[:, :1], 4, axis=1)) and np.array_equal(ext[:, 4:], f)
    assert (13 + shift) % 4 == 0 and (13 + shift) // 4 == 4                  # the file's sample 0 reads the file's column 0


def test_feature_files_are_checked_by_name(tmp_path):
    fd = tmp_path / "feat"
    fd.mkdir()
    np.save(str(fd / "a.npy"), np.zeros((5, 4), np.float32))
    assert cli_local.file_features(str(fd), "x/a.wav", 48, 5, 12).shape == (5, 4)
    with pytest.raises(SystemExit, match=r"a\.npy has 4 columns, but the 49 samples of a\.wav need 5"):
        cli_local.file_features(str(fd), "a.wav", 49, 5, 12)
    with pytest.raises(SystemExit, match=r"b\.npy is missing"):
        cli_local.file_features(str(fd), "b.wav", 10, 5, 12)
    with pytest.raises(SystemExit, match="has 5 feature channels, the model takes 80"):
        cli_local.file_features(str(fd), "a.wav", 10, 80, 12)
    np.save(str(fd / "c.npy"), np.zeros((5,), np.float32))
    with pytest.raises(SystemExit, match=r"c\.npy must hold a float \(F, frames\) array"):
        cli_local.file_features(str(fd), "c.wav", 10, 5, 12)
    assert cli_local.directory_channels(str(fd), ["a.wav", "b.wav"]) == 5


def test_cli_argument_errors_and_defaults(tmp_path):
    a = cli_args.parse([])
    assert (a.local_dir, a.local_hop, a.local) == (None, None, None)
    assert not any(k.startswith("local") for k in vars(a))                   # attributes of the namespace only when given
    a = cli_args.parse(["--local-dir", "feat", "--local-hop", "128"])
    assert (a.local_dir, a.local_hop) == ("feat", 128)
    a = cli_args.parse(["--utterances", "2", "--local", "a.npy", "--local", "b.npy"])
    assert a.local == ["a.npy", "b.npy"]
    for argv in (["--local-hop", "128"], ["--local-dir", "feat", "--local-hop", "0"],
                 ["--utterances", "3", "--local", "a.npy", "--local", "b.npy"]):
        with pytest.raises(SystemExit):
            cli_args.parse(argv)
    # model.build: local.json decides whether the network is locally conditioned (checked up to the device, which this box lacks)
    d = tmp_path / "m"
    d.mkdir()
    (d / "wavenet.json").write_text(json.dumps(dict(LR.TINY)))
    w, fd = tmp_path / "wav", tmp_path / "feat"
    w.mkdir()
    fd.mkdir()
    for fn in ("a.wav", "b.wav"):
        (w / fn).write_bytes(b"")
    np.save(str(fd / "a.npy"), np.zeros((5, 40), np.float32))
    a = cli_args.parse(["-g", "-1", "-m", str(d), "-w", str(w), "--local-dir", str(fd), "--local-hop", "12"])
    with pytest.raises(Exception, match="not supported"):
        cli_model.build(a, train=True)
    assert cli_local.load_config(str(d)) == (5, 12)
    with open(str(d / "wavenet.json")) as f:
        assert set(json.load(f)) == set(LR.TINY)                             # wavenet.json is unchanged
    a = cli_args.parse(["-g", "-1", "-m", str(d), "-w", str(w), "--local-dir", str(fd), "--local-hop", "16"])
    with pytest.raises(SystemExit, match="same values"):
        cli_model.build(a, train=True)
    from wavenet_amd.train_audio import evaluate, generate, train
    with pytest.raises(SystemExit, match="give --local FILE.npy"):
        generate.main(["-g", "-1", "-m", str(d)])
    with pytest.raises(SystemExit, match="has 5 feature channels|is missing"):
        generate.main(["-g", "-1", "-m", str(d), "--local", str(fd / "nothing.npy")])
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "wavenet.json").write_text(json.dumps(dict(LR.TINY)))
    with pytest.raises(SystemExit, match="not locally conditioned"):
        generate.main(["-g", "-1", "-m", str(plain), "--local", str(fd / "a.npy")])
