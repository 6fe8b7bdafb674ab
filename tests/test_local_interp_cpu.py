"""Linear interpolation between feature frames without a GPU: the float64 reference's gradients against central differences,
``frames_needed``, constructor and command-line errors, the ``local.json`` round trip, the library's refusals (which answer
before any device work) and the header."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import cond_ref
import local_cond_ref as LR
import local_interp_ref as LI
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, WaveNet, _lib
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import local as cli_local
from wavenet_amd.train_audio import model as cli_model
from wavenet_amd.wavenet import frames_needed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ---------------------------------------------------------------------------------------------------------
def test_reference_weights_and_the_rows_each_position_reads():
    j, al = LI.weights(LI.T, LI.HOP, LI.PHASE)
    assert al.dtype == np.float32 and j[0] == 0 and al[0] == np.float32(5) / np.float32(12)
    assert j[6] == 0 and j[7] == 1 and al[7] == 0.0 and j[-1] == 6 and al[-1] == np.float32(2) / np.float32(12)
    assert LI.frames_needed(LI.T, LI.HOP, LI.PHASE) == 8
    # a block that is zero except row f: positions of frame f carry 1 - alpha, those of frame f - 1 carry alpha, below Z nothing
    p = R.make_params(**LI.TINY)
    net = LI.LinearRefWaveNet(p, R.init_weights(p, 1234), dtype=torch.float64)
    for f in (0, 3, 7):
        rows = torch.zeros((1, 8, cond_ref.cond_rows(p)[1]), dtype=torch.float64)
        rows[0, f] = 1.0
        net.set_rows(rows, LI.HOP, LI.PHASE)
        for _, _, d, pre in net.layers():
            bf, bg = net.gate_bias(pre, d, LI.T)
            Z = R.conv_pad_and_prefix(LI.T, d, 2)[1]
            want = np.array([0.0 if t < Z else (1.0 - float(al[t])) if j[t] == f else float(al[t]) if j[t] == f - 1 else 0.0
                             for t in range(LI.T)])
            assert np.array_equal(bf[0, 0, 0].numpy(), want) and np.array_equal(bg[0, 5, 0].numpy(), want), (f, pre)


def test_reference_with_equal_neighbours_is_the_repeat_reference_exactly():
    """a + alpha (b - a) with b == a is a: rows that are equal within a clip give the per-frame reference bit for bit."""
    p = R.make_params(**LI.TINY)
    w = R.init_weights(p, 1234)
    rs = np.random.RandomState(0)
    x = rs.standard_normal((LI.B, 32, 1, LI.T)).astype(np.float32)
    row = (rs.standard_normal((LI.B, 1, cond_ref.cond_rows(p)[1])) * 0.5).astype(np.float32)
    a = LR.stack_forward(p, w, x, np.repeat(row, 7, axis=1), LI.HOP, LI.PHASE)
    b = LI.stack_forward(p, w, x, np.repeat(row, 8, axis=1), LI.HOP, LI.PHASE)
    for l in range(6):
        for k in range(4):
            assert np.array_equal(a[0][l][k], b[0][l][k]), (l, k)
    assert np.array_equal(a[1], b[1])


def test_reference_gradients_against_central_differences():
    """The reference's own gradients in float64 -- of the rows (stack objective) and of V, h and a weight (training loss) --
    against central differences.  The objective is smooth; with step e = 1e-6 on values of order 1 the truncation error is
    ~e^2 and the rounding error ~1e-16 / e = 1e-10 relative to the objective, so 1e-6 of the largest gradient entry bounds
    both with a wide margin."""
    p = R.make_params(**LI.TINY)
    w = R.init_weights(p, 1234)
    rs = np.random.RandomState(3)
    Bn, Tn, hop, phase, t_off = 2, 23, 6, 4, 7
    n = LR.frames_needed(Tn, hop, phase) + 1
    Rw = cond_ref.cond_rows(p)[1]
    x = rs.standard_normal((Bn, 32, 1, Tn))
    rows = rs.standard_normal((Bn, n, Rw)) * 0.5
    dout = rs.standard_normal((Bn, 32, 1, Tn))
    dskip = rs.standard_normal((Bn, p["softmax_conv_channels"][0], 1, Tn - t_off))
    g = LI.stack_row_grads(p, w, x, rows, hop, phase, dout, dskip, t_off)
    assert g.shape == rows.shape and np.abs(g[:, -1]).max() > 0            # the extra row takes part

    def objective(r):
        net = LI.LinearRefWaveNet(p, w, dtype=torch.float64).set_rows(torch.tensor(r), hop, phase)
        with torch.no_grad():
            out, skip = net.forward_residual_block(torch.tensor(x))
            return float((out * torch.tensor(dout)).sum() + (skip[:, :, :, t_off:] * torch.tensor(dskip)).sum())
    e = 1e-6
    scale = np.abs(g).max()
    for b, f, c in [(0, 0, 0), (1, n - 1, 40), (0, 2, 33), (1, 1, 200), (0, n - 1, 383), (1, 3, 100)]:
        hi, lo = rows.copy(), rows.copy()
        hi[b, f, c] += e
        lo[b, f, c] -= e
        fd = (objective(hi) - objective(lo)) / (2 * e)
        assert abs(fd - g[b, f, c]) <= 1e-6 * scale, (b, f, c, fd, g[b, f, c])
    # the whole model: V, h and one weight
    V, h = LR.init_local(p, frames=n, seed=5, clips=Bn)
    V, h = V.astype(np.float64), h.astype(np.float64)
    idx = rs.randint(0, 256, (Bn, Tn)).astype(np.int32)
    tgt = rs.randint(0, 256, (Bn, Tn - 15)).astype(np.int32)
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    loss, _, grads = LI.train_step_grads(p, w64, V, h, hop, phase, idx, tgt, dtype=torch.float64)
    key = "residual_0_block_1_wf/W"
    for name, arr, pos in (("V", V, (3, 2)), ("V", V, (380, 4)), ("h", h, (1, 2, n - 1)), ("h", h, (0, 0, 0)),
                           (key, w64[key], np.unravel_index(301, w64[key].shape))):
        def at(delta):
            a2 = arr.copy()
            a2[pos] += delta
            ww = dict(w64, **{key: a2}) if name == key else w64
            return LI.train_step_grads(p, ww, a2 if name == "V" else V, a2 if name == "h" else h, hop, phase, idx, tgt,
                                       dtype=torch.float64)[0]
        fd = (at(e) - at(-e)) / (2 * e)
        sc = np.abs(grads[name]).max()
        assert sc > 0 and abs(fd - grads[name][pos]) <= 1e-6 * sc + 1e-10, (name, pos, fd, grads[name][pos])


# ---- the model -------------------------------------------------------------------------------------------------------------
def test_frames_needed_and_constructor_errors():
    assert frames_needed(70, 12, 5) == 7 and frames_needed(70, 12, 5, "repeat") == 7 and frames_needed(70, 12, 5, "linear") == 8
    assert frames_needed(72, 12, 0, "linear") == 7 and frames_needed(1, 12, 11, "linear") == 2 and frames_needed(5, 1, 0, "linear") == 6
    with pytest.raises(Exception, match="'repeat' or 'linear'"):
        frames_needed(70, 12, 5, "cubic")
    p = Params(R.make_params(**LI.TINY))
    for cls in (WaveNet, FasterWaveNet):
        assert cls(p, seed=0, local_channels=5, local_hop=12).local_interp == "repeat"
        lin = cls(p, seed=0, local_channels=5, local_hop=12, local_interp="linear")
        assert lin.local_interp == "linear" and (lin.local_channels, lin.local_hop) == (5, 12)
        with pytest.raises(Exception, match="'repeat' or 'linear'"):
            cls(p, seed=0, local_channels=5, local_hop=12, local_interp="nearest")
        with pytest.raises(Exception, match="needs local conditioning"):
            cls(p, seed=0, local_interp="linear")
        assert cls(p, seed=0).local_interp == "repeat"
    rep, lin = WaveNet(p, seed=3, local_channels=5, local_hop=12), WaveNet(p, seed=3, local_channels=5, local_hop=12, local_interp="linear")
    assert torch.equal(rep._arena, lin._arena) and list(rep.state_dict()) == list(lin.state_dict())     # the mode adds no weight
    h = np.zeros((3, 5, 8), np.float32)
    assert tuple(lin._local_features(h, 3, 70, 5)[0].shape) == (3, 5, 8)
    rep._local_features(h[:, :, :7], 3, 70, 5)
    with pytest.raises(Exception, match=r"holds 7 feature columns, but 70 positions at hop 12 and phase 5 read 8 \(linear interpolation"):
        lin._local_features(h[:, :, :7], 3, 70, 5)


# ---- local.json and the command line -----------------------------------------------------------------------------------------
def test_local_json_keeps_a_repeat_file_as_it_was_and_a_resumed_run_must_find_the_same_mode(tmp_path):
    rep, lin, old = str(tmp_path / "rep"), str(tmp_path / "lin"), str(tmp_path / "old")
    assert cli_local.load_interp(rep) is None
    cli_local.ensure_config(old, 80, 256)
    cli_local.ensure_config(rep, 80, 256, "repeat")
    raw = open(os.path.join(rep, "local.json"), "rb").read()
    assert raw == open(os.path.join(old, "local.json"), "rb").read() == b'{"channels": 80, "hop": 256}'
    assert cli_local.load_interp(rep) == "repeat" and cli_local.load_config(rep) == (80, 256)
    assert cli_local.ensure_config(lin, 80, 256, "linear") == (80, 256)
    with open(os.path.join(lin, "local.json")) as f:
        assert json.load(f) == {"channels": 80, "hop": 256, "interp": "linear"}
    assert cli_local.load_interp(lin) == "linear" and cli_local.load_config(lin) == (80, 256)
    # resumed runs: no flag keeps the file's mode, the same mode passes, the other one stops with a message
    assert cli_local.ensure_config(lin, 80, 256) == (80, 256) and cli_local.ensure_config(lin, 80, 256, "linear") == (80, 256)
    assert cli_local.ensure_config(rep, 80, 256, "repeat") == (80, 256)
    with pytest.raises(SystemExit, match="trained with --local-interp linear, the command line gives repeat"):
        cli_local.ensure_config(lin, 80, 256, "repeat")
    with pytest.raises(SystemExit, match="trained with --local-interp repeat, the command line gives linear"):
        cli_local.ensure_config(rep, 80, 256, "linear")
    assert open(os.path.join(rep, "local.json"), "rb").read() == raw
    (tmp_path / "lin" / "local.json").write_text('{"channels": 80, "hop": 256, "interp": "cubic"}')
    with pytest.raises(Exception, match="interp"):
        cli_local.load_interp(lin)
    # the drivers supply the column behind the last by repeating it; file_features asks for no more than before
    f = np.arange(8, dtype=np.float32).reshape(2, 4)
    assert cli_local.with_extra_column(f, "repeat") is f and cli_local.with_extra_column(f, None) is f
    g = cli_local.with_extra_column(f, "linear")
    assert g.shape == (2, 5) and np.array_equal(g[:, :4], f) and np.array_equal(g[:, 4], f[:, 3])
    fd = tmp_path / "feat"
    fd.mkdir()
    np.save(str(fd / "a.npy"), np.zeros((5, 4), np.float32))
    assert cli_local.file_features(str(fd), "a.wav", 48, 5, 12).shape == (5, 4)


def test_cli_local_interp_argument(tmp_path):
    a = cli_args.parse([])
    assert a.local_interp is None and "local_interp" not in vars(a)
    a = cli_args.parse(["--local-dir", "feat", "--local-interp", "linear"])
    assert a.local_interp == "linear"
    for argv in (["--local-interp", "linear"], ["--local-dir", "feat", "--local-interp", "cubic"]):
        with pytest.raises(SystemExit):
            cli_args.parse(argv)
    # model.build: the mode goes to local.json with the first run, and a resumed run with the other mode stops
    d, w, fd = tmp_path / "m", tmp_path / "wav", tmp_path / "feat"
    for x in (d, w, fd):
        x.mkdir()
    (d / "wavenet.json").write_text(json.dumps(dict(LI.TINY)))
    (w / "a.wav").write_bytes(b"")
    np.save(str(fd / "a.npy"), np.zeros((5, 40), np.float32))
    base = ["-g", "-1", "-m", str(d), "-w", str(w), "--local-dir", str(fd), "--local-hop", "12"]
    with pytest.raises(Exception, match="not supported"):                    # (no CPU mode: the build stops at the device)
        cli_model.build(cli_args.parse(base + ["--local-interp", "linear"]), train=True)
    assert cli_local.load_config(str(d)) == (5, 12) and cli_local.load_interp(str(d)) == "linear"
    with pytest.raises(SystemExit, match="same mode"):
        cli_model.build(cli_args.parse(base + ["--local-interp", "repeat"]), train=True)
    with pytest.raises(Exception, match="not supported"):                    # no flag: the file's mode
        cli_model.build(cli_args.parse(base), train=True)
    assert cli_local.load_interp(str(d)) == "linear"


# ---- the library's refusals ------------------------------------------------------------------------------------------------
def test_interpolation_fields_are_refused_without_a_gpu():
    """The descriptor checks come before any device work: they answer on a machine without a device."""
    lib = _lib.lib()
    L = 2
    w = (ctypes.c_void_p * L)(0x1000, 0x2000)          # never dereferenced: every call below is refused first
    cd, dil = (ctypes.c_int * L)(32, 32), (ctypes.c_int * L)(1, 2)
    p = 0x3000

    def call(hop, phase, stride, interp, flags, reserved, T=64, bwd=False):
        d = _lib.WnStackDesc(n_layers=L, Cr=32, Cs=256, fw=2, cd=cd, dilation=dil, Wf=w, Wg=w, Wp=w, Ws=w, bf=w, bg=w,
                             bias_hop=hop, bias_phase=phase, bias_frame_stride=stride, bias_interp=interp)
        ex = _lib.WnExec(precision=0, flags=flags, reserved=reserved)
        if bwd:
            rc = lib.wn_stack_bwd(ctypes.byref(d), p, p, p, p, p, p, p, p, w, w, w, w, w, None, w, None, p, 1 << 20, 1, T, 0, 1,
                                  ctypes.byref(ex), None)
        else:
            rc = lib.wn_stack_fwd(ctypes.byref(d), p, p + 64, p, None, None, None, 1, T, 0, 0, 0, ctypes.byref(ex), None)
        return rc, lib.wn_last_error()
    for bwd in (False, True):
        for args_, word in (((12, 0, 64, 2, 2, 640), b"bias_interp"), ((12, 0, 64, -1, 2, 640), b"bias_interp"),
                            ((0, 0, 0, 1, 2, 64), b"without frames"),
                            ((12, 0, 64, 1, 2, 7 * 64 - 1), b"frames + 1")):           # 64 positions: 6 frames, 7 rows
            rc, msg = call(*args_, bwd=bwd)
            assert rc == _lib.WN_EARG and word in msg, (args_, bwd, msg)


def test_header_still_declares_69_functions_and_abi_5():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.findall(r"^#define\s+WN_ABI_VERSION\s+(\d+)", hdr, flags=re.M) == ["5"]
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))) == 69
    assert len(re.findall(r"^#define\s+WN_EXEC_\w+\s+\d+u", hdr, flags=re.M)) == 6
    # the mode sits at the head of each descriptor's local-conditioning group: the groups' own fields stay the trailing ones
    names, dnames = [f[0] for f in _lib.WnStackDesc._fields_], [f[0] for f in _lib.WnDecoderDesc._fields_]
    assert names[-4:] == ["bias_interp", "bias_hop", "bias_phase", "bias_frame_stride"]
    assert dnames[-6:] == ["frame_interp", "frame_bias", "n_frames", "frame_hop", "frame_phase", "frame_stride"]
    for name, want in (("WnStackDesc", names), ("WnDecoderDesc", dnames)):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1), flags=re.S)
        got = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.strip().split(",")]
        assert got == want, name
    assert _lib.WnStackDesc().bias_interp == 0 and _lib.WnDecoderDesc().frame_interp == 0
    assert "bias_interp" in hdr and "frame_interp" in hdr and "ANCHORED" in hdr
