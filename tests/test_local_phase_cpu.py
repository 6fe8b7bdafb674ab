"""A feature phase per clip without a GPU: header against binding, the library's refusals (which answer before any device
work), ``local_phase=`` sequences on the model's face, the trainer's ``--local-crop sample`` draw and the flag itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import local_cond_ref as LR
from oracle import wavenet_ref as R
from wavenet_amd import Params, WaveNet, _lib
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio.train import _Crops
from wavenet_amd.wavenet import LocalPhases, frames_needed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header and binding ----------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_and_the_table_sits_in_front_of_the_local_group():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.findall(r"^#define\s+WN_ABI_VERSION\s+(\d+)", hdr, flags=re.M) == ["5"]
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))) == 69
    assert len(re.findall(r"^#define\s+WN_EXEC_\w+\s+\d+u", hdr, flags=re.M)) == 6
    assert [f[0] for f in _lib.WnExec._fields_] == ["precision", "flags", "ws", "ws_bytes", "fwd_t1_min_blocks", "reserved", "plan"]
    names = [f[0] for f in _lib.WnStackDesc._fields_]
    assert names[-5:] == ["bias_phase_tab", "bias_interp", "bias_hop", "bias_phase", "bias_frame_stride"]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct WnStackDesc \{(.*?)\} WnStackDesc;", hdr, re.S).group(1), flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    got = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for d in decls for part in d.split(",")]
    assert got == names
    tab = [d for d in decls if "bias_phase_tab" in d]
    assert len(tab) == 1 and re.sub(r"\s+", " ", tab[0]) == "const int* bias_phase_tab"
    assert dict(_lib.WnStackDesc._fields_)["bias_phase_tab"] is ctypes.c_void_p
    assert ctypes.sizeof(_lib.WnStackDesc) == 16 + 10 * 8 + 8 + 16           # 4 ints, 2 + 8 pointers, the table, 4 ints
    d = _lib.WnStackDesc()
    assert d.bias_phase_tab is None and d.bias_phase == 0                    # NULL by default
    assert "bias_phase_tab" in hdr and "FENCE" in hdr


# ---- the library's refusals ------------------------------------------------------------------------------------------------
L = 2
_W = (ctypes.c_void_p * L)(0x1000, 0x2000)                # never dereferenced: every call below is refused first
_CD, _DIL = (ctypes.c_int * L)(32, 32), (ctypes.c_int * L)(1, 2)
_P = 0x3000
PER_CLIP = _lib.WN_EXEC_BIAS_PER_CLIP


def _call(which, tab, hop, phase, stride, flags, reserved, T=64, interp=0):
    lib = _lib.lib()
    d = _lib.WnStackDesc(n_layers=L, Cr=32, Cs=256, fw=2, cd=_CD, dilation=_DIL, Wf=_W, Wg=_W, Wp=_W, Ws=_W, bf=_W, bg=_W,
                         bias_phase_tab=tab, bias_interp=interp, bias_hop=hop, bias_phase=phase, bias_frame_stride=stride)
    ex = _lib.WnExec(precision=0, flags=flags, reserved=reserved)
    if which == "fwd":
        rc = lib.wn_stack_fwd(ctypes.byref(d), _P, _P + 64, _P, None, None, None, 1, T, 0, 0, 0, ctypes.byref(ex), None)
    else:
        rc = lib.wn_stack_bwd(ctypes.byref(d), _P, _P, _P, _P, _P, _P, None, None, _W, _W, _W, _W, _W, None, None, None, _P,
                              1 << 40, 1, T, 0, 0, ctypes.byref(ex), None)
    return rc, lib.wn_last_error()


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_the_table_is_refused_without_a_gpu_wherever_it_cannot_be_meant(which):
    """Every refusal answers WN_EARG with the field's name before any device work, forward and backward, on a machine without
    a device.  T = 64 at hop 12: the worst phase, 11, spans ceil(75 / 12) = 7 frames, 8 rows in linear mode; a scalar phase 0
    spans 6, which is why `reserved` = 6 frames is enough without a table and one short with one."""
    TAB = 0x4000
    for args_, word in (((TAB, 0, 0, 64, PER_CLIP, 640), b"bias_phase_tab without frames"),
                        ((TAB, 12, 0, 64, 0, 640), b"bias_phase_tab without WN_EXEC_BIAS_PER_CLIP"),
                        ((TAB, 0, 0, 64, 0, 640), b"bias_phase_tab without WN_EXEC_BIAS_PER_CLIP"),
                        ((TAB, 12, 3, 64, PER_CLIP, 640), b"bias_phase_tab together with bias_phase = 3"),
                        ((TAB + 2, 12, 0, 64, PER_CLIP, 640), b"bias_phase_tab is not 4-byte aligned"),
                        ((TAB, 12, 0, 64, PER_CLIP, 7 * 64 - 1), b"bias_phase_tab")):
        rc, msg = _call(which, *args_)
        assert rc == _lib.WN_EARG and word in msg, (args_, msg)
    # reserved one float below n_max * stride, in both modes; exactly n_max * stride passes this check (and the call is then
    # refused further on or not at all -- never for the geometry)
    for interp, n_max in ((0, 7), (1, 8)):
        rc, msg = _call(which, TAB, 12, 0, 64, PER_CLIP, n_max * 64 - 1, interp=interp)
        assert rc == _lib.WN_EARG and b"reserved" in msg and b"bias_phase_tab" in msg and (b"%d " % n_max) in msg, msg
        rc, msg = _call(which, None, 12, 0, 64, PER_CLIP, (n_max - 1) * 64 - 1, interp=interp)
        assert rc == _lib.WN_EARG and b"reserved" in msg and b"bias_phase_tab" not in msg, msg     # the scalar call is what it was
    # the kernels form t + phase in 32 bits, and a table may hold hop - 1
    rc, msg = _call(which, TAB, 1000, 0, 64, PER_CLIP, 2 ** 31 - 1, T=2 ** 31 - 500)
    assert rc == _lib.WN_EARG and b"bias_hop - 1" in msg and b"does not fit 32 bits" in msg and b"bias_phase_tab" in msg, msg


# ---- the model's face ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ["repeat", "linear"])
def test_local_features_takes_a_phase_per_clip_and_names_the_offending_clip(interp):
    p = Params(R.make_params(**LR.TINY))
    net = WaveNet(p, seed=5, local_channels=5, local_hop=12, local_interp=interp)
    need = frames_needed(70, 12, 11, interp)
    assert need == (7 if interp == "repeat" else 8)
    h = np.zeros((3, 5, need), np.float32)
    for seq in ([0, 5, 11], (0, 5, 11), np.array([0, 5, 11]), np.array([0, 5, 11], np.uint8), torch.tensor([0, 5, 11]),
                torch.tensor([0, 5, 11], dtype=torch.int32)):
        f, ph = net._local_features(h, 3, 70, seq)
        assert isinstance(ph, LocalPhases) and ph.hop == 12 and ph.tab.dtype == torch.int32 and ph.tab.tolist() == [0, 5, 11]
        assert tuple(f.shape) == (3, 5, need)
    again = net._local_features(h, 3, 70, ph)[1]
    assert again is ph                                                   # a checked table is handed through as it stands
    # the columns of the worst phase, whatever the phases are: a table of zeros still needs them; surplus ones are ignored
    with pytest.raises(Exception, match=r"holds %d feature columns, but 70 positions at hop 12 and phase 11 read %d" % (need - 1, need)):
        net._local_features(h[:, :, :need - 1], 3, 70, [0, 0, 0])
    net._local_features(np.zeros((3, 5, need + 2), np.float32), 3, 70, [0, 0, 0])
    assert net._local_features(h[:, :, :need - 1], 3, 70, 0)[1] == 0     # ... while the int form asks for its own phase's
    with pytest.raises(Exception, match="holds 2 phases for 3 clips"):
        net._local_features(h, 3, 70, [0, 5])
    with pytest.raises(Exception, match="holds 4 phases for 3 clips"):
        net._local_features(h, 3, 70, np.zeros(4, np.int64))
    with pytest.raises(Exception, match=r"integer phases, got float64 \(clip 0\)"):
        net._local_features(h, 3, 70, [0.0, 5.0, 11.0])
    with pytest.raises(Exception, match="integer phases, got float32"):
        net._local_features(h, 3, 70, torch.tensor([0.0, 5.0, 11.0]))
    with pytest.raises(Exception, match=r"must lie in \[0, local_hop = 12\), got -1 for clip 1"):
        net._local_features(h, 3, 70, [0, -1, 12])
    with pytest.raises(Exception, match=r"must lie in \[0, local_hop = 12\), got 12 for clip 2"):
        net._local_features(h, 3, 70, [0, 5, 12])
    with pytest.raises(Exception, match="1-D sequence"):
        net._local_features(h, 3, 70, [[0, 5, 11]])
    with pytest.raises(Exception, match="checked against hop 7"):
        net._local_features(h, 3, 70, LocalPhases(torch.zeros(3, dtype=torch.int32), 7))
    # an int works as it did, message for message
    with pytest.raises(Exception, match=r"local_phase= must lie in \[0, local_hop = 12\), got 12$"):
        net._local_features(h, 3, 70, 12)
    plain = WaveNet(p, seed=5)
    with pytest.raises(Exception, match="no local conditioning"):
        plain._local_features(None, 3, 70, [0, 0, 0])


# ---- the trainer's crops ---------------------------------------------------------------------------------------------------
IW, TW, HOP = 16, 24, 12


def _crops(crop=None, extra=False, n=400, shift=8, cols=None, features=True):
    sig = np.random.RandomState(3).randint(0, 256, n).astype(np.int32)
    cols = (n + shift + HOP - 1) // HOP + int(extra) if cols is None else cols
    feats = np.arange(5 * cols, dtype=np.float32).reshape(5, cols)
    kw = dict(features=feats, hop=HOP, shift=shift, extra_column=extra) if features else {}
    if crop is not None:
        kw["crop"] = crop
    return _Crops(sig, IW, TW, "cpu", **kw), sig, feats


@pytest.mark.parametrize("extra", [False, True])
def test_sample_crops_are_the_feature_less_draw_with_a_phase_and_columns_per_crop(extra):
    """One seed: the starts of ``crop="sample"`` are those of a _Crops without features (the same tokens), the phases and
    first columns follow the alignment rule -- index + shift = position, position // hop = column, position % hop = phase --
    and every crop carries the columns of the worst phase."""
    plain, sig, _ = _crops(features=False)
    samp, _, feats = _crops("sample", extra)
    np.random.seed(11)
    x0, t0 = plain.draw(6)
    state = np.random.get_state()[1].copy()
    np.random.seed(11)
    x1, t1, f1, ph = samp.draw(6)
    assert np.array_equal(np.random.get_state()[1], state)                  # the very same draw: the stream stands where it stood
    assert torch.equal(x0, x1) and torch.equal(t0, t1)
    np.random.seed(11)
    starts = np.random.randint(0, 400 - TW - IW - 1, size=6)
    assert np.array_equal(x1.numpy(), np.stack([sig[s:s + IW + TW] for s in starts]))
    assert ph.dtype.kind == "i" and np.array_equal(ph, (starts + 8) % HOP) and len(set(ph.tolist())) > 2
    n = frames_needed(IW + TW, HOP, HOP - 1, "linear" if extra else "repeat")
    assert tuple(f1.shape) == (6, 5, n) and n == (6 if extra else 5)      # ceil((40 + 11) / 12) = 5
    first = (starts + 8) // HOP
    assert np.array_equal(f1.numpy(), np.stack([feats[:, c:c + n] for c in first]))
    # position t of crop b reads column (start + shift + t) // hop of the file: column (t + phase) // hop of what it was handed
    for b in range(6):
        for t in (0, IW + TW - 1):
            assert f1[b, 0, (t + ph[b]) // HOP] == feats[0, (starts[b] + 8 + t) // HOP]


def test_a_sample_crop_at_the_end_of_the_file_repeats_the_last_column():
    """The worst-case column count runs past the file's columns for a crop near the end whose own phase needs fewer: the
    last column is repeated, nothing is indexed beyond the array."""
    n, shift = 400, 8
    cols = (n + shift + HOP - 1) // HOP                                     # 34: exactly what the tokens span
    samp, sig, feats = _crops("sample", n=n, shift=shift, cols=cols)
    last = n - TW - IW - 2                                                  # the largest start randint can return
    real = np.random.randint
    try:
        np.random.randint = lambda lo, hi, size: np.full(size, hi - 1)
        x, tg, f, ph = samp.draw(2)
    finally:
        np.random.randint = real
    assert int(x[0, 0]) == sig[last] and ph[0] == (last + shift) % HOP
    first = (last + shift) // HOP
    assert first + f.shape[2] > cols                                        # the count does run past the file
    want = feats[:, np.minimum(first + np.arange(f.shape[2]), cols - 1)]
    assert np.array_equal(f[0].numpy(), want) and np.array_equal(f[0, :, -1].numpy(), feats[:, -1])


@pytest.mark.parametrize("extra", [False, True])
def test_frame_crops_are_what_they_were(extra):
    """``crop="frame"`` and no argument at all: the same starts, columns, phases (none) and generator state afterwards."""
    old, _, _ = _crops(None, extra)
    new, _, _ = _crops("frame", extra)
    np.random.seed(5)
    a = old.draw(7)
    sa = np.random.get_state()[1].copy()
    np.random.seed(5)
    b = new.draw(7)
    assert len(a) == len(b) == 3 and all(torch.equal(u, v) for u, v in zip(a, b))
    assert np.array_equal(np.random.get_state()[1], sa)
    assert tuple(a[2].shape) == (7, 5, (IW + TW + HOP - 1) // HOP + int(extra))
    with pytest.raises(Exception, match="crop must be"):
        _crops("window")


def test_local_crop_parses_and_goes_with_local_dir(capsys):
    a = cli_args.parse([])
    assert a.local_crop is None and "local_crop" not in vars(a)
    a = cli_args.parse(["--local-dir", "feat", "--local-crop", "sample"])
    assert a.local_crop == "sample"
    assert cli_args.parse(["--local-dir", "feat", "--local-crop", "frame"]).local_crop == "frame"
    assert cli_args.parse(["--local-dir", "feat"]).local_crop is None
    for argv in (["--local-crop", "sample"], ["--local-dir", "feat", "--local-crop", "window"]):
        with pytest.raises(SystemExit):
            cli_args.parse(argv)
        assert "--local-crop {frame,sample} goes with --local-dir" in capsys.readouterr().err
