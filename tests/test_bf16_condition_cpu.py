"""Conditioning on bf16 storage, the parts that need no GPU: ``WaveNet.set_storage``, the constructor's refusals, the header's
``WN16_BWD_ROW_GRADS``, the unchanged ABI, the ``--storage`` flags, ``TrainStepGraph._hyper`` and the conditioned rounding
oracle (tests/bf16_cond_ref.py) against ``oracle.bf16_ref`` and against an autograd restatement of itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bf16_cond_ref as QC
from oracle import bf16_ref as Q
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, WaveNet, _lib
from wavenet_amd.graph import TrainStepGraph
from wavenet_amd.train_audio import args as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 3, residual_num_blocks=2,
             softmax_conv_channels=[256, 256])


def test_set_storage_checks_its_argument_and_marks_the_images_stale():
    net = WaveNet(Params(R.make_params(**SMALL)), seed=0, condition_classes=3, condition_channels=4)
    assert net.storage == "fp32"
    net._w16_stale = False
    net.set_storage("bf16")
    assert net.storage == "bf16" and net._w16_stale
    net._w16_stale = False
    net.set_storage("fp32")
    assert net.storage == "fp32" and net._w16_stale
    with pytest.raises(Exception, match="storage must be 'fp32' or 'bf16'"):
        net.set_storage("fp16")
    assert net.storage == "fp32"


@pytest.mark.parametrize("cls", [WaveNet, FasterWaveNet])
def test_the_constructor_still_refuses_and_names_set_storage(cls):
    p = Params(R.make_params(**SMALL))
    with pytest.raises(Exception, match="global conditioning is not available with storage='bf16'") as e:
        cls(p, seed=0, storage="bf16", condition_classes=3, condition_channels=4)
    assert "set_storage" in str(e.value)
    with pytest.raises(Exception, match="local conditioning is not available with storage='bf16'") as e:
        cls(p, seed=0, storage="bf16", local_channels=4, local_hop=16)
    assert "set_storage" in str(e.value)


def test_header_defines_the_row_gradient_bit_and_the_abi_is_what_it_was():
    h = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.search(r"^#define WN16_BWD_ROW_GRADS 1u", h, re.M)
    assert "pass 0" not in h[h.index("size_t wn16_stack_bwd_workspace_bytes"):h.index("int wn16_pack_pointwise")]
    assert _lib.WN16_BWD_ROW_GRADS == 1
    assert re.search(r"^#define WN_ABI_VERSION 5\b", h, re.M) and _lib.ABI_VERSION == 5
    assert len(set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", h))) == 69         # the declared entry points
    assert C.sizeof(_lib.WnStackDesc) == 120


def test_storage_flags_parse():
    ns = A.build_parser().parse_args(["--storage", "bf16"], namespace=A.Args())
    assert ns.storage == "bf16"
    assert A.build_parser().parse_args([], namespace=A.Args()).storage == "fp32"
    with pytest.raises(SystemExit):
        A.parse(["--storage", "fp8"])


def test_the_graphs_by_value_settings_hold_the_storage():
    net = WaveNet(Params(R.make_params(**SMALL)), seed=0)
    g = TrainStepGraph.__new__(TrainStepGraph)
    g.net = net
    a = g._hyper()
    net.set_storage("bf16")
    b = g._hyper()
    assert a != b and "fp32" in a and "bf16" in b


TINY = dict(quantization_steps=32, causal_conv_channels=[16], residual_conv_channels=[16] * 3, residual_num_blocks=2,
            softmax_conv_channels=[24, 32])


def _tiny():
    p = R.make_params(**TINY)
    w = R.init_weights(p, 3)
    w["softmax_0/b"] = (np.random.RandomState(2).standard_normal(32) * 0.3).astype(np.float32)
    rs = np.random.RandomState(4)
    iw = R.input_width(p)
    idx = rs.randint(0, 32, (2, iw + 21)).astype(np.int32)
    tgt = rs.randint(0, 32, (2, 21)).astype(np.int32)
    offsets = [(32 * l, 32 * l + 16) for l in range(6)]
    return p, w, idx, tgt, offsets, rs


def _dense(shape, kw, T):
    """a block of frames holds the rows the call reads (the middle entry of ``shape`` is a placeholder)"""
    if len(shape) == 2:
        return shape
    from wavenet_amd.wavenet import frames_needed
    worst = kw["hop"] - 1 if np.ndim(kw["phase"]) else kw["phase"]
    return (shape[0], frames_needed(T, kw["hop"], worst, "linear" if kw["interp"] else "repeat"), shape[2])


@pytest.mark.parametrize("shape,kw", [((2, 192), {}), ((2, 9, 192), dict(hop=5, phase=[0, 4], interp=1)),
                                      ((2, 2, 192), dict(hop=48, phase=47, interp=0))])
def test_rows_of_zeros_are_the_unconditioned_oracle_exactly(shape, kw):
    p, w, idx, tgt, offsets, _ = _tiny()
    shape = _dense(shape, kw, idx.shape[1])
    keep0, keep1 = {}, {}
    l0, lg0, g0 = Q.train_step(p, w, idx, tgt, keep=keep0)
    l1, lg1, g1, db = QC.train_step(p, w, idx, tgt, rows=dict(block=np.zeros(shape, np.float32), offsets=offsets, **kw), keep=keep1)
    assert l0 == l1 and np.array_equal(lg0, lg1)
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for a, b in zip(keep0["dadg"], keep1["dadg"]):
        assert np.array_equal(a, b)
    assert db.shape == shape
    lnone = QC.train_step(p, w, idx, tgt)
    assert lnone[0] == l0 and lnone[3] is None
    lay = list(Q._layers(p))
    x = keep0["x0"]
    z0, o0 = Q.layer_fwd(x, w[lay[1][0] + "wf/W"], w[lay[1][0] + "wg/W"], w[lay[1][0] + "projection_block/W"], 2, 1)
    z1, o1 = QC.layer_fwd(x, w[lay[1][0] + "wf/W"], w[lay[1][0] + "wg/W"], w[lay[1][0] + "projection_block/W"], 2, 1,
                          np.zeros(x.shape), np.zeros(x.shape))
    assert np.array_equal(z0, z1) and np.array_equal(o0, o1)


@pytest.mark.parametrize("shape,kw", [((2, 192), {}), ((2, 9, 192), dict(hop=5, phase=[0, 4], interp=0)),
                                      ((2, 9, 192), dict(hop=5, phase=[3, 1], interp=1)), ((2, 3, 192), dict(hop=16, phase=15, interp=1))])
def test_hand_written_backward_with_rows_agrees_with_autograd(shape, kw):
    """the bar of tests/test_oracle.py for the unconditioned pair: loss 1e-6, logits 1e-5, every gradient 3e-3 in the 2-norm"""
    p, w, idx, tgt, offsets, rs = _tiny()
    shape = _dense(shape, kw, idx.shape[1])
    rows = dict(block=(rs.standard_normal(shape) * 0.5).astype(np.float32), offsets=offsets, **kw)
    l1, lg1, g1, d1 = QC.train_step(p, w, idx, tgt, rows=rows)
    l2, lg2, g2, d2 = QC.train_step_autograd(p, w, idx, tgt, rows=rows)
    l0 = Q.train_step(p, w, idx, tgt)[0]
    assert abs(l1 - l2) < 1e-6 and abs(l1 - l0) > 1e-4          # ... and the rows matter
    np.testing.assert_allclose(lg1, lg2, atol=1e-5)
    g1, g2 = dict(g1, block=d1), dict(g2, block=d2)
    for k in g1:
        n = np.linalg.norm(g2[k]) + 1e-12
        assert np.linalg.norm(g1[k] - g2[k]) <= 3e-3 * n, (k, np.linalg.norm(g1[k] - g2[k]) / n)
    assert np.linalg.norm(d1) > 0


def test_row_values_follow_the_three_operation_lerp():
    blk = np.random.RandomState(1).standard_normal((2, 5, 8)).astype(np.float32)
    rows = dict(block=blk, hop=3, phase=[0, 2], interp=1)
    y = QC.row_values(rows, 2, 9)
    for b, ph in enumerate([0, 2]):
        for t in range(9):
            pp = t + ph
            a = np.float32(pp % 3) / np.float32(3)
            r0, r1 = blk[b, pp // 3], blk[b, pp // 3 + 1]
            want = (r0 + np.float32(a) * (r1 - r0).astype(np.float32)).astype(np.float32)
            assert np.array_equal(y[b, t], want)
    same = QC.row_values(dict(block=np.repeat(blk[:, :1], 5, axis=1), hop=3, phase=1, interp=1), 2, 9)
    assert np.array_equal(same, np.broadcast_to(blk[:, :1], (2, 9, 8)))
