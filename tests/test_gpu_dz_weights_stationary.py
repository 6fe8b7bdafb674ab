"""dz of the skip path with the weights held in registers (k_dz_ws) against the kernel it replaces.

Every case calls wn_skip_sum_bwd_dz twice on the same inputs -- default flags (k_dz_ws) and WN_EXEC_NO_PIPELINED_GEMM
(k_colgemm_b3<2, 0, 3, 8>) -- and asks for IDENTICAL results, bit for bit (same products in the same order), and for every
layer's dz within 1e-4 of its largest entry of Ws^T dskip formed in float64 (the gradient bar of test_gpu_parity.py;
chainer's Convolution2D backward for the 1x1 skip projection, wavenet.py:363-364).
"""
import os

import numpy as np
import pytest
import torch

from wavenet_amd import _lib

from gpu_util import EX, to_np

pytestmark = pytest.mark.gpu

CS, CD = 256, 32

# L, B, T, t_off: the smallest shapes at which each path of the kernel can still go wrong
CASES = {
    # five full layer groups; 513 columns per clip (16 tiles + 1 column): a ragged last tile, a clip boundary inside a range
    "five_groups_ragged": (40, 2, 700, 187),
    # a second group with one live wave and seven idle ones
    "one_live_wave": (9, 1, 300, 100),
    # a group with idle waves and a window of 31 columns: less than one tile
    "partial_tile": (3, 1, 131, 100),
    # more workgroups than column tiles per range; the XCD mapping with B a multiple of 8
    "many_ranges": (8, 8, 4096 + 96, 4094),
}

_cache = {}


def _inputs(name):
    """(Ws on the device, dskip on the device, the float64 reference per layer) of a case: made once, left unchanged."""
    if name not in _cache:
        L, B, T, t_off = CASES[name]
        tw = T - t_off
        rs = np.random.RandomState(20260 + L * 1000 + tw)
        Ws = (rs.randn(L, CS, CD) * 0.05).astype(np.float32)                       # weights ~ N(0, 0.05)
        row_scale = 10.0 ** (-6.0 * rs.rand(B, tw, 1))                              # per-row magnitudes over 1e-6 .. 1
        dskip = (rs.randn(B, tw, CS) * row_scale).astype(np.float32)
        ref = np.einsum("btc,lcd->lbtd", dskip.astype(np.float64), Ws.astype(np.float64))
        _cache[name] = ([torch.from_numpy(Ws[l]).cuda() for l in range(L)], torch.from_numpy(dskip).cuda(), ref)
    return _cache[name]


def _run(name, flags):
    from wavenet_amd._lib import ptr, ptr_array, int_array, stream_ptr
    L, B, T, t_off = CASES[name]
    Ws, dskip, _ = _inputs(name)
    dz = [torch.full((B, T, CD), float("nan"), device="cuda") for _ in range(L)]
    rc = _lib.lib().wn_skip_sum_bwd_dz(L, ptr_array(Ws), int_array([CD] * L), ptr(dskip), ptr_array(dz), B, T, t_off, T - t_off, CS,
                                       EX("fp16x2", flags=flags), stream_ptr())
    _lib.check(rc, "wn_skip_sum_bwd_dz")
    torch.cuda.synchronize()
    return dz


def _skip_generic():
    if os.environ.get("WAVENET_HIP_FORCE_GENERIC") == "1":
        pytest.skip("generic kernels only")


@pytest.mark.parametrize("name", list(CASES))
def test_weights_stationary_dz_is_the_older_kernel_bit_for_bit(name):
    _skip_generic()
    L, B, T, t_off = CASES[name]
    new = _run(name, None)
    old = _run(name, _lib.WN_EXEC_NO_PIPELINED_GEMM)
    ref = _inputs(name)[2]
    for l in range(L):
        assert torch.equal(new[l], old[l]), (name, l)
        got = to_np(new[l])
        assert not got[:, :t_off].any(), (name, l)                                 # below the loss window: zeros
        err, scale = np.abs(got[:, t_off:] - ref[l]).max(), np.abs(ref[l]).max()
        assert err <= 1e-4 * scale, (name, l, err, scale)


def test_weights_stationary_dz_is_the_same_from_run_to_run():
    """No dependence on which workgroup is resident when: the first shape twice, identical."""
    _skip_generic()
    a = _run("five_groups_ragged", None)
    b = _run("five_groups_ragged", None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
