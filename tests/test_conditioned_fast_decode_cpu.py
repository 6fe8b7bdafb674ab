"""CPU: conditioned decoding on the specialised 32/256-channel decoder -- the flag, the host's forecast of the decoder form and
the descriptor a conditioned model builds.  No device: descriptors are built from models that were never moved to one."""
import os
import re

import pytest

from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# config 4's shape at 2 x 5 layers (tests/test_gpu_ragged_generation.py's NINE)
NINE = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 5, residual_num_blocks=2,
            softmax_conv_channels=[256, 256])
KINDS = {"plain": {}, "local": dict(local_channels=5, local_hop=5), "global": dict(condition_classes=3, condition_channels=8),
         "local+global": dict(local_channels=5, local_hop=5, condition_classes=3, condition_channels=8)}


def _net(kind, over=NINE):
    return FasterWaveNet(Params(R.make_params(**over)), seed=0, **KINDS[kind])


def test_the_header_defines_the_flag_and_the_binding_mirrors_it():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.search(r"^#define WN_DECODER_GATE_ROWS 128u\s*$", hdr, re.M)
    assert _lib.WN_DECODER_GATE_ROWS == 128
    # the bit is free: no other WnExec / WnDecoderDesc flag uses it
    others = {k: int(v) for k, v in re.findall(r"^#define (WN_(?:EXEC|DECODER)_[A-Z_]+) (\d+)u\b", hdr, re.M) if k != "WN_DECODER_GATE_ROWS"}
    assert "WN_DECODER_ONE_WORKGROUP" in others and "WN_EXEC_FORCE_GENERIC" in others
    assert all(v & 128 == 0 for v in others.values()), others


def test_no_new_export_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 69 and declared == set(_lib.EXPORTS)
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.ABI_VERSION


@pytest.mark.parametrize("kind", ["local", "global", "local+global"])
def test_a_conditioned_model_of_config_4s_shape_is_forecast_on_the_specialised_decoder(kind):
    net = _net(kind)
    assert net._nine_workgroup_shape(0) is True
    assert net._nine_workgroup_shape(_lib.WN_DECODER_ONE_WORKGROUP) is True        # (that flag picks the kernel, not the form)
    assert net._nine_workgroup_shape(_lib.WN_EXEC_FORCE_GENERIC) is False


def test_the_forecast_of_other_models_is_what_it_was():
    assert _net("plain")._nine_workgroup_shape(0) is True
    assert _net("plain")._nine_workgroup_shape(_lib.WN_EXEC_FORCE_GENERIC) is False
    with_bias = dict(NINE, residual_conv_dilation_no_bias=False)               # tests/test_gpu_batched_generation.py's biased model
    assert _net("plain", with_bias)._nine_workgroup_shape(0) is False
    other = dict(NINE, residual_conv_channels=[16] * 5)                          # a conditioned model of another shape
    assert _net("local+global", other)._nine_workgroup_shape(0) is False


@pytest.mark.parametrize("kind,want", [("plain", False), ("local", True), ("global", True), ("local+global", True)])
def test_desc_sets_the_flag_for_conditioned_models_only(kind, want):
    net = _net(kind)
    d, keep = net._desc()
    assert bool(d.flags & _lib.WN_DECODER_GATE_ROWS) == want
    net.exec_flags = _lib.WN_DECODER_ONE_WORKGROUP                               # the model's own flags travel with it
    d, keep = net._desc(step_limit=3)
    assert bool(d.flags & _lib.WN_DECODER_GATE_ROWS) == want and d.flags & _lib.WN_DECODER_ONE_WORKGROUP and d.step_limit == 3
    net.exec_flags = _lib.WN_EXEC_FORCE_GENERIC                                  # ... the library ignores the flag on that form
    d, keep = net._desc()
    assert d.flags & _lib.WN_EXEC_FORCE_GENERIC and bool(d.flags & _lib.WN_DECODER_GATE_ROWS) == want
    biased = _net("plain", dict(NINE, residual_conv_dilation_no_bias=False))     # bias tensors alone are no conditioning
    assert not biased._desc()[0].flags & _lib.WN_DECODER_GATE_ROWS
