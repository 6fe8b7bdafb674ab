"""Scoring without a GPU: the new WnExec flag, the host helpers of wavenet_amd/scoring.py, the evaluate command's parser."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gpu_util import CFG1
from wavenet_amd import Params, _lib, scoring
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import evaluate
from wavenet_amd.train_audio.train import input_width_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_defines_the_row_flag_and_the_binding_mirrors_it():
    text = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    m = re.search(r"^#define\s+WN_EXEC_HEAD_ROW_NLL\s+(\d+)u\b", text, re.M)
    assert m and int(m.group(1)) == 32
    assert _lib.WN_EXEC_HEAD_ROW_NLL == 32
    others = (_lib.WN_EXEC_FORCE_GENERIC, _lib.WN_EXEC_NO_FWD_GROUPS, _lib.WN_EXEC_NO_PIPELINED_GEMM,
              _lib.WN_EXEC_NO_MULTI_LAYER_BWD, _lib.WN_DECODER_ONE_WORKGROUP)
    assert all(_lib.WN_EXEC_HEAD_ROW_NLL & f == 0 for f in others)
    assert _lib.default_exec_flags() & _lib.WN_EXEC_HEAD_ROW_NLL == 0        # a per-call bit, never a model default


@pytest.mark.parametrize("chunk,batch", [(5, 3), (64, 2)])
def test_plan_chunks_covers_every_sample_exactly_once_and_in_order(chunk, batch):
    for n in (1, 2, chunk - 1, chunk, chunk + 1, 3 * chunk * batch + 7):
        plan = scoring.plan_chunks(n, chunk, batch)
        pos = 0
        for launch in plan:
            assert 1 <= len(launch) <= batch
            assert len({w for _, w in launch}) == 1                         # one width per launch: the rows of a batch
            for start, width in launch:
                assert start == pos and 1 <= width <= chunk
                pos += width
        assert pos == n, (n, plan)
        # full launches first, at most one smaller batch of full pieces, at most one ragged piece
        assert len(plan) == n // (chunk * batch) + (1 if (n // chunk) % batch else 0) + (1 if n % chunk else 0)
    assert scoring.plan_chunks(0, chunk, batch) == []
    with pytest.raises(ValueError):
        scoring.plan_chunks(4, 0, 1)
    with pytest.raises(ValueError):
        scoring.plan_chunks(4, 1, 0)


def test_context_width_is_the_training_input_width_for_filter_width_two():
    for p in (Params(), Params(CFG1)):
        assert scoring.context_width(p) == input_width_of(p)
    assert scoring.context_width(Params()) == 1024
    assert scoring.context_width(Params(CFG1)) == 17
    wide = Params(dict(causal_conv_filter_width=3, causal_conv_channels=[8, 8], residual_conv_filter_width=3,
                       residual_conv_channels=[8, 8], residual_num_blocks=2))
    assert scoring.context_width(wide) == 1 + 2 * 2 + 2 * (2 * 1 + 2 * 3)   # sum of (fw - 1) * dilation, dilations 1 and 3
    assert scoring.silence_token(256) == 127 and scoring.silence_token(64) == 32


def test_summarize_on_a_hand_made_array():
    got = scoring.summarize(np.array([0.5, 1.5, 2.0, 0.0], dtype=np.float32))
    assert got == {"samples": 4, "nats_per_sample": 1.0, "bits_per_sample": 1.0 / math.log(2.0)}
    # summed in float64: in float32, 1e8 + 1 is 1e8 and the sum would be 0
    assert scoring.summarize(np.array([1e8, 1.0, -1e8], dtype=np.float32))["nats_per_sample"] == 1.0 / 3.0
    assert scoring.summarize(np.zeros((0,), np.float32)) == {"samples": 0, "nats_per_sample": 0.0, "bits_per_sample": 0.0}


def test_the_evaluate_parser_has_its_own_defaults_and_leaves_the_shared_one_alone():
    a = evaluate.build_parser().parse_args([])
    assert vars(a) == dict(gpu_device=0, wav_dir="wav", model_dir="model", chunk_width=16384, batch_size=8, json=None)
    b = evaluate.build_parser().parse_args(["-g", "1", "-w", "held", "-m", "m2", "--chunk-width", "100", "--batch-size", "3",
                                            "--json", "out.json"])
    assert vars(b) == dict(gpu_device=1, wav_dir="held", model_dir="m2", chunk_width=100, batch_size=3, json="out.json")
    shared = vars(cli_args.parse([]))
    assert "chunk_width" not in shared and "json" not in shared and shared["batch_size"] == 16


def test_the_row_form_names_its_null_pointer_without_a_gpu():
    lib = _lib.lib()
    one = (C.c_float * 4)()
    p = C.cast(one, C.c_void_p)
    for flags, word in ((_lib.WN_EXEC_HEAD_ROW_NLL, b"row_nll"), (0, b"dlogits")):
        ex = _lib.WnExec()
        ex.precision, ex.flags = _lib.GEMM_PRECISIONS.index("fp16x2"), flags
        rc = lib.wn_head_xent(p, p, None, p, p, None, 4, 32, 256, _lib.WN_ACT_RELU, 0, C.byref(ex), None)
        msg = lib.wn_last_error()
        assert rc == _lib.WN_EARG and msg.startswith(b"wn_head_xent: " + word) and msg.endswith(b"is NULL"), (flags, msg)
