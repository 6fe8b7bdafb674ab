"""Global conditioning without a GPU: the CPU reference checks itself, the model's new links leave the old layout alone, the
header carries the new flag, and the speaker labels of the command line."""
import json
import os
import re

import numpy as np
import pytest
import torch

import cond_ref
from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, WaveNet, _lib
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import model as cli_model
from wavenet_amd.train_audio import speakers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(seed=3, tw=40):
    p = R.make_params(**cond_ref.TINY)
    w = R.init_weights(p, 1234)
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, 256, (cond_ref.B, cond_ref.T)).astype(np.int32)
    tgt = rs.randint(0, 256, (cond_ref.B, tw)).astype(np.int32)
    return p, w, idx, tgt


# ---- the reference checks itself -------------------------------------------------------------------------------------------
def test_reference_with_a_zero_projection_is_the_unconditioned_oracle():
    """V = 0 makes every conditioning bias 0, and the reference must then BE the oracle's ``train_step_grads``.

    Exactly, where the oracle is exact with itself: the reference runs one clip at a time, and its logits are bit for bit
    those of ``train_step_grads`` on that clip (adding a zero bias changes no bit).  The oracle on the whole batch is NOT
    bit-identical to the oracle clip by clip -- torch's CPU convolution picks its blocking by batch size; the float32 logits
    of this very case differ by 1.3e-7 between B = 3 and three B = 1 calls -- so against the whole-batch call the float32
    comparison is held to float32 rounding (2e-6 of each tensor's largest entry), and the same comparison in float64, where
    that rounding is 1e-16, to 1e-12: any term missing or counted twice is orders of magnitude above either."""
    p, w, idx, tgt = _case()
    E, V = cond_ref.init_condition(p)
    loss, logits, g = cond_ref.train_step_grads(p, w, E, np.zeros_like(V), cond_ref.IDS, idx, tgt)
    for b in range(cond_ref.B):
        _, lg_b, _ = R.train_step_grads(p, w, idx[b:b + 1], tgt[b:b + 1])
        assert np.array_equal(logits[b:b + 1], lg_b), b
    for dtype, tol in ((torch.float32, 2e-6), (torch.float64, 1e-12)):
        loss, logits, g = cond_ref.train_step_grads(p, w, E, np.zeros_like(V), cond_ref.IDS, idx, tgt, dtype=dtype)
        loss0, logits0, g0 = R.train_step_grads(p, w, idx, tgt, dtype=dtype)
        assert abs(loss - loss0) <= tol * abs(loss0)
        assert np.abs(logits - logits0).max() <= tol * np.abs(logits0).max()
        for k in g0:
            assert np.abs(g[k] - g0[k]).max() <= tol * max(np.abs(g0[k]).max(), 1e-30), (k, dtype)
        assert not g["E"].any()                            # no path from E to the loss through a zero projection
        assert g["V"].any()


def test_reference_gradients_of_the_conditioning_tensors_agree_with_central_differences():
    """float64, a few entries of E and V (a used class, the repeated class, the unused class: exactly 0)."""
    p, w, idx, tgt = _case(tw=12)
    E, V = cond_ref.init_condition(p)
    E, V = E.astype(np.float64), V.astype(np.float64)
    ids = cond_ref.IDS
    _, _, g = cond_ref.train_step_grads(p, w, E, V, ids, idx, tgt, dtype=torch.float64)
    assert not g["E"][1].any()                             # class 1 is not in the batch
    h = 1e-6
    for name, entries in (("E", [(2, 0), (0, 5), (2, 7), (1, 3)]), ("V", [(0, 0), (37, 4), (191, 7), (100, 2)])):
        for i, j in entries:
            vals = []
            for s in (+1, -1):
                A = {"E": E.copy(), "V": V.copy()}
                A[name][i, j] += s * h
                vals.append(cond_ref.loss_only(p, w, A["E"], A["V"], ids, idx, tgt))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[name][i, j]) <= 1e-7 + 1e-5 * abs(fd), (name, i, j, fd, g[name][i, j])


# ---- the model: new links after the head, nothing else moves ---------------------------------------------------------------
def test_state_dict_keys_and_shapes_of_a_conditioned_model():
    p = Params(R.make_params(**cond_ref.TINY))
    net = WaveNet(p, seed=0, condition_classes=3, condition_channels=8)
    sd = net.state_dict()
    assert sd["global_condition_embed/W"].shape == (3, 8, 1, 1)
    assert sd["global_condition_projection/W"].shape == (6 * 2 * 32, 8, 1, 1)
    assert list(sd)[-2:] == ["global_condition_embed/W", "global_condition_projection/W"]
    assert [ln.name for ln in net.links()][-2:] == ["global_condition_embed", "global_condition_projection"]
    assert net._cond_offsets == [(64 * l, 64 * l + 32) for l in range(6)] and net._cond_rows == 384
    f = FasterWaveNet(p, seed=0, condition_classes=3, condition_channels=8)
    assert set(f.state_dict()) == set(sd)


def test_an_unconditioned_model_is_what_it_was():
    """Same parameter count, same arena layout, same seeded draws: the conditioned model's arena BEGINS with the
    unconditioned one's, bit for bit."""
    p = Params(R.make_params(**cond_ref.TINY))
    plain, cond = WaveNet(p, seed=5), WaveNet(p, seed=5, condition_classes=3, condition_channels=8)
    want = sum(int(np.prod(ws)) + (bs[0] if bs else 0) for _, ws, bs in R.weight_specs(p.to_dict()))
    assert plain.num_parameters == want
    assert cond.num_parameters == want + 3 * 8 + 384 * 8
    n = plain._arena.numel()
    assert [(ln.name, k, o, m) for ln, k, o, m, _ in plain._spans] == [(ln.name, k, o, m) for ln, k, o, m, _ in cond._spans[:-2]]
    assert torch.equal(plain._arena, cond._arena[:n])
    assert plain.condition_classes == 0 and not any(k.startswith("global_condition") for k in plain.state_dict())


def test_params_keep_their_key_set():
    keys = set(Params().to_dict())
    assert not any("condition" in k or "speaker" in k for k in keys)
    p = Params(R.make_params(**cond_ref.TINY))
    WaveNet(p, seed=0, condition_classes=2, condition_channels=4)
    assert set(p.to_dict()) == keys


def test_constructor_and_checkpoint_mismatches_raise_clearly():
    p = Params(R.make_params(**cond_ref.TINY))
    with pytest.raises(Exception, match="condition_classes > 0 and condition_channels > 0"):
        WaveNet(p, seed=0, condition_classes=3)
    pw = Params(R.make_params(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 2,
                              residual_num_blocks=1, softmax_conv_channels=[256, 256]))
    with pytest.raises(Exception, match="bf16"):
        WaveNet(pw, seed=0, storage="bf16", condition_classes=3, condition_channels=8)
    pb = Params(R.make_params(**dict(cond_ref.TINY, residual_conv_dilation_no_bias=False)))
    with pytest.raises(Exception, match="residual_conv_dilation_no_bias"):
        WaveNet(pb, seed=0, condition_classes=3, condition_channels=8)
    plain, cond = WaveNet(p, seed=0), WaveNet(p, seed=0, condition_classes=3, condition_channels=8)
    with pytest.raises(Exception, match="checkpoint is globally conditioned"):
        plain.load_state_dict(cond.state_dict())
    with pytest.raises(Exception, match="model is globally conditioned and the checkpoint is not"):
        cond.load_state_dict(plain.state_dict())
    other = WaveNet(p, seed=0, condition_classes=4, condition_channels=8)
    with pytest.raises(Exception, match="shape of global_condition_embed/W"):
        cond.load_state_dict(other.state_dict())
    # ids: a conditioned model needs them, an unconditioned one refuses them, and they are range-checked on the host
    with pytest.raises(Exception, match="pass condition="):
        cond._condition_ids(None, 3)
    with pytest.raises(Exception, match="no global conditioning"):
        plain._condition_ids([0, 1, 2], 3)
    with pytest.raises(Exception, match=r"must lie in \[0, 3\)"):
        cond._condition_ids([0, 3, 1], 3)
    with pytest.raises(Exception, match="2 class ids for 3 clips"):
        cond._condition_ids([0, 1], 3)
    assert plain._condition_ids(None, 3) is None
    assert cond._condition_ids([2, 0, 2], 3).tolist() == [2, 0, 2]


def test_checkpoint_files_round_trip_the_conditioning_tensors_on_the_host(tmp_path):
    p = Params(R.make_params(**cond_ref.TINY))
    a = WaveNet(p, seed=1, condition_classes=3, condition_channels=8)
    a.save(str(tmp_path))
    b = WaveNet(p, seed=2, condition_classes=3, condition_channels=8)
    assert not np.array_equal(a.state_dict()["global_condition_embed/W"], b.state_dict()["global_condition_embed/W"])
    b.load(str(tmp_path))
    for k, v in a.state_dict().items():
        assert np.array_equal(v, b.state_dict()[k]), k
    with pytest.raises(Exception, match="globally conditioned"):
        WaveNet(p, seed=2).load(str(tmp_path))


# ---- the header -----------------------------------------------------------------------------------------------------------
def test_header_defines_the_flag_as_bit_2_and_keeps_its_69_functions_at_version_5():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.findall(r"^#define\s+WN_EXEC_BIAS_PER_CLIP\s+(\w+)", hdr, flags=re.M) == ["2u"]
    assert re.findall(r"^#define\s+WN_ABI_VERSION\s+(\d+)", hdr, flags=re.M) == ["5"]
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 69 and declared == set(_lib.EXPORTS)
    assert _lib.WN_EXEC_BIAS_PER_CLIP == 2 and _lib.ABI_VERSION == 5
    # every other flag keeps its bit
    flags = dict(re.findall(r"^#define\s+(WN_EXEC_\w+)\s+(\d+)u", hdr, flags=re.M))
    assert flags == {"WN_EXEC_FORCE_GENERIC": "1", "WN_EXEC_BIAS_PER_CLIP": "2", "WN_EXEC_NO_FWD_GROUPS": "4",
                     "WN_EXEC_NO_PIPELINED_GEMM": "8", "WN_EXEC_NO_MULTI_LAYER_BWD": "16", "WN_EXEC_HEAD_ROW_NLL": "32"}
    # the struct layout did not change: the stride travels in the field that was reserved
    assert [f[0] for f in _lib.WnExec._fields_] == ["precision", "flags", "ws", "ws_bytes", "fwd_t1_min_blocks", "reserved", "plan"]


# ---- speakers on the command line -----------------------------------------------------------------------------------------
def test_speaker_label_parsing():
    assert speakers.speaker_label("p225_001.wav") == "p225"
    assert speakers.speaker_label("/data/vctk/p304_17_mic2.WAV") == "p304"
    assert speakers.speaker_label("solo.wav") == "solo"
    with pytest.raises(ValueError, match="no speaker label"):
        speakers.speaker_label("_x.wav")
    assert speakers.label_table(["p300_2.wav", "p225_1.wav", "p225_2.wav", "b.wav"]) == ["b", "p225", "p300"]


def test_speakers_json_round_trip_and_a_resumed_run_must_find_the_same_table(tmp_path):
    d = str(tmp_path / "model")
    assert speakers.load_table(d) is None
    assert speakers.ensure_table(d, ["p225", "p300"], 16) == (["p225", "p300"], 16)
    with open(os.path.join(d, "speakers.json")) as f:
        assert json.load(f) == {"speakers": ["p225", "p300"], "condition_channels": 16}
    assert speakers.load_table(d) == (["p225", "p300"], 16)
    assert speakers.ensure_table(d, ["p225", "p300"], 16) == (["p225", "p300"], 16)          # the resumed run
    with pytest.raises(SystemExit, match="same table"):
        speakers.ensure_table(d, ["p225", "p300", "p301"], 16)
    with pytest.raises(SystemExit, match="same table"):
        speakers.ensure_table(d, ["p225", "p300"], 8)
    assert not os.path.exists(os.path.join(d, "wavenet.json"))                               # that file is not this one's business
    (tmp_path / "model" / "speakers.json").write_text("{broken")
    with pytest.raises(Exception, match="could not load"):
        speakers.load_table(d)


def test_speaker_lookup_errors_are_clear():
    t = ["p225", "p300"]
    assert speakers.class_id(t, "p300", "generate") == 1
    assert speakers.class_id(None, None, "generate") is None
    with pytest.raises(SystemExit, match="unknown speaker 'p999'"):
        speakers.class_id(t, "p999", "generate")
    with pytest.raises(SystemExit, match="not conditioned on speakers"):
        speakers.class_id(None, "p225", "generate")
    with pytest.raises(SystemExit, match="name one"):
        speakers.class_id(t, None, "generate")
    assert speakers.utterance_speakers(None, 3) == [None] * 3
    assert speakers.utterance_speakers(["a"], 3) == ["a"] * 3
    assert speakers.utterance_speakers(["a", "b", "c"], 3) == ["a", "b", "c"]
    with pytest.raises(ValueError, match="one for all of them, or one each"):
        speakers.utterance_speakers(["a", "b"], 3)


def test_cli_argument_errors_and_defaults(tmp_path):
    a = cli_args.parse([])
    assert (a.speaker_prefix, a.condition_channels, a.speaker) == (False, None, None)
    assert "speaker" not in vars(a) and "speaker_prefix" not in vars(a)      # attributes of the namespace only when given
    a = cli_args.parse(["--speaker-prefix", "--condition-channels", "16"])
    assert (a.speaker_prefix, a.condition_channels) == (True, 16)
    a = cli_args.parse(["--utterances", "2", "--speaker", "p225", "--speaker", "p300"])
    assert a.speaker == ["p225", "p300"]
    for argv in (["--speaker-prefix"], ["--condition-channels", "8"], ["--speaker-prefix", "--condition-channels", "0"],
                 ["--utterances", "3", "--speaker", "a", "--speaker", "b"]):
        with pytest.raises(SystemExit):
            cli_args.parse(argv)
    # model.build: the table decides whether the network is conditioned (checked up to the device, which this box lacks)
    d = tmp_path / "m"
    d.mkdir()
    (d / "wavenet.json").write_text(json.dumps(dict(cond_ref.TINY)))
    w = tmp_path / "wav"
    w.mkdir()
    for fn in ("p225_001.wav", "p225_002.wav", "p300_001.wav"):
        (w / fn).write_bytes(b"")
    a = cli_args.parse(["-g", "-1", "-m", str(d), "-w", str(w), "--speaker-prefix", "--condition-channels", "8"])
    with pytest.raises(Exception, match="not supported"):
        cli_model.build(a)
    assert speakers.load_table(str(d)) == (["p225", "p300"], 8)
    with open(str(d / "wavenet.json")) as f:
        assert set(json.load(f)) == set(cond_ref.TINY)                       # wavenet.json is unchanged
    (w / "p301_001.wav").write_bytes(b"")
    with pytest.raises(SystemExit, match="same table"):
        cli_model.build(a)
    from wavenet_amd.train_audio import generate
    with pytest.raises(SystemExit, match="unknown speaker"):
        generate.main(["-g", "-1", "-m", str(d), "--speaker", "nobody"])
    with pytest.raises(SystemExit, match="name one"):
        generate.main(["-g", "-1", "-m", str(d)])
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "wavenet.json").write_text(json.dumps(dict(cond_ref.TINY)))
    with pytest.raises(SystemExit, match="not conditioned on speakers"):
        generate.main(["-g", "-1", "-m", str(plain), "--speaker", "p225"])
