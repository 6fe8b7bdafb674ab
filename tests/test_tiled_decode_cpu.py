"""Decoding in utterance tiles without a GPU: the header's define and the binding's constant (and an ABI and an export list that
did not move), ``tile_fit`` against the LDS formula, the ``"auto"`` policy ``pick_tile`` over a table, ``--tile`` on the command
line, and the refusals of ``tile=`` on models that never touch a device."""
import os
import re

import numpy as np
import pytest

from oracle import wavenet_ref as R
from wavenet_amd import FasterWaveNet, Params, _lib
from wavenet_amd.faster_wavenet import TILE_SIZES, check_tile, pick_tile, tile_fit, tile_lds_bytes
from wavenet_amd.train_audio import args as cli_args
from wavenet_amd.train_audio import generate as cli_generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFG5 = dict(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 10, residual_num_blocks=4,
            softmax_conv_channels=[512, 256])
CFG2 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10, residual_num_blocks=4,
            softmax_conv_channels=[256, 256])
A = dict(quantization_steps=256, causal_conv_channels=[16], residual_conv_channels=[16] * 4, residual_num_blocks=2,
         softmax_conv_channels=[32, 256])


def test_the_header_and_the_binding_agree_and_the_abi_did_not_move():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.findall(r"^#define\s+WN_DECODER_TILE_MAX\s+(\d+)\b", hdr, flags=re.M) == ["16"]
    assert _lib.WN_DECODER_TILE_MAX == 16 == max(TILE_SIZES)
    assert re.findall(r"^#define\s+WN_DECODER_BATCH_MAX_ANY\s+(\d+)\b", hdr, flags=re.M) == [str(_lib.WN_DECODER_BATCH_MAX_ANY)]
    declared = set(re.findall(r"\b(wn(?:16)?_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS) and len(_lib.EXPORTS) == 69
    assert _lib.ABI_VERSION == 5 == int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1))
    # the table of same_weights is documented at wn_decoder_run_batch
    doc = hdr[:hdr.index("int wn_decoder_run_batch(")]
    assert "2, 4, 8, 16" in doc and "treated as 1" in doc


def _lds(maxc, U):
    return U * (7 * maxc + 16) * 4


@pytest.mark.parametrize("cfg, maxc, fit", [(CFG5, 512, 8), (CFG2, 256, 16), (A, 256, 16)], ids=["config5", "config2", "A"])
def test_tile_fit_is_the_lds_rule(cfg, maxc, fit):
    """A tile keeps U x (7 maxc + 16) floats; the bound is 150 KiB: U <= 8 for config 5 (maxc = 512), 16 for maxc <= 256."""
    pp = Params(R.make_params(**cfg))
    for U in (1,) + TILE_SIZES:
        assert tile_lds_bytes(pp, U) == _lds(maxc, U)
    assert tile_fit(pp) == fit == max(U for U in (1,) + TILE_SIZES if _lds(maxc, U) <= 150 * 1024)
    if fit < 16:
        assert _lds(maxc, 2 * fit) > 150 * 1024


def test_tile_fit_of_a_model_too_wide_for_any_tile_is_one():
    wide = dict(A, softmax_conv_channels=[4096, 256])
    assert tile_fit(Params(R.make_params(**wide))) == 1


PICKS = [
    # (N, n_cu, fit) -> U.  The measured rule (profiles/tiled_decode.json): 2 wherever a tile applies -- at every measured N
    # U = 2 was the fastest and every larger U slower --, off for one utterance and for a model no tile fits
    ((1, 256, 16), 0), ((2, 256, 16), 2), ((16, 256, 16), 2), ((64, 256, 16), 2), ((256, 256, 16), 2), ((1024, 256, 16), 2),
    ((16, 256, 8), 2), ((64, 256, 8), 2), ((256, 256, 8), 2), ((1024, 256, 8), 2), ((1024, 256, 2), 2), ((1024, 256, 1), 0),
    ((3, 8, 16), 2), ((1024, 304, 4), 2), ((1, 8, 2), 0),
]
# what was measured: (shape's tile_fit, N) -> the tile size with the best median rate (profiles/tiled_decode.json)
MEASURED_BEST = {(16, 16): 2, (16, 64): 2, (16, 256): 2, (16, 1024): 2, (8, 16): 2, (8, 64): 2, (8, 256): 2, (8, 1024): 2}


@pytest.mark.parametrize("args, want", PICKS)
def test_pick_tile_over_a_table(args, want):
    assert pick_tile(*args) == want
    assert want == 0 or (want in TILE_SIZES and want <= args[2])


def test_pick_tile_picks_the_best_measured_size_at_every_measured_point():
    import json
    doc = json.load(open(os.path.join(ROOT, "profiles", "tiled_decode.json")))
    seen = {}
    for shape in doc["shapes"].values():
        for N, row in shape["batches"].items():
            rates = {k: v["median_tokens_per_s"] for k, v in row.items() if k == "off" or k.isdigit()}
            best = max(rates, key=rates.get)
            seen[(shape["tile_fit"], int(N))] = 0 if best == "off" else int(best)
            pick = pick_tile(int(N), shape["n_cu"], shape["tile_fit"])
            assert rates[str(pick) if pick else "off"] >= rates[best] * (1.0 - row["parent_spread"]), (N, pick, best)
            assert row["checksums_equal"]
    assert seen == MEASURED_BEST


def test_the_tile_flag_on_the_command_line(tmp_path, monkeypatch):
    def no_model(*a, **kw):
        raise AssertionError("the model was built")
    monkeypatch.setattr(cli_generate._model, "build", no_model)
    m = str(tmp_path / "model")
    with pytest.raises(SystemExit, match="give --fast"):
        cli_generate.main(["-m", m, "--utterances", "4", "--tile", "4"])
    for bad in ("3", "32", "0", "1", "Auto", "4.0", "-2"):
        with pytest.raises(SystemExit, match="--tile takes auto, 2, 4, 8 or 16"):
            cli_generate.main(["-m", m, "--fast", "--utterances", "4", "--tile", bad])
    assert not os.path.exists(m)
    for given, want in (("auto", "auto"), ("2", 2), ("4", 4), ("8", 8), ("16", 16)):
        a = cli_args.parse(["--fast", "--utterances", "3", "--prompt", "p.wav", "--speaker", "p225", "--best-of", "2", "--report", "r.json",
                            "--tile", given])
        assert cli_generate.tile_job(a) == want
    for argv in (["--fast", "--local", "a.npy", "--chunk-frames", "4", "--tile", "8"], ["--fast", "--keep", "k.wav", "--tile", "auto"],
                 ["--fast", "--local-dir", "feats", "--tile", "2"]):
        assert cli_generate.tile_job(cli_args.parse(argv)) is not None
    # an attribute of the namespace only when given
    for argv in ([], ["--fast", "--best-of", "4", "--report", "r.json"], ["--fast", "--local", "a.npy", "--chunk-frames", "4"]):
        a = cli_args.parse(argv)
        assert a.tile is None and "tile" not in vars(a) and cli_generate.tile_job(a) is None
    assert "tile" in vars(cli_args.parse(["--fast", "--tile", "auto"]))
    assert "--tile" in " ".join(cli_args.build_parser().format_help().split())


def test_tile_is_validated_without_a_device():
    assert [check_tile(t) for t in (0, 1, 2, 4, 8, 16, "auto", np.int64(8))] == [0, 0, 2, 4, 8, 16, "auto", 8]
    for bad in (3, 32, -1, 5, 2.0, "4", "AUTO", True, None, [4]):
        with pytest.raises(ValueError, match=r"tile= takes 0 / 1 \(off\), 2, 4, 8, 16 or \"auto\""):
            check_tile(bad)
    net = FasterWaveNet(Params(R.make_params(**A)), seed=0)                    # never moved to a device
    assert FasterWaveNet.batch_tile == 0 and net.batch_tile == 0
    u = np.zeros((3, 4)) + 0.5
    with pytest.raises(ValueError, match=r"generate_batch: tile= takes .* got 3"):
        net.generate_batch(4, u, tile=3)
    with pytest.raises(ValueError, match=r"open_stream: tile= takes .* got 'four'"):
        net.open_stream(utterances=3, tile="four")
    net.batch_tile = 5                                                         # the attribute is checked like the argument
    with pytest.raises(ValueError, match="got 5"):
        net.generate_batch(4, u)
    del net.batch_tile
    # a U that does not fit names tile_fit's value, before anything else is looked at
    wide = FasterWaveNet(Params(R.make_params(**dict(A, softmax_conv_channels=[512, 256]))), seed=0)
    assert tile_fit(wide.params) == 8
    with pytest.raises(ValueError, match=r"tile=16 does not fit this model.*230400 bytes.*153600.*\(tile_fit\) is 8"):
        wide.generate_batch(4, u, tile=16)
    with pytest.raises(ValueError, match=r"open_stream: tile=16 does not fit"):
        wide.open_stream(utterances=3, tile=16)
    assert check_tile(8, wide.params) == 8 and check_tile("auto", wide.params) == "auto"
