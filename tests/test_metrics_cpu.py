"""The copy-synthesis metrics on values worked out by hand, and the command lines that use them: what they parse to and what
they refuse before a model is built."""
import json
import math

import numpy as np
import pytest
import torch

from wavenet_amd import metrics


def test_log_mel_distance_is_zero_on_equal_inputs_and_20_over_ln10_x_db_for_an_offset_of_x_nats():
    a = np.random.RandomState(0).randn(8, 5)
    mean, per_column = metrics.log_mel_distance(a, a.copy())
    assert mean == 0.0 and per_column.shape == (5,) and (per_column == 0.0).all()
    mean, per_column = metrics.log_mel_distance(a, a - 0.5)
    assert abs(mean - 0.5 * 20.0 / math.log(10.0)) < 1e-12 and np.abs(per_column - 4.342944819032518).max() < 1e-12
    # one channel of two off by 1 nat in column 0, both off by 2 nats in column 1: rms = sqrt(1 / 2), 2
    b = np.zeros((2, 2))
    b[0, 0], b[:, 1] = 1.0, 2.0
    mean, per_column = metrics.log_mel_distance(np.zeros((2, 2)), b)
    k = 20.0 / math.log(10.0)
    assert np.allclose(per_column, [k * math.sqrt(0.5), 2 * k], rtol=1e-14) and abs(mean - k * (math.sqrt(0.5) + 2) / 2) < 1e-12
    assert metrics.log_mel_distance(np.zeros((3, 0)), np.zeros((3, 0)))[0] is None
    with pytest.raises(ValueError, match="one shape"):
        metrics.log_mel_distance(np.zeros((3, 2)), np.zeros((3, 3)))
    assert metrics.log_mel_distance(torch.zeros(2, 2), torch.as_tensor(b))[0] == mean


def test_f0_metrics_an_octave_is_1200_cents_and_a_gross_error():
    ref = np.array([[100.0, 200.0, 0.0, 150.0, 0.0], [0.1, 0.1, 0.9, 0.1, 0.9]])
    got = ref.copy()
    same = metrics.f0_metrics(ref, got)
    assert same == {"frames": 5, "voiced_frames": 3, "f0_rmse_cents": 0.0, "f0_gross_error": 0.0, "vuv_error": 0.0}
    got[0] = [200.0, 200.0, 120.0, 0.0, 0.0]             # an octave up; right; voiced where the reference is not; the reverse; right
    m = metrics.f0_metrics(ref, got)
    assert m["voiced_frames"] == 2 and abs(m["vuv_error"] - 2 / 5) < 1e-15
    assert abs(m["f0_rmse_cents"] - math.sqrt(1200.0 ** 2 / 2)) < 1e-9 and m["f0_gross_error"] == 0.5
    got[0] = [119.0, 241.0, 0.0, 150.0, 0.0]             # 19 % is no gross error, 20.5 % is one
    m = metrics.f0_metrics(ref, got)
    assert m["f0_gross_error"] == 1 / 3 and m["vuv_error"] == 0.0
    want = math.sqrt((((1200 * math.log2(1.19)) ** 2) + (1200 * math.log2(1.205)) ** 2) / 3)
    assert abs(m["f0_rmse_cents"] - want) < 1e-9


def test_f0_metrics_gives_none_not_nan_where_nothing_is_averaged():
    ref = np.array([[100.0, 0.0], [0.1, 0.9]])
    got = np.array([[0.0, 90.0], [0.9, 0.1]])
    m = metrics.f0_metrics(ref, got)
    assert m["voiced_frames"] == 0 and m["f0_rmse_cents"] is None and m["f0_gross_error"] is None and m["vuv_error"] == 1.0
    m = metrics.f0_metrics(np.zeros((2, 0)), np.zeros((2, 0)))
    assert m == {"frames": 0, "voiced_frames": 0, "f0_rmse_cents": None, "f0_gross_error": None, "vuv_error": None}
    json.dumps(m)
    with pytest.raises(ValueError, match=r"\(2, n\)"):
        metrics.f0_metrics(np.zeros((3, 2)), np.zeros((3, 2)))


def test_pick_closest_is_the_smallest_distance_the_lowest_index_on_ties_and_never_none_or_nan():
    assert metrics.pick_closest([3.0, 1.0, 2.0]) == 1 and metrics.pick_closest([2.0, 1.0, 1.0]) == 1
    assert metrics.pick_closest([None, float("nan"), 5.0]) == 2 and metrics.pick_closest([None, None]) == 0
    with pytest.raises(ValueError, match="no candidate"):
        metrics.pick_closest([])


def test_the_first_compared_column_is_the_first_whose_span_starts_behind_the_window():
    # W = 15, win 64, hop 16: column k spans k * 16 - 32 .. k * 16 + 31; column 3 starts at sample 16 >= 15, column 2 at 0
    assert metrics.first_free_column(15, 64, 16) == 3 and metrics.first_free_column(16, 64, 16) == 3
    assert metrics.first_free_column(17, 64, 16) == 4 and metrics.first_free_column(0, 64, 16) == 2
    assert metrics.first_free_column(15, 105, 16) == 5                     # S = 105: from k * 16 - 52 on; 5 * 16 - 52 = 28, 4 * 16 - 52 = 12


def test_total_weights_every_figure_by_what_it_was_averaged_over():
    rows = [dict(samples=100, emitted=np.zeros(90), log_mel_distance_db=2.0, mel_columns=4, f0_rmse_cents=30.0, f0_gross_error=0.5,
                 voiced_frames=2, vuv_error=0.25, pitch_columns=4, nats_per_sample=1.0),
            dict(samples=50, emitted=np.zeros(10), log_mel_distance_db=5.0, mel_columns=2, f0_rmse_cents=None, f0_gross_error=None,
                 voiced_frames=0, vuv_error=None, pitch_columns=0, nats_per_sample=3.0),
            dict(samples=60, emitted=np.zeros(50), log_mel_distance_db=None, mel_columns=0, f0_rmse_cents=40.0, f0_gross_error=0.0,
                 voiced_frames=6, vuv_error=0.5, pitch_columns=12, nats_per_sample=2.0)]
    t = metrics.total(rows)
    assert t["samples"] == 210 and t["voiced_frames"] == 8
    assert abs(t["log_mel_distance_db"] - (2.0 * 4 + 5.0 * 2) / 6) < 1e-12
    assert abs(t["f0_rmse_cents"] - math.sqrt((900.0 * 2 + 1600.0 * 6) / 8)) < 1e-12 and t["f0_gross_error"] == 0.125
    assert abs(t["vuv_error"] - (0.25 * 4 + 0.5 * 12) / 16) < 1e-12
    assert abs(t["nats_per_sample"] - (90 * 1.0 + 10 * 3.0 + 50 * 2.0) / 150) < 1e-12
    none = metrics.total([rows[1]])
    assert none["f0_rmse_cents"] is None and none["vuv_error"] is None and none["log_mel_distance_db"] == 5.0


# ---- the command lines ------------------------------------------------------------------------------------------------------------
def _no_model(monkeypatch):
    from wavenet_amd.train_audio import model as cli_model

    def build(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli_model, "build", build)


def test_without_the_new_flags_both_parsers_give_the_namespace_they_gave():
    from wavenet_amd.train_audio import args as cli_args
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    for argv in ([], ["--fast", "--from-wav", "f.wav", "--best-of", "3"], ["--fast", "--keep", "k.wav"], ["--local-mel", "--mels", "8"]):
        without, with_flag = cli_args.parse(argv), cli_args.parse(argv + ["--rank", "mel"])
        assert "rank" not in vars(without) and without.rank == "likelihood" and with_flag.rank == "mel"
        assert {k: v for k, v in vars(with_flag).items() if k != "rank"} == vars(without)
    assert vars(cli_evaluate.build_parser().parse_args([])) == {
        "gpu_device": 0, "wav_dir": "wav", "model_dir": "model", "chunk_width": 16384, "batch_size": 8, "json": None}
    got = vars(cli_evaluate.build_parser().parse_args(["--copy-synthesis", "--seconds", "1.5", "--seed", "3", "--temperature", "0.9",
                                                       "--top-k", "5", "--top-p", "0.8"]))
    assert {k: got[k] for k in ("copy_synthesis", "seconds", "seed", "temperature", "top_k", "top_p")} == {
        "copy_synthesis": True, "seconds": 1.5, "seed": 3, "temperature": 0.9, "top_k": 5, "top_p": 0.8}


@pytest.mark.parametrize("argv,word", [
    (["--fast", "--rank", "mel"], "--rank mel compares every candidate with the columns of the recording.*give --from-wav FILE.wav"),
    (["--fast", "--local", "f.npy", "--rank", "mel"], "--from-wav FILE.wav \\(it does not go with --local\\)"),
    (["--fast", "--keep", "k.wav", "--rank", "mel"], "it does not go with --keep"),
    (["--fast", "--local-dir", "d", "--rank", "mel"], "it does not go with --local-dir"),
    (["--fast", "--from-wav", "f.wav", "--chunk-frames", "4", "--rank", "mel"], "--rank mel .* does not go with --chunk-frames"),
    (["--fast", "--from-wav", "f.wav", "--rank", "closest"], "--rank takes likelihood or mel, got 'closest'"),
])
def test_generate_refuses_rank_mel_without_a_recording_before_a_model_is_built(tmp_path, monkeypatch, argv, word):
    from wavenet_amd.train_audio import generate as cli_generate
    _no_model(monkeypatch)
    with pytest.raises(SystemExit, match=word):
        cli_generate.main(["-m", str(tmp_path / "model"), "-o", str(tmp_path / "out")] + argv)


def test_evaluate_refuses_copy_synthesis_without_mel_parameters_before_a_model_is_built(tmp_path, monkeypatch):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    _no_model(monkeypatch)
    model = tmp_path / "model"
    model.mkdir()
    base = ["-w", str(tmp_path), "-m", str(model)]
    with pytest.raises(SystemExit, match="--copy-synthesis .* needs the mel parameters .*local.json has no \"mel\""):
        cli_evaluate.main(base + ["--copy-synthesis"])
    (model / "local.json").write_text(json.dumps({"channels": 8, "hop": 16}))
    with pytest.raises(SystemExit, match="has no \"mel\""):
        cli_evaluate.main(base + ["--copy-synthesis", "--seed", "1"])
    with pytest.raises(SystemExit, match="--seed goes with --copy-synthesis"):
        cli_evaluate.main(base + ["--seed", "1"])
    with pytest.raises(SystemExit, match="--seconds, --top-k go with --copy-synthesis"):
        cli_evaluate.main(base + ["--seconds", "1", "--top-k", "4"])
    (model / "local.json").write_text(json.dumps({"channels": 8, "hop": 16, "mel": {"win": 64}}))
    with pytest.raises(SystemExit, match="--seconds S needs S > 0"):
        cli_evaluate.main(base + ["--copy-synthesis", "--seconds", "0"])
    with pytest.raises(AssertionError, match="a model was built"):          # everything checked: the model comes next
        cli_evaluate.main(base + ["--copy-synthesis", "--seconds", "1"])


def test_a_report_without_distances_is_what_it_was_and_with_them_gains_rank_and_a_distance_per_file(tmp_path):
    from wavenet_amd.train_audio import generate as cli_generate
    ranked = [(1, [2.0, 1.5, 3.0])]
    plain = cli_generate.write_report(str(tmp_path / "a.json"), ["out/generated.wav"], [np.zeros(10, np.int32)], ranked, 3)
    assert sorted(plain) == ["files", "total"] and sorted(plain["files"][0]) == sorted(
        ["file", "samples", "nats_per_sample", "bits_per_sample", "candidates", "kept"])
    mel = cli_generate.write_report(str(tmp_path / "b.json"), ["out/generated.wav"], [np.zeros(10, np.int32)], ranked, 3, [4.25])
    assert mel["rank"] == "mel" and mel["files"][0]["log_mel_distance_db"] == 4.25
    assert {k: v for k, v in mel["files"][0].items() if k != "log_mel_distance_db"} == plain["files"][0] and mel["total"] == plain["total"]
    assert json.loads((tmp_path / "b.json").read_text()) == mel
