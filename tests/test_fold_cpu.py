"""Folded decoding without a GPU: the rule of wavenet_amd/fold.py against the brute force of tests/fold_ref.py, the file bytes, and
every refusal of ``FasterWaveNet.generate_folded`` and of ``generate --fold`` -- made before a model is built or a device touched."""
import json

import numpy as np
import pytest

import fold_ref
from wavenet_amd import FasterWaveNet, Params, data, fold
from wavenet_amd.wavenet import coarse_frames_needed

# n < B | n = k B | n = k B + O and one more | O = 0 and O = B | W = 0 | W > a_1 (the clamp: segment 1 starts at 0)
GRID = [(n, B, O, W) for B, O in ((7, 3), (7, 0), (7, 7), (1, 0), (1, 1), (5, 2))
        for n in sorted({1, 2, B - 1, B, B + 1, 2 * B, 3 * B, 2 * B + O, 2 * B + O + 1, 3 * B + O, 3 * B + O + 1, 4 * B + 3} - {0})
        for W in (0, 2, B + 4)]


def test_the_grid_holds_the_cases_it_is_there_for():
    assert any(n < B for n, B, O, W in GRID) and any(n == 3 * B for n, B, O, W in GRID)
    assert any(n == 2 * B + O and O for n, B, O, W in GRID) and any(n == 2 * B + O + 1 and O for n, B, O, W in GRID)
    assert any(O == 0 for n, B, O, W in GRID) and any(O == B for n, B, O, W in GRID) and any(W == 0 for n, B, O, W in GRID)
    assert any(W > B and n > B + O for n, B, O, W in GRID)


@pytest.mark.parametrize("n,B,O,W", GRID)
def test_plans_equal_the_brute_force_and_keep_their_properties(n, B, O, W):
    plan = fold.fold_plan(n, B, O, W)
    a, b, s, e = fold_ref.plan(n, B, O, W)
    assert [tuple(g) for g in plan.segments] == list(zip(a, b, s, e))
    S = len(plan.segments)
    assert S == max(1, -(-(n - O) // B)) and (plan.n, plan.body, plan.overlap, plan.warmup) == (n, B, O, W)
    # the last-body rule
    assert all(g.b - g.a == B for g in plan.segments[:-1])
    last = plan.segments[-1]
    assert last.b == n and (S == 1 or O < last.b - last.a <= B + O) and last.b - last.a <= max(n, B + O)
    # segment 0 starts at 0; a clamped warm-up takes the utterance's window (s = 0)
    assert plan.segments[0].s == 0 and all(g.s == max(0, g.a - W) for g in plan.segments[1:])
    if W > B and S > 1:
        assert plan.segments[1].s == 0
    # one owner per position; at most two segments meet outside the warm-ups; the weights over a position sum to 1
    decoded, owners = fold_ref.covers(n, B, O, W)
    assert all(len(o) == 1 for o in owners) and all(1 <= len(d) <= 2 for d in decoded)
    assert fold.owner(plan).tolist() == [o[0] for o in owners]
    w = fold.fade_weights(plan)
    assert w.shape == (S, n) and np.array_equal(w.sum(axis=0), np.ones(n))
    for p in range(n):
        assert sorted(np.nonzero(w[:, p])[0].tolist()) == decoded[p] or (len(decoded[p]) == 2 and 0.0 in w[decoded[p], p])
    assert fold.useful_share(plan) == n / float(sum(y - x for x, y in zip(s, e)))


def test_fold_arguments_are_refused_by_name():
    for bad, word in (((10, 0, 0, 0), "body must be at least 1 sample, got 0"), ((10, 4, 5, 0), r"overlap must lie in \[0, body = 4\], got 5"),
                      ((10, 4, -1, 0), "overlap must lie in"), ((10, 4, 2, -3), "warmup must be >= 0 samples, got -3"),
                      ((0, 4, 2, 0), "n must be at least 1 sample, got 0"), ((10, 4.0, 2, 0), "body must be an integer")):
        with pytest.raises(ValueError, match=word):
            fold.fold_plan(*bad)


def test_auto_body_is_the_derived_bound():
    assert fold.auto_body(160000, 28, 256, 4094) == 4 * (4094 + 256)             # the 80 % term wins
    assert fold.auto_body(160000, 4, 5, 11) == 40000                           # the capacity term wins
    assert fold.auto_body(10, 4, 0, 0) == 3 and fold.auto_body(1, 100, 0, 0) == 1
    for n, cap, O, W in ((1000, 7, 5, 20), (99999, 256, 16, 300)):
        plan = fold.fold_plan(n, fold.auto_body(n, cap, O, W), O, W)
        assert len(plan.segments) <= cap and (len(plan.segments) == 1 or fold.useful_share(plan) >= 0.8)


COLUMN_CASES = [(hop, phase, interp, U) for hop in (5, 6) for phase in (0, 3) for interp in ("repeat", "linear") for U in (1, 2, 3)
                if hop % U == 0]


@pytest.mark.parametrize("hop,phase,interp,U", COLUMN_CASES)
def test_segment_columns_against_the_table_of_positions(hop, phase, interp, U):
    window = 13
    for n, B, O, W in ((83, 37, 8, 11), (83, 37, 8, 50), (200, 37, 8, 11), (30, 7, 7, 0), (9, 20, 3, 4)):
        plan = fold.fold_plan(n, B, O, W)
        whole = coarse_frames_needed(window + n - 1, hop, U, phase, interp)             # what generate(n, ...) itself asks for
        got = fold.check_columns(plan, window, phase, hop, interp, U, whole)
        for g, (first, count, ph) in zip(plan.segments, got):
            read = fold_ref.columns_read(g.s, g.e, window, phase, hop, interp, U)
            assert (first, ph) == divmod(g.s + phase, hop)
            assert read[0] == first and read[-1] == first + count - 1 and first + count <= whole, (g, read, first, count)
        # the last segment needs the utterance's last column -- under linear interpolation and behind a learned layer the column
        # behind the last position's own: one column fewer is refused, the segment and both counts named
        assert sum(got[-1][:2]) == whole
        k = [first + count == whole for first, count, _ in got].index(True)          # the first segment that reaches it is named
        with pytest.raises(ValueError, match=r"segment %d \(samples %d \.\. %d\) reads feature columns %d \.\. %d, the utterance has %d: "
                                             r"%d are needed" % (k, plan.segments[k].s, plan.segments[k].e, got[k][0], whole - 1,
                                                                 whole - 1, whole)):
            fold.check_columns(plan, window, phase, hop, interp, U, whole - 1)
    assert (5, "linear", 1) in {(h, i, u) for h, _, i, u in COLUMN_CASES} and (6, "linear", 3) in {(h, i, u) for h, _, i, u in COLUMN_CASES}


def test_unfold_by_hand_equal_sides_and_the_tie():
    table = np.arange(16, dtype=np.int16)                       # the value of token q is q
    plan = fold.fold_plan(6, 3, 2, 1)
    assert [tuple(g) for g in plan.segments] == [(0, 3, 0, 5), (3, 6, 2, 6)]
    # seam [3, 5): w = 0.25, 0.75.  0 + 0.25 * 2 = 0.5 -> 0 and 0 + 0.75 * 6 = 4.5 -> 4: half goes to even
    assert fold.unfold([[1, 2, 3, 0, 0], [9, 2, 6, 7]], plan, table).tolist() == [1, 2, 3, 0, 4, 7]
    # 0 + 0.25 * 6 = 1.5 -> 2 and 2 + 0.75 * (0 - 2) = 0.5 -> 0
    assert fold.unfold([[1, 2, 3, 0, 2], [9, 6, 0, 7]], plan, table).tolist() == [1, 2, 3, 2, 0, 7]
    # equal tokens on both sides give that token's value, whatever the weight; the warm-up sample (9) is never read
    rows = [[1, 2, 3, 11, 15], [9, 11, 15, 7]]
    assert fold.unfold(rows, plan, table).tolist() == [1, 2, 3, 11, 15, 7]
    assert fold.identical_seams(rows, plan) == 1 and fold.identical_seams([[1, 2, 3, 11, 14], [9, 11, 15, 7]], plan) == 0
    assert fold.gather_owner(rows, plan).tolist() == [1, 2, 3, 11, 15, 7]
    assert fold.unfold(rows, plan, table).dtype == np.int16
    with pytest.raises(ValueError, match="row 1 holds 3 samples, segment 1 decodes 4"):
        fold.unfold([[1, 2, 3, 0, 0], [9, 2, 6]], plan, table)
    # the clip: a table that leaves int16 by rounding cannot exist, but the rule is stated -- values at the rim stay
    rim = np.array([-32768, 32767], dtype=np.int16)
    assert fold.unfold([[0, 1, 0, 1, 1], [0, 1, 1, 0]], plan, rim).tolist() == [-32768, 32767, -32768, 32767, 32767, -32768]


@pytest.mark.parametrize("n,B,O,W", [(83, 37, 8, 11), (83, 37, 8, 50), (200, 37, 8, 11), (40, 8, 8, 3), (23, 5, 0, 2), (12, 30, 4, 4)])
def test_unfold_equals_the_brute_force_on_the_files_own_values(n, B, O, W):
    table = data.pcm_table(256)
    plan = fold.fold_plan(n, B, O, W)
    rs = np.random.RandomState(n + B)
    rows = [rs.randint(0, 256, (g.e - g.s,)).astype(np.int32) for g in plan.segments]
    for u in range(0, len(rows) - 1, 2):                     # every other seam: equal on both sides
        g, h = plan.segments[u], plan.segments[u + 1]
        rows[u + 1][g.b - h.s:g.b - h.s + O] = rows[u][g.b - g.s:g.b - g.s + O]
    got = fold.unfold(rows, plan, table)
    assert np.array_equal(got, fold_ref.unfold(rows, n, B, O, W, table))
    assert fold.identical_seams(rows, plan) == (len(rows) if O == 0 else len(rows) // 2) - (1 if O == 0 else 0)
    own = fold.owner(plan)
    for u in range(0, len(rows) - 1, 2):
        b = plan.segments[u].b
        assert np.array_equal(got[b:b + O], table[[rows[own[p]][p - plan.segments[own[p]].s] for p in range(b, b + O)]])


@pytest.mark.parametrize("Q", [256, 64])
def test_save_pcm_file_writes_the_bytes_of_save_audio_file(tmp_path, Q):
    tokens = np.concatenate([np.arange(Q), np.arange(Q)[::-1], [Q // 2] * 3]).astype(np.int32)
    table = data.pcm_table(Q)
    assert table.dtype == np.int16 and table.shape == (Q,)
    data.save_audio_file(str(tmp_path / "a.wav"), tokens, Q, format="16bit_pcm", sampling_rate=8000)
    data.save_pcm_file(str(tmp_path / "b.wav"), table[tokens], 8000)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    with pytest.raises(Exception, match="integer PCM values, got float"):
        data.save_pcm_file(str(tmp_path / "c.wav"), table[tokens].astype(np.float32), 8000)


# ---- the method's refusals: a model on the host, never moved to a device ------------------------------------------------------------
TINY = dict(quantization_steps=256, causal_conv_channels=[8], residual_conv_channels=[8] * 3, residual_num_blocks=2,
            softmax_conv_channels=[16, 256])


def test_generate_folded_refuses_before_any_device_work():
    plain = FasterWaveNet(Params(TINY), seed=0)
    with pytest.raises(ValueError, match=r"generate_folded: this model has no local conditioning \(local_channels = 0\)"):
        plain.generate_folded(50, np.zeros(50), 20)
    net = FasterWaveNet(Params(TINY), seed=0, local_channels=5, local_hop=5)
    W = net.input_width
    h = np.zeros((5, coarse_frames_needed(W + 49, 5, 1, 0, "repeat")), np.float32)
    u = np.zeros(50)
    for kw, word in ((dict(body=20, overlap=21), r"overlap must lie in \[0, body = 20\], got 21"),
                     (dict(body=0), "body must be at least 1 sample, got 0"),
                     (dict(body=4), r"overlap must lie in \[0, body = 4\], got 5"),            # the default overlap: local_hop
                     (dict(body=20, warmup=-1), "warmup must be >= 0 samples, got -1"),
                     (dict(body="auto", warmup=-1), "warmup must be >= 0 samples, got -1"),
                     (dict(body="car"), "body= takes samples per segment or \"auto\", got 'car'"),
                     (dict(body=20, forced=np.zeros(50, np.int32)), "forced= is not an argument of this method"),
                     (dict(body=20, tile=3), "tile= takes"),
                     (dict(body=20, local_phase=5), r"local_phase must lie in \[0, local_hop = 5\), got 5")):
        with pytest.raises(ValueError, match=word):
            net.generate_folded(50, u, local=h, **kw)
    with pytest.raises(ValueError, match=r"generate_folded: segment 2 \(samples %d \.\. 50\) reads feature columns \d+ \.\. %d, the "
                                         r"utterance has %d: %d are needed" % (40 - 11, h.shape[1] - 1, h.shape[1] - 1, h.shape[1])):
        net.generate_folded(50, u, 20, 5, 11, local=h[:, :-1])
    with pytest.raises(ValueError, match=r"generate_folded: utterance 1: segment 1 "):
        net.generate_folded([50, 50], [u, u], 30, 5, 11, local=[h, h[:, :-1]])
    with pytest.raises(Exception, match="utterance 0 has 49 uniforms for its 50 samples"):
        net.generate_folded(50, u[:49], 20, local=h)
    with pytest.raises(Exception, match="pass local="):
        net.generate_folded(50, u, 20)


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def _no_model(monkeypatch):
    from wavenet_amd.train_audio import model as cli_model

    def build(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(cli_model, "build", build)


def test_the_namespace_lacks_the_flags_unless_given_and_the_help_names_them():
    from wavenet_amd.train_audio import args as cli_args
    new = ("fold", "fold_overlap", "fold_warmup")
    for argv in ([], ["--fast", "--local", "f.npy"], ["--fast", "--local-dir", "feat", "--tile", "auto"]):
        without = cli_args.parse(argv)
        assert not set(new) & set(vars(without))
        assert (without.fold, without.fold_overlap, without.fold_warmup) == (None, None, None)
        given = cli_args.parse(argv + ["--fold", "auto", "--fold-overlap", "0.01", "--fold-warmup", "0.5"])
        assert {k: v for k, v in vars(given).items() if k not in new} == vars(without)
        assert (given.fold, given.fold_overlap, given.fold_warmup) == ("auto", 0.01, 0.5)
        assert cli_args.parse(argv + ["--fold", "1.5"]).fold == "1.5"
    text = cli_args.build_parser().format_help()
    assert "--fold FOLD" in text and "--fold-overlap FOLD_OVERLAP" in text and "--fold-warmup FOLD_WARMUP" in text


def test_generate_refuses_fold_before_a_model_is_built(tmp_path, monkeypatch):
    from wavenet_amd.train_audio import generate as cli_generate
    _no_model(monkeypatch)
    model = tmp_path / "model"
    model.mkdir()
    base = ["-m", str(model), "-o", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="--fold decodes the segments of an utterance in one batched run on the device: give --fast"):
        cli_generate.main(base + ["--local", "f.npy", "--fold", "1"])
    with pytest.raises(SystemExit, match="--fold needs a locally conditioned checkpoint .*local.json is missing"):
        cli_generate.main(base + ["--fast", "--fold", "1"])
    (model / "local.json").write_text(json.dumps({"channels": 5, "hop": 5}))
    fast = base + ["--fast", "--local", "f.npy"]
    for extra, word in ((["--chunk-frames", "4"], "--fold does not go with --chunk-frames"),
                        (["--best-of", "2"], "--fold does not go with --best-of 2"),
                        (["--rank", "likelihood"], "--fold does not go with --rank")):
        with pytest.raises(SystemExit, match=word):
            cli_generate.main(fast + ["--fold", "1"] + extra)
    with pytest.raises(SystemExit, match="--fold does not go with --keep"):
        cli_generate.main(base + ["--fast", "--keep", "k.wav", "--local", "f.npy", "--fold", "1"])
    for bad in ("0", "-1", "nan", "car", "0.00001"):
        with pytest.raises(SystemExit, match="--fold takes seconds .*or auto.*got %r" % bad):
            cli_generate.main(fast + ["--fold", bad])
    with pytest.raises(SystemExit, match="--fold-overlap takes seconds"):
        cli_generate.main(fast + ["--fold", "1", "--fold-overlap", "-0.5"])
    with pytest.raises(SystemExit, match="--fold-warmup takes seconds"):
        cli_generate.main(fast + ["--fold", "auto", "--fold-warmup", "-0.5"])
    with pytest.raises(SystemExit, match="--fold-overlap 2 is .* samples, more than the .* of --fold 1"):
        cli_generate.main(fast + ["--fold", "1", "--fold-overlap", "2"])
    with pytest.raises(SystemExit, match="--fold-overlap and --fold-warmup sizes the segments of a folded run: give --fold"):
        cli_generate.main(fast + ["--fold-overlap", "0.1", "--fold-warmup", "0.1"])
    sr = cli_generate._model.load_params(str(model)).sampling_rate
    job = cli_generate.fold_job(cli_generate._args.parse(fast + ["--fold", "0.5", "--fold-warmup", "0.25"]))
    assert job == (int(round(0.5 * sr)), None, int(round(0.25 * sr)))
    assert cli_generate.fold_job(cli_generate._args.parse(fast + ["--fold", "auto", "--fold-overlap", "0"])) == ("auto", 0, None)
    assert cli_generate.fold_job(cli_generate._args.parse(fast)) is None


def test_evaluate_takes_fold_with_copy_synthesis_only_and_checks_it_before_a_model_is_built(tmp_path, monkeypatch):
    from wavenet_amd.train_audio import evaluate as cli_evaluate
    _no_model(monkeypatch)
    model = tmp_path / "model"
    model.mkdir()
    (model / "local.json").write_text(json.dumps({"channels": 8, "hop": 16, "mel": {"win": 64}}))
    base = ["-w", str(tmp_path), "-m", str(model)]
    assert not {"fold", "fold_overlap", "fold_warmup"} & set(vars(cli_evaluate.build_parser().parse_args(base)))
    with pytest.raises(SystemExit, match="--fold, --fold-warmup go with --copy-synthesis"):
        cli_evaluate.main(base + ["--fold", "1", "--fold-warmup", "0.1"])
    with pytest.raises(SystemExit, match="evaluate: --fold takes seconds .*got 'car'"):
        cli_evaluate.main(base + ["--copy-synthesis", "--fold", "car"])
    with pytest.raises(SystemExit, match="evaluate: --fold-overlap sizes the segments of a folded run: give --fold"):
        cli_evaluate.main(base + ["--copy-synthesis", "--fold-overlap", "0.1"])
    sr = cli_evaluate._model.load_params(str(model)).sampling_rate
    args = cli_evaluate.build_parser().parse_args(base + ["--copy-synthesis", "--fold", "auto", "--fold-overlap", "0.5"])
    assert cli_evaluate.copy_synthesis_job(args) == {"fold": ("auto", int(round(0.5 * sr)), None)}
    with pytest.raises(AssertionError, match="a model was built"):          # everything checked: the model comes next
        cli_evaluate.main(base + ["--copy-synthesis", "--fold", "0.5"])
