"""Evaluation driver (new; the reference has none): the model's negative log-likelihood on every .wav file of a directory,
teacher-forced, in nats and bits per sample -- the held-out number that tells overfitting from learning.

    python -m wavenet_amd.train_audio.evaluate -w held_out_wav -m model [--ema] [--json scores.json]
    python -m wavenet_amd.train_audio.evaluate -w held_out_wav -m model --copy-synthesis [--seconds S] [--seed N] [--json FILE]
                                               [--fold SECONDS|auto [--fold-overlap SECONDS] [--fold-warmup SECONDS]]

Files are read as training reads them (mu-law tokens, silence trimmed) and scored by ``WaveNet.score``.  The command has
its own parser: it shares ``-g / -w / -m`` with train and generate and takes none of their other flags."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

from .. import data, scoring
from . import launch as _launch
from . import local as _local
from . import model as _model
from . import speakers as _speakers


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-g", "--gpu_device", type=int, default=0, help="HIP device index")
    ap.add_argument("-w", "--wav-dir", type=str, default="wav", help="directory of .wav files to score")
    ap.add_argument("-m", "--model-dir", type=str, default="model", help="wavenet.json + checkpoints")
    ap.add_argument("--chunk-width", type=int, default=16384, help="scored samples per piece of a file")
    ap.add_argument("--batch-size", type=int, default=8, help="pieces per launch")
    # present in the namespace only when given (train_audio.model.build reads it with a default of off)
    ap.add_argument("--ema", action="store_true", default=argparse.SUPPRESS,
                    help="score the checkpoint's averaged weights (wavenet.ema.npz, written by train --ema-decay)")
    ap.add_argument("--local-dir", type=str, default=argparse.SUPPRESS, metavar="FEAT_DIR",
                    help="the files' features, NAME.npy per NAME.wav (a locally conditioned checkpoint needs them)")
    ap.add_argument("--local-mel", action="store_true", default=argparse.SUPPRESS,
                    help="score every file under the log-mel features of the file itself, made on the device (a checkpoint trained "
                         "with train --local-mel); --local-dir, when given too, wins")
    ap.add_argument("--resample", action="store_true", default=argparse.SUPPRESS,
                    help="bring every file to the model's sampling_rate on the device before it is encoded (and make --local-mel "
                         "features at that rate); without it a file's samples are taken as they are, whatever its rate")
    ap.add_argument("--json", type=str, default=None, metavar="FILE", help="also write the table to FILE")
    ap.add_argument("--gpus", type=int, default=argparse.SUPPRESS, metavar="N",
                    help="score the files on N ranks, one per GPU from --gpu_device on (1 .. 8): rank r takes every N-th file from "
                         "the r-th on, rank 0 prints and writes the table, which is the single-process one value for value; not "
                         "with --copy-synthesis")
    # copy synthesis (wavenet_amd/metrics.py; copy_synthesis_dir below): present in the namespace only when given
    ap.add_argument("--copy-synthesis", action="store_true", default=argparse.SUPPRESS,
                    help="instead of scoring, resynthesise every file from its own features (a checkpoint trained with train "
                         "--local-mel; the fast decoder, all files in one batched run) and print how close the result is: the "
                         "log-spectral distance on the mel scale in dB, the F0 error in cents, gross F0 errors and the voiced / "
                         "unvoiced error, against the file itself")
    ap.add_argument("--seconds", type=float, default=argparse.SUPPRESS, metavar="S", help="--copy-synthesis: at most S seconds of every file")
    ap.add_argument("--seed", type=int, default=argparse.SUPPRESS, metavar="N", help="--copy-synthesis: numpy seed of the draws")
    ap.add_argument("--temperature", type=float, default=argparse.SUPPRESS, help="--copy-synthesis: as for generate")
    ap.add_argument("--top-k", type=int, default=argparse.SUPPRESS, help="--copy-synthesis: as for generate")
    ap.add_argument("--top-p", type=float, default=argparse.SUPPRESS, help="--copy-synthesis: as for generate")
    # folded resynthesis (FasterWaveNet.generate_folded; metrics.copy_synthesis(..., fold=)): present in the namespace only when given
    ap.add_argument("--fold", type=str, default=argparse.SUPPRESS, metavar="SECONDS|auto",
                    help="--copy-synthesis: resynthesise every file folded -- cut into overlapping segments of SECONDS (auto: sized to "
                         "fill one launch), all decoded side by side and cross-faded, as generate --fold does -- and print the same "
                         "figures: what folding costs on this checkpoint")
    ap.add_argument("--fold-overlap", type=float, default=argparse.SUPPRESS, metavar="SECONDS", help="--fold: as for generate")
    ap.add_argument("--fold-warmup", type=float, default=argparse.SUPPRESS, metavar="SECONDS", help="--fold: as for generate")
    return ap


COPY_FLAGS = ("seconds", "seed", "temperature", "top_k", "top_p", "fold", "fold_overlap", "fold_warmup")
COPY_KEYS = ("log_mel_distance_db", "f0_rmse_cents", "f0_gross_error", "vuv_error", "voiced_frames", "nats_per_sample")


def copy_synthesis_job(args):
    """``evaluate --copy-synthesis``: the checks, made before a model is built.  Returns None without the flag, else the keywords
    of ``copy_synthesis_dir`` that the command line gives."""
    given = [f for f in COPY_FLAGS if hasattr(args, f)]
    if not getattr(args, "copy_synthesis", False):
        if given:
            raise SystemExit("evaluate: {} go{} with --copy-synthesis".format(
                ", ".join("--" + f.replace("_", "-") for f in given), "es" if len(given) == 1 else ""))
        return None
    if _local.load_mel(args.model_dir) is None:
        raise SystemExit("evaluate: --copy-synthesis compares mel columns and needs the mel parameters of a checkpoint trained with "
                         "train --local-mel ({} has no \"mel\")".format(os.path.join(args.model_dir, _local.FILE)))
    kw = {f: getattr(args, f) for f in given if not f.startswith("fold")}
    if any(f.startswith("fold") for f in given):
        # generate's own checks and conversion to samples (a folded run is a --fast one)
        from . import generate as _generate
        probe = argparse.Namespace(fast=True, chunk_frames=None, keep=None, best_of=1, model_dir=args.model_dir,
                                   **{f: getattr(args, f) for f in given if f.startswith("fold")})
        try:
            kw["fold"] = _generate.fold_job(probe)
        except SystemExit as e:
            raise SystemExit(str(e).replace("generate:", "evaluate:", 1))
    if "seconds" in kw and not kw["seconds"] > 0:
        raise SystemExit("evaluate: --seconds S needs S > 0, got {}".format(kw["seconds"]))
    from .. import sampling
    try:
        sampling.check_controls(kw.get("temperature", 1.0), kw.get("top_k", 0), kw.get("top_p", 1.0))
    except ValueError as e:
        raise SystemExit("evaluate: {}".format(e))
    return kw


def copy_synthesis_dir(net, params, wav_dir, local_dir=None, seconds=None, seed=None, resample=False, verbose: bool = True,
                       forced: bool = False, fold=None, **controls):
    """Resynthesise every .wav file of ``wav_dir`` (sorted by name) from its own features and compare the result with the file:
    ``metrics.copy_synthesis`` over all files, one ``generate_batch`` run (``net``: a ``FasterWaveNet`` whose checkpoint has
    "mel" in local.json).  A file is read as training reads it (``resample``: at the model's rate) and cut to ``seconds``; its
    features are its feature file in ``local_dir`` or, without one, its log-mel columns made on the device; its speaker is the
    label its name carries.  ``seed``: numpy's, set once before the files' uniforms are drawn in order.  ``controls``:
    temperature, top_k, top_p.  A checkpoint with "pitch" in local.json: the network's features are ``acoustic.MelPitch``'s (mel
    rows, then pitch channels), while the figures keep comparing pure ``LogMel`` columns (the mel count) and ``Pitch`` rows of file
    and resynthesis.  ``forced``: every sample behind the window is given instead of drawn (the resynthesis is then the file and every
    distance 0: features and metrics sit on one grid).  ``fold``: None, or (body, overlap, warmup) in samples -- the resynthesis is
    ``generate_folded``'s (``metrics.copy_synthesis(..., fold=)``) and every row of the table gains "fold".  Returns ``{"files": [{"file", "samples", "log_mel_distance_db", "f0_rmse_cents",
    "f0_gross_error", "vuv_error", "voiced_frames", "nats_per_sample"}, ...], "total": {...}}`` -- the total weighted by what each
    figure was averaged over (``metrics.total``: compared columns, frames voiced in both, emitted samples) -- and prints one line
    per file and one for the total unless ``verbose`` is off."""
    import numpy as np
    import torch
    from .. import metrics
    from ..pitch import Pitch
    local, mel = getattr(net, "local", None), getattr(net, "local_mel", None)
    with_pitch = getattr(net, "local_pitch", None)
    settings = _local.analysis_settings(mel, with_pitch)
    mels = None if local is None else local[0] - (_local.PITCH_CHANNELS if with_pitch else 0)
    if local is None or mel is None:
        raise SystemExit("evaluate: --copy-synthesis needs a checkpoint trained with train --local-mel")
    files = sorted(fn for fn in os.listdir(wav_dir) if fn.endswith(".wav"))
    if not files:
        raise Exception("no .wav file in {}".format(wav_dir))
    Q, W = params.quantization_steps, int(net.input_width)
    labels = getattr(net, "speakers", None)
    cids = None if labels is None else [_speakers.class_id(labels, _speakers.speaker_label(fn), fn) for fn in files]
    tokens, feats, rates = [], [], []
    rkw = dict(rate=int(params.sampling_rate), device=net.device) if resample else {}
    with torch.cuda.device(net.device):
        for fn in files:
            t, rate = data.load_audio_file(os.path.join(wav_dir, fn), quantization_steps=Q, **rkw)
            t = np.asarray(t, dtype=np.int32)
            if seconds is not None:
                t = t[:int(rate * seconds)]
            if t.size < W + 2:
                raise SystemExit("evaluate: --copy-synthesis: {} holds {} samples{}; the window takes {} and the decoder runs two more "
                                 "at least".format(fn, t.size, "" if seconds is None else " within --seconds {}".format(seconds), W))
            tokens.append(t)
            rates.append(int(rate))
            feats.append(_local.with_extra_column(
                _local.file_or_mel_features(local_dir, settings, fn, t, rate, local[0], local[1], Q),
                getattr(net, "local_interp", "repeat"), getattr(net, "local_upsample", 1)))
        if len(set(rates)) > 1:
            raise SystemExit("evaluate: --copy-synthesis analyses all files on one column grid, and {} holds files at {} Hz: give "
                             "--resample".format(wav_dir, ", ".join(str(r) for r in sorted(set(rates)))))
        try:
            pitch = Pitch(rates[0], hop=local[1], win=mel["win"], device=net.device)
        except ValueError as e:
            raise SystemExit("evaluate: --copy-synthesis: {}".format(e))
        if seed is not None:
            np.random.seed(seed)
        uniforms = [np.random.random_sample(t.size - W) for t in tokens]
        fkw = {"forced": [t[W:] for t in tokens]} if forced else {}
        if fold is not None:
            fkw["fold"] = fold
        got = metrics.copy_synthesis(net, tokens, feats, cids, uniforms, _local.mel_analyser(rates[0], mels, local[1], mel["win"]),
                                     pitch, **fkw, **controls)
    table = {"files": [dict([("file", fn), ("samples", r["samples"])] + [(k, r[k]) for k in COPY_KEYS] +
                            ([("fold", r["fold"])] if "fold" in r else [])) for fn, r in zip(files, got)]}
    whole = metrics.total(got)
    table["total"] = dict([("samples", whole["samples"])] + [(k, whole[k]) for k in COPY_KEYS])
    if verbose:
        fmt = lambda v, spec: "-" if v is None else format(v, spec)
        for r in table["files"] + [dict(file="total", **table["total"])]:
            sys.stdout.write("{:<32} {:>10d} samples  {} dB log-mel  {} cents F0 ({} gross, {} voiced frames)  {} V/UV  {} nats/sample\n".format(
                r["file"], r["samples"], fmt(r["log_mel_distance_db"], ".4f"), fmt(r["f0_rmse_cents"], ".2f"),
                fmt(r["f0_gross_error"], ".4f"), r["voiced_frames"], fmt(r["vuv_error"], ".4f"), fmt(r["nats_per_sample"], ".6f")))
        sys.stdout.flush()
    return table


def table_of(rows):
    """``{"files": rows, "total": {...}}`` of scored rows, the total weighted by samples and summed in the rows' order."""
    nats, samples = 0.0, 0
    for row in rows:
        nats += row["nats_per_sample"] * row["samples"]
        samples += row["samples"]
    mean = nats / samples if samples else 0.0
    return {"files": rows, "total": {"samples": samples, "nats_per_sample": mean, "bits_per_sample": mean / math.log(2.0)}}


def merge_rows(rows_per_rank):
    """The rows that the ranks scored (rank r holds those of ``files[r::world]``, possibly none), back in sorted file order."""
    return sorted((row for rows in rows_per_rank for row in rows), key=lambda row: row["file"])


def evaluate_dir(net, params, wav_dir, chunk_width: int = 16384, batch_size: int = 8, verbose: bool = True, local_dir=None,
                 local_mel=None, resample=False, shard=None):
    """Score every .wav file of ``wav_dir`` (sorted by name).  Returns ``{"files": [{"file", "samples", "nats_per_sample",
    "bits_per_sample"}, ...], "total": {"samples", "nats_per_sample", "bits_per_sample"}}``, the total weighted by
    samples, and prints one line per file and one for the total unless ``verbose`` is off.  A checkpoint conditioned on
    speakers scores every file under the label its name carries (train_audio/speakers.py); an unknown label stops the run.
    A locally conditioned checkpoint scores every file under its feature file in ``local_dir`` (train_audio/local.py); the
    pieces of a launch share a phase, so ``chunk_width`` is rounded up to a multiple of the hop.  ``local_mel`` ({"win": W}, the
    checkpoint's "mel" entry; with its "pitch" entry inside, ``local.analysis_settings``, the pitch channels follow the mel rows):
    without ``local_dir``, every file is scored under the log-mel features of its own tokens.
    ``resample``: every file is read at the model's sampling_rate (``data.load_audio_file(..., rate=)``, on the network's device).
    ``shard`` = (rank, world), inside a process group of that size: this process scores ``files[rank::world]`` -- possibly no
    file --, the rows are exchanged (``all_gather_object``) and every rank returns the whole table.  A file's row does not depend
    on the other files and the total is summed in sorted order, so the table is the single-process one, value for value."""
    local = getattr(net, "local", None)
    _local.require_match(local, local_dir is not None or local_mel is not None, "evaluate", "--local-dir FEAT_DIR or --local-mel")
    if local is not None:
        chunk_width = -(-int(chunk_width) // local[1]) * local[1]
    files = sorted(fn for fn in os.listdir(wav_dir) if fn.endswith(".wav"))
    if not files:
        raise Exception("no .wav file in {}".format(wav_dir))
    rows = []
    labels = getattr(net, "speakers", None)
    cids = {fn: None if labels is None else _speakers.class_id(labels, _speakers.speaker_label(fn), fn) for fn in files}
    for fn in files if shard is None else files[int(shard[0])::int(shard[1])]:
        rkw = dict(rate=int(params.sampling_rate), device=net.device) if resample else {}
        tokens, rate = data.load_audio_file(os.path.join(wav_dir, fn), quantization_steps=params.quantization_steps, **rkw)
        lkw = {} if local is None else {"local": _local.with_extra_column(
            _local.file_or_mel_features(local_dir, local_mel, fn, tokens, rate, local[0], local[1], params.quantization_steps),
            getattr(net, "local_interp", "repeat"), getattr(net, "local_upsample", 1))}
        row = scoring.summarize(net.score(tokens, chunk_width=chunk_width, batch_size=batch_size, condition=cids[fn], **lkw))
        rows.append(dict(file=fn, **row))
    if shard is not None:
        import torch.distributed as dist
        per_rank = [None] * int(shard[1])
        dist.all_gather_object(per_rank, rows)
        rows = merge_rows(per_rank)
    table = table_of(rows)
    if verbose:
        for r in rows + [dict(file="total", **table["total"])]:
            sys.stdout.write("{:<32} {:>10d} samples  {:.6f} nats/sample  {:.6f} bits/sample\n".format(
                r["file"], r["samples"], r["nats_per_sample"], r["bits_per_sample"]))
        sys.stdout.flush()
    return table


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    copy = copy_synthesis_job(args)                          # before a model is built
    gpus = getattr(args, "gpus", 1)
    try:
        _launch.check_gpus(gpus)
    except ValueError as e:
        ap.error(str(e))
    if gpus > 1:
        # --gpus N: this process starts the N ranks of this very command line as a child (train_audio/launch.py) and hands their
        # exit code on; it builds no model and touches no device.  A rank finds WORLD_SIZE set and scores its files
        if copy is not None:
            raise SystemExit("evaluate: --gpus {} covers the likelihood table; --copy-synthesis runs on one device".format(gpus))
        if not _launch.in_rank():
            code = _launch.run("wavenet_amd.train_audio.evaluate", sys.argv[1:] if argv is None else list(argv), gpus)
            if code:
                raise SystemExit(code)
            return None
    args.fast, args.seed = copy is not None, None            # what train_audio.model.build reads beyond the shared flags
    if copy is not None:
        params, net = _model.build(args)
        table = copy_synthesis_dir(net, params, args.wav_dir, local_dir=getattr(args, "local_dir", None),
                                   resample=bool(getattr(args, "resample", False)), **copy)
        if args.json:
            with open(args.json, "w") as f:
                json.dump(table, f, indent=2)
        return table
    want_mel = bool(getattr(args, "local_mel", False))
    if want_mel and _local.load_mel(args.model_dir) is None:                 # before a model is built
        raise SystemExit("evaluate: --local-mel needs a checkpoint trained with train --local-mel ({} has no \"mel\")".format(
            os.path.join(args.model_dir, _local.FILE)))
    rank, world = _launch.join(args)                         # before a model is built; (0, 1) without --gpus
    with _launch.rank_stdout(rank):                          # rank 0 alone prints, and writes --json
        params, net = _launch.build_in_turn(lambda: _model.build(args), rank, world)
        skw = {} if world == 1 else {"shard": (rank, world)}
        table = evaluate_dir(net, params, args.wav_dir, chunk_width=args.chunk_width, batch_size=args.batch_size,
                             local_dir=getattr(args, "local_dir", None),
                             local_mel=_local.analysis_settings(net.local_mel, getattr(net, "local_pitch", None)) if want_mel else None,
                             resample=bool(getattr(args, "resample", False)), **skw)
        if args.json and rank == 0:
            with open(args.json, "w") as f:
                json.dump(table, f, indent=2)
    _launch.leave(world)                                     # a barrier precedes exit
    return table


if __name__ == "__main__":
    main()
