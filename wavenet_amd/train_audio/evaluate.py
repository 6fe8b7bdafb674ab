"""Evaluation driver (new; the reference has none): the model's negative log-likelihood on every .wav file of a directory,
teacher-forced, in nats and bits per sample -- the held-out number that tells overfitting from learning.

    python -m wavenet_amd.train_audio.evaluate -w held_out_wav -m model [--ema] [--json scores.json]

Files are read as training reads them (mu-law tokens, silence trimmed) and scored by ``WaveNet.score``.  The command has
its own parser: it shares ``-g / -w / -m`` with train and generate and takes none of their other flags."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

from .. import data, scoring
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
    return ap


def evaluate_dir(net, params, wav_dir, chunk_width: int = 16384, batch_size: int = 8, verbose: bool = True, local_dir=None,
                 local_mel=None, resample=False):
    """Score every .wav file of ``wav_dir`` (sorted by name).  Returns ``{"files": [{"file", "samples", "nats_per_sample",
    "bits_per_sample"}, ...], "total": {"samples", "nats_per_sample", "bits_per_sample"}}``, the total weighted by
    samples, and prints one line per file and one for the total unless ``verbose`` is off.  A checkpoint conditioned on
    speakers scores every file under the label its name carries (train_audio/speakers.py); an unknown label stops the run.
    A locally conditioned checkpoint scores every file under its feature file in ``local_dir`` (train_audio/local.py); the
    pieces of a launch share a phase, so ``chunk_width`` is rounded up to a multiple of the hop.  ``local_mel`` ({"win": W}, the
    checkpoint's "mel" entry): without ``local_dir``, every file is scored under the log-mel features of its own tokens.
    ``resample``: every file is read at the model's sampling_rate (``data.load_audio_file(..., rate=)``, on the network's device)."""
    local = getattr(net, "local", None)
    _local.require_match(local, local_dir is not None or local_mel is not None, "evaluate", "--local-dir FEAT_DIR or --local-mel")
    if local is not None:
        chunk_width = -(-int(chunk_width) // local[1]) * local[1]
    files = sorted(fn for fn in os.listdir(wav_dir) if fn.endswith(".wav"))
    if not files:
        raise Exception("no .wav file in {}".format(wav_dir))
    rows, nats, samples = [], 0.0, 0
    labels = getattr(net, "speakers", None)
    cids = {fn: None if labels is None else _speakers.class_id(labels, _speakers.speaker_label(fn), fn) for fn in files}
    for fn in files:
        rkw = dict(rate=int(params.sampling_rate), device=net.device) if resample else {}
        tokens, rate = data.load_audio_file(os.path.join(wav_dir, fn), quantization_steps=params.quantization_steps, **rkw)
        lkw = {} if local is None else {"local": _local.with_extra_column(
            _local.file_or_mel_features(local_dir, local_mel, fn, tokens, rate, local[0], local[1], params.quantization_steps),
            getattr(net, "local_interp", "repeat"), getattr(net, "local_upsample", 1))}
        row = scoring.summarize(net.score(tokens, chunk_width=chunk_width, batch_size=batch_size, condition=cids[fn], **lkw))
        rows.append(dict(file=fn, **row))
        nats += row["nats_per_sample"] * row["samples"]
        samples += row["samples"]
    mean = nats / samples if samples else 0.0
    table = {"files": rows, "total": {"samples": samples, "nats_per_sample": mean,
                                      "bits_per_sample": mean / math.log(2.0)}}
    if verbose:
        for r in rows + [dict(file="total", **table["total"])]:
            sys.stdout.write("{:<32} {:>10d} samples  {:.6f} nats/sample  {:.6f} bits/sample\n".format(
                r["file"], r["samples"], r["nats_per_sample"], r["bits_per_sample"]))
        sys.stdout.flush()
    return table


def main(argv=None):
    args = build_parser().parse_args(argv)
    args.fast, args.seed = False, None                       # what train_audio.model.build reads beyond the shared flags
    want_mel = bool(getattr(args, "local_mel", False))
    if want_mel and _local.load_mel(args.model_dir) is None:                 # before a model is built
        raise SystemExit("evaluate: --local-mel needs a checkpoint trained with train --local-mel ({} has no \"mel\")".format(
            os.path.join(args.model_dir, _local.FILE)))
    params, net = _model.build(args)
    table = evaluate_dir(net, params, args.wav_dir, chunk_width=args.chunk_width, batch_size=args.batch_size,
                         local_dir=getattr(args, "local_dir", None), local_mel=net.local_mel if want_mel else None,
                         resample=bool(getattr(args, "resample", False)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(table, f, indent=2)
    return table


if __name__ == "__main__":
    main()
