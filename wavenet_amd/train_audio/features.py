"""Write log-mel feature files for local conditioning: ``FEAT_DIR/NAME.npy`` per ``WAV_DIR/NAME.wav``.

    python -m wavenet_amd.train_audio.features -w WAV_DIR -o FEAT_DIR [--hop 256 --mels 80 --win 1024] [--device]

A file is read as training reads it (``data.load_audio_file``: mu-law tokens, silence trimmed) and the spectrogram is taken
of those tokens decoded back to a waveform, so column k belongs to tokens k * hop .. (k + 1) * hop - 1 of what the network
sees.  See wavenet_amd/features.py for the definition.  ``--device`` writes the same files from the kernel
(``features.LogMel.batch`` over the tokens, at most 64 files per launch): float32 sums in place of float64 ones.
``--resample -m MODEL_DIR`` (or ``--rate R``) reads every file at the model's sampling_rate, as ``train --resample`` does (on the
GPU with ``--device``, else by the numpy definition), and the filterbank is that rate's.
``--pitch [--f0-min 60 --f0-max 500 --f0-threshold 0.15]`` writes (F + 3, frames) files: three pitch channels -- voiced, log-F0,
aperiodicity -- behind the mel rows, from ``acoustic.MelPitch`` with ``--device`` (the values ``train --local-mel --local-pitch``
sees) and from ``acoustic.mel_pitch`` on the host without."""
from __future__ import annotations

import argparse
import os

import numpy as np

from .. import data, features
from .local import feature_path


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-w", "--wav-dir", type=str, default="wav", help="directory of .wav files")
    ap.add_argument("-o", "--output-dir", type=str, default="features", help="where NAME.npy goes")
    ap.add_argument("--hop", type=int, default=256, help="samples per feature column")
    ap.add_argument("--mels", type=int, default=80, help="mel channels F")
    ap.add_argument("--win", type=int, default=1024, help="analysis window in samples")
    ap.add_argument("--quantization-steps", type=int, default=256, help="the model's quantization_steps")
    ap.add_argument("--device", action="store_true",
                    help="compute on the GPU (features.LogMel): the values that train --local-mel and generate --from-wav see")
    ap.add_argument("--pitch", action="store_true", default=argparse.SUPPRESS,
                    help="three pitch channels behind the mel rows: voiced, log-F0 between --f0-min (0) and --f0-max (1), aperiodicity")
    ap.add_argument("--f0-min", type=float, default=argparse.SUPPRESS, help="--pitch: lowest F0 in Hz (60)")
    ap.add_argument("--f0-max", type=float, default=argparse.SUPPRESS, help="--pitch: highest F0 in Hz (500)")
    ap.add_argument("--f0-threshold", type=float, default=argparse.SUPPRESS, help="--pitch: YIN's voicing threshold (0.15)")
    ap.add_argument("--resample", action="store_true", default=argparse.SUPPRESS,
                    help="bring every file to the rate of -m MODEL_DIR's wavenet.json (or --rate R) before it is encoded")
    ap.add_argument("-m", "--model-dir", type=str, default=argparse.SUPPRESS, help="--resample: where wavenet.json lies")
    ap.add_argument("--rate", type=int, default=argparse.SUPPRESS, help="--resample: the rate itself")
    return ap


def target_rate(args):
    """None without --resample, else the rate it converts to: --rate R, or sampling_rate of -m MODEL_DIR's wavenet.json."""
    if not getattr(args, "resample", False):
        if hasattr(args, "rate") or hasattr(args, "model_dir"):
            raise SystemExit("features: --rate R and -m MODEL_DIR go with --resample")
        return None
    if hasattr(args, "rate"):
        if args.rate < 1:
            raise SystemExit("features: --rate R needs R >= 1, got {}".format(args.rate))
        return int(args.rate)
    if not hasattr(args, "model_dir"):
        raise SystemExit("features: --resample needs the rate to convert to: give -m MODEL_DIR or --rate R")
    from . import model as _model
    return int(_model.load_params(args.model_dir).sampling_rate)


def pitch_settings(args):
    """None without --pitch, else {"fmin", "fmax", "threshold"} of the command line; the three flags go with --pitch."""
    given = {k: getattr(args, f) for k, f in (("fmin", "f0_min"), ("fmax", "f0_max"), ("threshold", "f0_threshold")) if hasattr(args, f)}
    if not getattr(args, "pitch", False):
        if given:
            raise SystemExit("features: --f0-min, --f0-max and --f0-threshold go with --pitch")
        return None
    from .local import DEFAULT_PITCH
    return dict(DEFAULT_PITCH, **{k: float(v) for k, v in given.items()})


def device_features(paths, quantization_steps, mels, hop, win, rate=None, pitch=None):
    """[(tokens, (F, frames) float32 array)] of wav files, LogMel.batch over each run of files that share a sampling rate.
    ``rate``: every file is read at that rate (converted on the device).  ``pitch`` ({"fmin", "fmax", "threshold"}):
    ``acoustic.MelPitch.batch`` instead, (F + 3, frames) arrays."""
    if rate is None:
        loaded = [data.load_audio_file(p, quantization_steps=quantization_steps) for p in paths]
    else:
        loaded = [(t, rate) for t in data.load_audio_files(paths, rate, quantization_steps, "cuda")]
    feats = [None] * len(paths)
    for rate in sorted({r for _, r in loaded}):
        if pitch is None:
            mel = features.LogMel(rate, n_mels=mels, hop=hop, win=win)
        else:
            from .. import acoustic
            mel = acoustic.MelPitch(rate, n_mels=mels, hop=hop, win=win, fmin=pitch["fmin"], fmax=pitch["fmax"],
                                    threshold=pitch["threshold"])
        idx = [i for i, (_, r) in enumerate(loaded) if r == rate]
        for at in range(0, len(idx), features.LOGMEL_MAX_CLIPS):
            part = idx[at:at + features.LOGMEL_MAX_CLIPS]
            for i, out in zip(part, mel.batch([loaded[i][0] for i in part], quantization_steps)):
                feats[i] = out.cpu().numpy()
    return [(tok, f) for (tok, _), f in zip(loaded, feats)]


def main(argv=None):
    args = build_parser().parse_args(argv)
    to_rate = target_rate(args)
    pitch = pitch_settings(args)
    files = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
    if not files:
        raise SystemExit("no .wav file in {}".format(args.wav_dir))
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    if args.device:
        features._check_logmel_shape(args.mels, args.hop, args.win)      # before any file is read
        got = device_features([os.path.join(args.wav_dir, fn) for fn in files], args.quantization_steps, args.mels, args.hop,
                              args.win, to_rate, pitch)
        for fn, (tokens, feats) in zip(files, got):
            out = feature_path(args.output_dir, fn)
            np.save(out, feats)
            print("{}: {} samples -> {} {}".format(fn, tokens.size, out, feats.shape))
            written.append(out)
        return written
    for fn in files:
        tokens, rate = data.load_audio_file(os.path.join(args.wav_dir, fn), quantization_steps=args.quantization_steps,
                                            rate=to_rate)
        signal = data.mulaw_decode(tokens, args.quantization_steps)
        if pitch is None:
            feats = features.log_mel(signal, rate, n_mels=args.mels, hop=args.hop, win=args.win)
        else:
            from .. import acoustic
            feats = acoustic.mel_pitch(signal, rate, args.mels, args.hop, args.win, pitch["fmin"], pitch["fmax"],
                                       pitch["threshold"]).astype(np.float32)
        out = feature_path(args.output_dir, fn)
        np.save(out, feats)
        print("{}: {} samples -> {} {}".format(fn, tokens.size, out, feats.shape))
        written.append(out)
    return written


if __name__ == "__main__":
    main()
