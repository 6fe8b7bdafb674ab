"""Write log-mel feature files for local conditioning: ``FEAT_DIR/NAME.npy`` per ``WAV_DIR/NAME.wav``.

    python -m wavenet_amd.train_audio.features -w WAV_DIR -o FEAT_DIR [--hop 256 --mels 80 --win 1024]

A file is read as training reads it (``data.load_audio_file``: mu-law tokens, silence trimmed) and the spectrogram is taken
of those tokens decoded back to a waveform, so column k belongs to tokens k * hop .. (k + 1) * hop - 1 of what the network
sees.  See wavenet_amd/features.py for the definition."""
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
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    files = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
    if not files:
        raise SystemExit("no .wav file in {}".format(args.wav_dir))
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    for fn in files:
        tokens, rate = data.load_audio_file(os.path.join(args.wav_dir, fn), quantization_steps=args.quantization_steps)
        signal = data.mulaw_decode(tokens, args.quantization_steps)
        feats = features.log_mel(signal, rate, n_mels=args.mels, hop=args.hop, win=args.win)
        out = feature_path(args.output_dir, fn)
        np.save(out, feats)
        print("{}: {} samples -> {} {}".format(fn, tokens.size, out, feats.shape))
        written.append(out)
    return written


if __name__ == "__main__":
    main()
