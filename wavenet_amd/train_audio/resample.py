"""Write a directory of .wav files at another sampling rate: ``OUT_DIR/NAME.wav`` per ``WAV_DIR/NAME.wav``, mono, 16-bit PCM.

    python -m wavenet_amd.train_audio.resample -w WAV_DIR -o OUT_DIR --rate 16000 [--device]

The left channel of every file goes through ``wavenet_amd.resample`` and ``to_pcm16`` of the result is written: from the
kernel with ``--device`` (``Resampler.batch``, files grouped by their rate, at most 64 per launch), from the numpy definition
without.  A file already at the rate is written as its left channel, unchanged.  Only 16-bit PCM and float files are read.
Training on the written files is training on the originals with ``train --resample``, bit for bit, when ``--device`` is given:
both take the kernel's 16-bit values."""
from __future__ import annotations

import argparse
import os

import numpy as np

from .. import data, resample


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-w", "--wav-dir", type=str, default="wav", help="directory of .wav files")
    ap.add_argument("-o", "--output-dir", type=str, default="wav_resampled", help="where NAME.wav goes")
    ap.add_argument("--rate", type=int, required=True, help="the rate to convert to")
    ap.add_argument("--device", action="store_true", help="convert on the GPU (resample.Resampler): the values that --resample sees")
    return ap


def convert(paths, rate, device=None):
    """[(file's rate, its samples, int16 PCM at ``rate``)] of wav files, ``Resampler.batch`` over the files of one rate."""
    from scipy.io import wavfile
    read = []
    for p in paths:
        file_rate, signal = wavfile.read(p)
        read.append((int(file_rate), data._convertible(p, signal)))
    out = [None] * len(paths)
    for key in sorted({(r, x.dtype == np.int16) for r, x in read}):
        idx = [i for i, (r, x) in enumerate(read) if (r, x.dtype == np.int16) == key]
        rs = resample.resampler(key[0], rate, device)
        for at in range(0, len(idx), resample.RESAMPLE_MAX_CLIPS):
            part = idx[at:at + resample.RESAMPLE_MAX_CLIPS]
            for i, pcm in zip(part, rs.batch([read[i][1] for i in part], out="pcm16")):
                out[i] = np.asarray(pcm.cpu() if hasattr(pcm, "cpu") else pcm, dtype=np.int16)
    return [(r, x.size, pcm) for (r, x), pcm in zip(read, out)]


def main(argv=None):
    from scipy.io import wavfile
    args = build_parser().parse_args(argv)
    if args.rate < 1:
        raise SystemExit("resample: --rate R needs R >= 1, got {}".format(args.rate))
    files = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
    if not files:
        raise SystemExit("no .wav file in {}".format(args.wav_dir))
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    got = convert([os.path.join(args.wav_dir, fn) for fn in files], args.rate, "cuda" if args.device else None)
    for fn, (file_rate, n, pcm) in zip(files, got):
        out = os.path.join(args.output_dir, fn)
        wavfile.write(out, args.rate, pcm)
        print("{}: {} samples at {} Hz -> {} samples at {} Hz".format(fn, n, file_rate, pcm.size, args.rate))
        written.append(out)
    return written


if __name__ == "__main__":
    main()
