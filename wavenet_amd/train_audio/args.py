"""Command-line flags of the reference's train_audio scripts (train_audio/args.py:5-18: same spellings and defaults),
plus the loop sizes train.py:112-114 / 124 hard-codes, so that a short run does not need an edit."""
from __future__ import annotations

import argparse

from . import launch

# (flags, type, default, help); a bool default makes a store_true switch
_REFERENCE_FLAGS = (
    (("-g", "--gpu_device"), int, 0, "HIP device index"),
    (("-w", "--wav-dir"), str, "wav", "directory of .wav files to train on"),
    (("-m", "--model-dir"), str, "model", "wavenet.json + checkpoints"),
    (("-o", "--output_dir"), str, "generated_audio", "where generate writes generated.wav"),
    (("-s", "--seconds"), float, 1.0, "length of the generated audio"),
    (("--lr",), float, 0.001, "learning_rate"),
    (("--fast",), None, False, "FasterWaveNet: queue-cached generation"),
    (("--seed",), int, None, "numpy seed (crops, sampling)"),
)
_LOOP_FLAGS = (
    (("--batch-size",), int, 16, "train.py:112"),
    (("--train-width",), int, 500, "train.py:113"),
    (("--max-epoch",), int, 2000, "train.py:114 (epochs run 1 .. max_epoch - 1)"),
    (("--repeat",), int, 500, "updates per file per epoch (train.py:124)"),
    (("--no-graph",), None, False, "launch every update op by op instead of replaying a HIP graph"),
)
# sampling controls of generate (wavenet_amd/sampling.py; the reference draws from the raw softmax, generate.py:39): all off
_SAMPLING_FLAGS = (
    (("--temperature",), float, 1.0, "divide the logits by this before the softmax (1 = off)"),
    (("--top-k",), int, 0, "draw from the k most probable values only (0 = off)"),
    (("--top-p",), float, 1.0, "draw from the smallest set of most probable values holding this share of the mass (1 = off)"),
)
# batched generation (FasterWaveNet.generate_batch; the reference writes one utterance from silence): both off
_BATCH_FLAGS = (
    (("--utterances",), int, None, "write this many utterances, generated_000.wav ... (with --fast: one batched run)"),
)
# the exponential moving average of the weights (WaveNet.enable_ema; the reference trains and generates from the raw
# iterates): all off.  A command line without them parses to what it parsed to before they existed: they are attributes of
# the namespace only when given, and read as their defaults (the class attributes of ``Args``) when not.
_EMA_FLAGS = (
    (("--ema-decay",), float, 0.0, "train: keep an exponential moving average of the weights with this decay, saved as "
                                   "wavenet.ema.npz (0 = off; 0.999 - 0.9999 is usual)"),
    (("--valid-wav-dir",), str, None, "train: after every epoch, print the negative log-likelihood of this directory's .wav "
                                      "files (and, with --ema-decay, that of the averaged weights)"),
    (("--ema",), None, False, "generate: use the checkpoint's averaged weights (wavenet.ema.npz)"),
)
# global conditioning on a speaker label (WaveNet(..., condition_classes, condition_channels); train_audio/speakers.py): all
# off, and -- like the flags above -- attributes of the namespace only when given
_SPEAKER_FLAGS = (
    (("--speaker-prefix",), None, False, "train: condition on the speaker, a file's base name up to the first '_' "
                                         "(p225_001.wav -> p225); the label table goes to <model-dir>/speakers.json"),
    (("--condition-channels",), int, None, "train --speaker-prefix: width H of the learned speaker embedding"),
)
# local conditioning on feature files (WaveNet(..., local_channels, local_hop); train_audio/local.py): off, and attributes of
# the namespace only when given
_LOCAL_FLAGS = (
    (("--local-dir",), str, None, "train: condition on the feature file <local-dir>/NAME.npy of every NAME.wav, a float (F, frames) "
                                  "array with one column per --local-hop samples (python -m wavenet_amd.train_audio.features "
                                  "writes log-mel ones); F and the hop go to <model-dir>/local.json.  generate --fast: vocode "
                                  "every NAME.npy of the directory into <output_dir>/NAME.wav, each at the length its features "
                                  "cover (-s caps them), in one batched run; excludes --local"),
    (("--local-hop",), int, None, "train --local-dir / --local-mel: samples per feature column (256 unless local.json says otherwise)"),
    (("--local-interp",), str, None, "train --local-dir / --local-mel: how the features reach the sample rate, 'repeat' (a column holds for "
                                     "its hop samples) or 'linear' (interpolated between neighbouring columns, a column anchored "
                                     "at the first sample of its frame); stored in local.json, which generate and evaluate follow"),
    (("--local-crop",), str, None, "train --local-dir / --local-mel: where crops start, 'frame' (on a feature column border, the default) or "
                                   "'sample' (anywhere, as without features: one --seed selects the same crops; every crop "
                                   "carries its own phase).  A property of the run, not of the checkpoint"),
    (("--local-upsample",), int, None, "train --local-dir / --local-mel: a learned upsampling layer of factor U ahead of the projection (U "
                                       "divides the hop; the network then runs at hop / U); stored in local.json when U > 1, "
                                       "which generate and evaluate follow"),
)
# log-mel features made from the audio on the device (features.LogMel; train_audio/local.py "mel"): off, attributes of the
# namespace only when given
_MEL_FLAGS = (
    (("--local-mel",), None, False, "train: condition on the log-mel spectrogram of every .wav file itself, made on the device when "
                                    "the file is loaded (--mels F channels, one column per --local-hop samples, a window of --win); "
                                    "F, the hop and the window go to <model-dir>/local.json.  Excludes --local-dir"),
    (("--mels",), int, None, "train --local-mel: mel channels F (80 unless local.json says otherwise)"),
    (("--win",), int, None, "train --local-mel: analysis window in samples (1024 unless local.json says otherwise)"),
)
# pitch channels behind the mel rows (acoustic.MelPitch; train_audio/local.py "pitch"): off, attributes of the namespace only
# when given
_PITCH_FLAGS = (
    (("--local-pitch",), None, False, "train --local-mel: add three pitch channels behind the mel rows -- voiced, log-F0 between --f0-min "
                                      "(0) and --f0-max (1), aperiodicity -- tracked on the device from the same audio "
                                      "(pitch.Pitch); the three settings go to <model-dir>/local.json, whose channels are then "
                                      "--mels + 3, and evaluate and generate follow it"),
    (("--f0-min",), float, None, "train --local-pitch: lowest F0 in Hz (60 unless local.json says otherwise)"),
    (("--f0-max",), float, None, "train --local-pitch: highest F0 in Hz (500 unless local.json says otherwise)"),
    (("--f0-threshold",), float, None, "train --local-pitch: YIN's voicing threshold (0.15 unless local.json says otherwise)"),
    (("--f0-scale",), float, 1.0, "generate, on a checkpoint trained with --local-pitch: multiply the pitch of every voiced column of "
                                  "the features by S before the network sees them (--from-wav, --local, --local-dir; streamed "
                                  "chunks included); excludes --rank mel and --keep"),
)
# activation storage of the run (WaveNet.set_storage): fp32, and an attribute of the namespace only when given
_STORAGE_FLAGS = (
    (("--storage",), str, "fp32", "train, evaluate: activation storage, 'fp32' or 'bf16' (bfloat16 activations with fp32 accumulation "
                                  "on the 128-channel kernels; conditioned models included).  A property of the run, not of the "
                                  "checkpoint: weights, optimiser state and checkpoints are fp32 either way"),
)
# crops drawn across the whole corpus (wavenet_amd/corpus.py; train_audio/train.py train_corpus): off, an attribute of the
# namespace only when given, checked by train before the model is built
_CORPUS_FLAGS = (
    (("--corpus",), None, False, "train: keep every .wav file of --wav-dir on the device and draw each batch uniformly over all "
                                 "training windows of all files -- a batch then mixes files and speakers, each crop with its own "
                                 "file's speaker, features and phase, gathered in one launch -- instead of --repeat updates on "
                                 "one file after the other.  An epoch stays files x --repeat updates, with a checkpoint every "
                                 "--repeat.  A property of the run, not of the checkpoint"),
)
# files at any rate (wavenet_amd/resample.py; data.load_audio_file(..., rate=)): off, an attribute of the namespace only when given
_RESAMPLE_FLAGS = (
    (("--resample",), None, False, "train, generate: bring every .wav file that is read (the training files, --valid-wav-dir, "
                                   "--prompt, --keep, --from-wav) to the model's sampling_rate on the device before it is "
                                   "encoded, and make --local-mel features at that rate; a file already at that rate is read as "
                                   "without the flag.  Without it a file's samples are taken as they are, whatever its rate.  "
                                   "A property of the run, not of the checkpoint"),
)
# data parallelism over the GPUs of the node (wavenet_amd/dp.py; train_audio/launch.py): off, an attribute of the namespace only
# when given, checked by parse (the range) and by train (the batch) before anything is launched
_GPUS_FLAGS = (
    (("--gpus",), int, 1, "train: N ranks, one per GPU from --gpu_device on, each training its equal share of every batch, with one "
                          "all-reduce of the gradients per update; 1 .. 8.  --batch-size stays the GLOBAL batch and must divide "
                          "by N, so the flag changes the speed, not the optimisation problem; rank 0 prints and writes the "
                          "checkpoints.  A property of the run, not of the checkpoint"),
)
# likelihood of what was generated (FasterWaveNet.generate(..., return_chosen=True); sampling.chosen_nll / pick_best): off, and
# attributes of the namespace only when given.  generate checks them (both need --fast) before the model is built
_LIKELIHOOD_FLAGS = (
    (("--report",), str, None, "generate --fast: write FILE.json with the negative log-likelihood the model gave every written "
                               ".wav -- samples, nats and bits per emitted sample (prompt and window excluded) -- and the total "
                               "weighted by samples, as evaluate --json does for held-out audio"),
    (("--best-of",), int, 1, "generate --fast: draw every utterance K times, all candidates in the same batched run, and write "
                             "the one the model found most likely (lowest nats per sample).  Likelihood rewards quiet, "
                             "predictable audio: a ranking tool, most useful when vocoding from features, not a quality score.  "
                             "With --keep the figure covers the kept samples too: a candidate is judged by how the real audio "
                             "continues from what was drawn into it"),
)
# what --best-of ranks on (wavenet_amd/metrics.py; train_audio/generate.py rank_job / MelRank): likelihood, an attribute of the
# namespace only when given, checked by generate before the model is built
_RANK_FLAGS = (
    (("--rank",), str, "likelihood", "generate --fast --from-wav FILE.wav --best-of K: what the K candidates are ranked on, 'likelihood' "
                                     "(lowest nats per sample) or 'mel' (the smallest log-spectral distance on the mel scale to the "
                                     "recording's own columns, the candidates analysed on the device in one batch; --report then "
                                     "carries each kept file's log_mel_distance_db).  'mel' goes with --from-wav only, not with "
                                     "--chunk-frames"),
)
# streaming synthesis (FasterWaveNet.open_stream; train_audio/generate.py stream_job / generate_streamed): off, attributes of the
# namespace only when given, checked by generate before the model is built
_STREAM_FLAGS = (
    (("--chunk-frames",), int, None, "generate --fast --local FILE.npy: vocode as a stream -- hand the decoder C feature columns at a "
                                     "time, draw what they allow and append it to generated.wav as it goes; prints the time to the "
                                     "first written chunk.  With C >= the file's columns the output is byte for byte that of the "
                                     "command without the flag (with --best-of K > 1 the file is written at the end, when the "
                                     "ranking is known).  One utterance, from silence: excludes --utterances, --prompt, --keep and "
                                     "--local-dir"),
    (("--ring-frames",), int, None, "generate --chunk-frames: rows of the ring of projected feature rows the decoder reads in place "
                                    "(default: what one chunk and the largest pull need)"),
)
# decoding in utterance tiles (FasterWaveNet.batch_tile; train_audio/generate.py tile_job): off, an attribute of the namespace only
# when given, checked by generate before the model is built
_TILE_FLAGS = (
    (("--tile",), str, None, "generate --fast: decode the utterances of a batched run in tiles of U that share one read of the "
                             "weights -- auto, 2, 4, 8 or 16 (models of any shape but the specialised 32/256-channel one, which "
                             "ignores it); the samples are the same, bit for bit"),
)
# folded decoding (FasterWaveNet.generate_folded, wavenet_amd/fold.py; train_audio/generate.py fold_job): off, attributes of the
# namespace only when given, checked by generate before the model is built
_FOLD_FLAGS = (
    (("--fold",), str, None, "generate --fast, on a locally conditioned checkpoint (--local, --local-dir, --from-wav): decode every "
                             "utterance as overlapping segments of this many SECONDS side by side in one batched run and cross-fade "
                             "them where they meet; auto sizes the segments to fill one launch.  The uniforms are those of the "
                             "command without the flag, keyed by position: with SECONDS at least the utterance's length the file "
                             "is the same, byte for byte.  --report gains \"fold\" per file.  Excludes --chunk-frames, --keep, "
                             "--best-of and --rank.  evaluate --copy-synthesis: resynthesise folded"),
    (("--fold-overlap",), float, None, "generate / evaluate --fold: SECONDS of every seam, decoded by both neighbours and "
                                       "cross-faded (default: one feature column; at most --fold's)"),
    (("--fold-warmup",), float, None, "generate / evaluate --fold: SECONDS a segment decodes from a silent window ahead of its "
                                      "body and throws away (default: input_width samples)"),
)
# regenerating stretches of a recording (FasterWaveNet.generate(..., forced=...); train_audio/generate.py keep_job / keep_mask): off,
# attributes of the namespace only when given, checked by generate before the model is built
_KEEP_HELP = ("generate --fast: keep this recording and draw only the --redraw stretches: the file's first input_width samples are "
              "the window, every later sample is emitted as the file has it unless a --redraw range covers it, and the output is "
              "the file with those ranges regenerated.  Without --redraw everything is kept: with --report the run is the "
              "decoder's own likelihood of the file.  Repeatable: one file for all utterances, or one per utterance; excludes "
              "--prompt, -s and --local-dir")
_REDRAW_HELP = ("generate --keep: a stretch A:B, in seconds of the kept file, to draw instead of keeping; repeatable, applies to "
                "every utterance; it cannot start inside the window (the first input_width samples)")
_LOCAL_HELP = ("generate: the (F, frames) .npy features to generate from (a locally conditioned checkpoint needs them); repeatable: "
               "one file for all utterances, or one per utterance.  Without -s the length is what the features cover")
_FROM_WAV_HELP = ("generate --fast: copy synthesis -- read this recording as training reads it, make its log-mel features on the "
                  "device with the checkpoint's \"mel\" settings (a train --local-mel checkpoint) and generate as --local would from "
                  "those columns; with --chunk-frames C the analyser is fed C hops of audio at a time.  Repeatable: one file for all "
                  "utterances, or one per utterance; excludes --local, --local-dir and --keep")
_SPEAKER_HELP = ("generate: the speaker label to generate as (a conditioned checkpoint needs one); repeatable: one label for all "
                 "utterances, or one per utterance")
_PROMPT_HELP = ("a .wav file whose last input_width samples seed the generation instead of silence; repeatable: one file for "
                "all utterances, or one per utterance")


class Args(argparse.Namespace):
    """What :func:`parse` returns: the defaults of ``_EMA_FLAGS`` live here, not in the instance."""
    ema_decay, valid_wav_dir, ema = 0.0, None, False
    speaker_prefix, condition_channels, speaker = False, None, None
    local_dir, local_hop, local, local_interp, local_crop = None, None, None, None, None
    local_upsample = None
    local_mel, mels, win, from_wav = False, None, None, None
    local_pitch, f0_min, f0_max, f0_threshold, f0_scale = False, None, None, None, 1.0
    storage = "fp32"
    corpus = False
    resample = False
    gpus = 1
    report, best_of = None, 1
    rank = "likelihood"
    keep, redraw = None, None
    chunk_frames, ring_frames = None, None
    tile = None
    fold, fold_overlap, fold_warmup = None, None, None


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__)
    for flags, typ, default, text in _REFERENCE_FLAGS + _LOOP_FLAGS + _SAMPLING_FLAGS + _BATCH_FLAGS:
        if typ is None:
            ap.add_argument(*flags, action="store_true", default=default, help=text)
        else:
            ap.add_argument(*flags, type=typ, default=default, help=text)
    for flags, typ, default, text in _EMA_FLAGS + _SPEAKER_FLAGS + _LOCAL_FLAGS + _MEL_FLAGS + _PITCH_FLAGS + _STORAGE_FLAGS + _CORPUS_FLAGS + _RESAMPLE_FLAGS + _GPUS_FLAGS + _LIKELIHOOD_FLAGS + _RANK_FLAGS + _STREAM_FLAGS + _TILE_FLAGS + _FOLD_FLAGS:
        assert getattr(Args, flags[0].lstrip("-").replace("-", "_")) == default
        if typ is None:
            ap.add_argument(*flags, action="store_true", default=argparse.SUPPRESS, help=text)
        else:
            ap.add_argument(*flags, type=typ, default=argparse.SUPPRESS, help=text + " (default: %r)" % (default,))
    ap.add_argument("--prompt", action="append", default=None, metavar="FILE.wav", help=_PROMPT_HELP)
    ap.add_argument("--speaker", action="append", default=argparse.SUPPRESS, metavar="LABEL", help=_SPEAKER_HELP)
    ap.add_argument("--local", action="append", default=argparse.SUPPRESS, metavar="FILE.npy", help=_LOCAL_HELP)
    ap.add_argument("--keep", action="append", default=argparse.SUPPRESS, metavar="FILE.wav", help=_KEEP_HELP)
    ap.add_argument("--from-wav", action="append", default=argparse.SUPPRESS, metavar="FILE.wav", help=_FROM_WAV_HELP)
    ap.add_argument("--redraw", action="append", default=argparse.SUPPRESS, metavar="A:B", help=_REDRAW_HELP)
    return ap


def utterance_prompts(args):
    """(number of utterances, prompt file of each utterance or None for silence) of a parsed command line, or (None, None)
    when neither --utterances nor --prompt was given: the reference's single ``generated.wav`` from silence."""
    if args.utterances is None and not args.prompt:
        return None, None
    files = list(args.prompt or [])
    n = args.utterances if args.utterances is not None else max(1, len(files))
    if n < 1:
        raise ValueError("--utterances must be at least 1, got %d" % n)
    if len(files) not in (0, 1, n):
        raise ValueError("%d --prompt files for %d utterances: give one for all of them, or one each" % (len(files), n))
    return n, (files * n if len(files) == 1 else files or [None] * n)


def kept_files(args):
    """(number of utterances, kept file of each utterance) of a command line with --keep, or (None, None) without."""
    if not args.keep:
        return None, None
    files = list(args.keep)
    n = args.utterances if args.utterances is not None else len(files)
    if n < 1:
        raise ValueError("--utterances must be at least 1, got %d" % n)
    if len(files) not in (1, n):
        raise ValueError("%d --keep files for %d utterances: give one for all of them, or one each" % (len(files), n))
    return n, (files * n if len(files) == 1 else files)


def utterance_count(args):
    """The utterances a command line asks for: --keep's, else --utterances / --prompt's, else one."""
    return kept_files(args)[0] or utterance_prompts(args)[0] or 1


def parse(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv, namespace=Args())
    try:
        utterance_prompts(args)
        kept_files(args)
    except ValueError as e:
        ap.error(str(e))
    if not (0.0 <= args.ema_decay < 1.0):
        ap.error("--ema-decay must lie in [0, 1), got %r" % (args.ema_decay,))
    if args.speaker_prefix and (args.condition_channels is None or args.condition_channels < 1):
        ap.error("--speaker-prefix needs --condition-channels H with H >= 1")
    if args.condition_channels is not None and not args.speaker_prefix:
        ap.error("--condition-channels goes with --speaker-prefix")
    has_local = args.local_dir is not None or args.local_mel
    if args.local_mel and args.local_dir is not None:
        ap.error("--local-mel (features made from the audio) and --local-dir FEAT_DIR (feature files) exclude each other")
    if (args.mels is not None or args.win is not None) and not args.local_mel:
        ap.error("--mels F and --win W go with --local-mel")
    if args.local_mel:
        from .. import features
        try:
            features._check_logmel_shape(args.mels, args.local_hop, args.win)      # what is given; model.build checks what is used
        except ValueError as e:
            ap.error("--local-mel: %s" % e)
    if args.local_pitch and (not args.local_mel or args.local_dir is not None):
        ap.error("--local-pitch (pitch channels made from the audio) goes with --local-mel, not with --local-dir FEAT_DIR")
    if (args.f0_min is not None or args.f0_max is not None or args.f0_threshold is not None) and not args.local_pitch:
        ap.error("--f0-min, --f0-max and --f0-threshold go with --local-pitch")
    if args.from_wav:
        bad = [f for f, on in (("--local", args.local), ("--local-dir", args.local_dir is not None), ("--keep", args.keep)) if on]
        if bad:
            ap.error("--from-wav FILE.wav (features made from a recording) excludes %s" % ", ".join(bad))
        if not args.fast:
            ap.error("--from-wav needs --fast")
        n = utterance_count(args)
        if len(args.from_wav) not in (1, n):
            ap.error("%d --from-wav files for %d utterances: give one for all of them, or one each" % (len(args.from_wav), n))
    if args.local_hop is not None and (not has_local or args.local_hop < 1):
        ap.error("--local-hop H goes with --local-dir or --local-mel and needs H >= 1")
    if args.local_interp is not None and (not has_local or args.local_interp not in ("repeat", "linear")):
        ap.error("--local-interp {repeat,linear} goes with --local-dir or --local-mel")
    if args.local_crop is not None and (not has_local or args.local_crop not in ("frame", "sample")):
        ap.error("--local-crop {frame,sample} goes with --local-dir or --local-mel")
    if args.local_upsample is not None and (not has_local or args.local_upsample < 1):
        ap.error("--local-upsample U goes with --local-dir or --local-mel and needs U >= 1")
    if args.storage not in ("fp32", "bf16"):
        ap.error("--storage {fp32,bf16}, got %r" % (args.storage,))
    try:
        launch.check_gpus(args.gpus)
    except ValueError as e:
        ap.error(str(e))
    if args.local and args.local_dir is not None:
        ap.error("--local-dir FEAT_DIR (every feature file of a directory) and --local FILE.npy exclude each other")
    if args.local:
        n = utterance_count(args)
        if len(args.local) not in (1, n):
            ap.error("%d --local files for %d utterances: give one for all of them, or one each" % (len(args.local), n))
    if args.speaker:
        from .speakers import utterance_speakers
        try:
            utterance_speakers(args.speaker, utterance_count(args))
        except ValueError as e:
            ap.error(str(e))
    return args
