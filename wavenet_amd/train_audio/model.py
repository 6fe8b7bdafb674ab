"""``model/wavenet.json`` -> network (train_audio/model.py:8-58): read the hyper-parameter file if it is there, otherwise
write the reference's starting configuration, build WaveNet or FasterWaveNet, load the checkpoint, move to the device."""
from __future__ import annotations

import json
import os

import torch

from .. import FasterWaveNet, Params, WaveNet
from . import local as _local
from . import speakers as _speakers


def default_params() -> Params:
    """The configuration model.py:23-43 writes on the first run."""
    p = Params()
    p.quantization_steps = 256
    p.sampling_rate = 8000
    p.causal_conv_no_bias = True
    p.causal_conv_filter_width = 2
    p.causal_conv_channels = [256]
    p.residual_conv_dilation_no_bias = True
    p.residual_conv_projection_no_bias = True
    p.residual_conv_filter_width = 2
    p.residual_conv_channels = [128] * 8
    p.residual_num_blocks = 1
    p.softmax_conv_no_bias = False
    p.softmax_conv_channels = [256, 256]
    p.optimizer = "adam"
    p.momentum = 0.9
    p.weight_decay = 0
    p.gradient_clipping = 1.0
    return p


def load_params(model_dir: str) -> Params:
    os.makedirs(model_dir, exist_ok=True)
    filename = os.path.join(model_dir, "wavenet.json")
    if os.path.isfile(filename):
        print("loading", filename)
        try:
            with open(filename) as f:
                return Params(json.load(f))
        except Exception:
            raise Exception("could not load {}".format(filename))
    params = default_params()
    with open(filename, "w") as f:
        json.dump(params.to_dict(), f, indent=4)
    return params


def local_pitch_settings(args, params, hop=None, win=None, had=None):
    """``train --local-mel --local-pitch``: {"fmin", "fmax", "threshold"} from --f0-min / --f0-max / --f0-threshold, else from the
    checkpoint's local.json, else the defaults -- after ``pitch.pitch_lags`` and ``pitch.Pitch``'s device refusal were tried with
    the model's rate and the run's hop and window; a refusal stops the command.  None without --local-pitch.  ``hop``, ``win``,
    ``had``: what ``build`` has resolved already; a caller without them (the driver, before a model is built) gets them resolved
    the same way."""
    if not bool(getattr(args, "local_pitch", False)):
        return None
    have = _local.load_config(args.model_dir)
    if hop is None:
        hop = getattr(args, "local_hop", None) or (have[1] if have else _local.DEFAULT_HOP)
    if win is None:
        was = _local.load_mel(args.model_dir) if have else None
        win = getattr(args, "win", None) or (was["win"] if was else _local.DEFAULT_WIN)
    if had is None:
        had = _local.load_pitch(args.model_dir) if have else None
    given = {"fmin": getattr(args, "f0_min", None), "fmax": getattr(args, "f0_max", None),
             "threshold": getattr(args, "f0_threshold", None)}
    pitch = {k: float(given[k] if given[k] is not None else (had or _local.DEFAULT_PITCH)[k]) for k in _local.PITCH_KEYS}
    try:
        _local.check_pitch(params.sampling_rate, hop, win, pitch)
    except ValueError as e:
        raise SystemExit("--local-pitch: {}".format(e))
    return pitch


def build(args, train: bool = False):
    """-> (params, wavenet) on ``cuda:<args.gpu_device>``.  There is no CPU mode (``-g -1`` in the reference): the product
    path is the HIP library and fails loudly without a device.

    ``args.ema_decay`` > 0 (train) keeps a weight average, resumed from the checkpoint's ``wavenet.ema.npz`` when it is there;
    ``args.ema`` (generate, evaluate) loads that file's averaged weights as the model's weights.  Both are read with a
    default, so that a caller with a parser of its own need not know them.

    Speakers: ``args.speaker_prefix`` (train) takes the label table from the .wav files of ``args.wav_dir`` and writes it, with
    ``args.condition_channels``, to ``speakers.json`` -- or checks it against the one already there.  Whenever that file
    exists the network is built globally conditioned on its labels, and ``net.speakers`` is the table (None otherwise).

    Features: ``args.local_dir`` with ``train`` (the training driver) reads the channel count F from the feature file of the first .wav file and writes it,
    with the hop, to ``local.json`` -- or checks both against the one already there.  Whenever that file exists the network
    is built locally conditioned, and ``net.local`` is (F, hop) (None otherwise); ``args.local_interp`` (train) goes into the
    file the same way and ``net.local_interp`` is the file's mode; so does ``args.local_upsample`` (``"upsample"``, written
    for U > 1 only), and ``net.local_upsample`` is the file's factor.  ``args.local_mel`` (train) takes F, the hop and the
    window from --mels / --local-hop / --win instead of a feature file and adds ``"mel": {"win": W}``; ``net.local_mel`` is that
    entry of the file (None without it).  ``args.local_pitch`` (train, with ``args.local_mel``) adds 3 pitch channels behind the
    mel rows: ``"pitch": {"fmin", "fmax", "threshold"}`` from --f0-min / --f0-max / --f0-threshold, ``"channels"`` = mels + 3, after
    ``pitch.Pitch``'s refusals were tried at the model's rate; ``net.local_pitch`` is that entry of the file (None without it)."""
    params = load_params(args.model_dir)
    local_dir = getattr(args, "local_dir", None)
    if local_dir is not None and train:                                     # (evaluate and generate read the config only)
        wavs = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
        have = _local.load_config(args.model_dir)
        hop = getattr(args, "local_hop", None) or (have[1] if have else _local.DEFAULT_HOP)
        local = _local.ensure_config(args.model_dir, _local.directory_channels(local_dir, wavs), hop,
                                     getattr(args, "local_interp", None), getattr(args, "local_upsample", None))
    elif bool(getattr(args, "local_mel", False)) and train:                  # the features are made from the audio: F is a flag
        have = _local.load_config(args.model_dir)
        hop = getattr(args, "local_hop", None) or (have[1] if have else _local.DEFAULT_HOP)
        was = _local.load_mel(args.model_dir) if have else None
        win = getattr(args, "win", None) or (was["win"] if was else _local.DEFAULT_WIN)
        had = _local.load_pitch(args.model_dir) if have else None
        mels = getattr(args, "mels", None) or (_local.mel_count(args.model_dir) if have else _local.DEFAULT_MELS)
        from .. import features
        try:
            features._check_logmel_shape(mels, hop, win)
        except ValueError as e:
            raise SystemExit("--local-mel: {}".format(e))
        pitch = local_pitch_settings(args, params, hop, win, had)           # three pitch channels behind the mel rows, or None
        local = _local.ensure_config(args.model_dir, mels + (_local.PITCH_CHANNELS if pitch else 0), hop,
                                     getattr(args, "local_interp", None), getattr(args, "local_upsample", None), mel={"win": win},
                                     pitch=pitch)
    else:
        local = _local.load_config(args.model_dir)
    if bool(getattr(args, "speaker_prefix", False)):
        wavs = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
        table = _speakers.ensure_table(args.model_dir, _speakers.label_table(wavs), getattr(args, "condition_channels", None))
    else:
        table = _speakers.load_table(args.model_dir)
    cond = dict(condition_classes=len(table[0]), condition_channels=table[1]) if table else {}
    if local:
        cond.update(local_channels=local[0], local_hop=local[1], local_interp=_local.load_interp(args.model_dir))
        if _local.load_upsample(args.model_dir) > 1:                            # a learned upsampling layer ahead of the projection
            cond.update(local_upsample=_local.load_upsample(args.model_dir))
    net = (FasterWaveNet if args.fast else WaveNet)(params, seed=args.seed, **cond)
    net.speakers = table[0] if table else None
    net.local = local
    net.local_mel = _local.load_mel(args.model_dir) if local else None
    net.local_pitch = _local.load_pitch(args.model_dir) if local else None
    params.dump()
    ema_decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
    use_ema = bool(getattr(args, "ema", False))
    if use_ema and ema_decay > 0:
        raise Exception("--ema loads the averaged weights as the model's weights; it does not go with --ema-decay")
    if ema_decay > 0:
        net.enable_ema(ema_decay)
    if use_ema:
        try:
            net.load(args.model_dir, weights="ema")
        except FileNotFoundError as e:
            raise SystemExit("--ema: {}".format(e))
    else:
        net.load(args.model_dir)
    if ema_decay > 0:
        net.enable_ema(ema_decay)                  # the command line wins over the decay the checkpoint was written with
    if args.gpu_device < 0:
        raise Exception("--gpu_device -1 (CPU) is not supported: this engine runs on a HIP device only")
    torch.cuda.set_device(args.gpu_device)
    net.to_gpu(args.gpu_device)
    net.set_storage(getattr(args, "storage", "fp32"))      # --storage: how the model runs, nothing of it is in the checkpoint
    return params, net
