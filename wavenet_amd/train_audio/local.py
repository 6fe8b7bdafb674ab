"""Local conditioning on the command line: feature files next to the .wav files, and ``model/local.json``.

A feature file is ``FEAT_DIR/NAME.npy`` for ``WAV_DIR/NAME.wav``: a float (F, frames) array with one column per ``hop``
samples OF THE TOKENS AS TRAINING READS THEM (``data.load_audio_file``: mu-law, silence trimmed) -- column k belongs to
tokens k * hop .. (k + 1) * hop - 1.  ``python -m wavenet_amd.train_audio.features`` writes log-mel files of that kind.

``local.json`` holds ``{"channels": F, "hop": H}``: whenever it exists the network is built locally conditioned
(``wavenet.json`` is unchanged), and a resumed run must find the same values.  ``train --local-interp linear`` adds
``"interp": "linear"`` -- the key is written ONLY then, so a repeat-mode file is byte for byte what it always was; a file
without it means "repeat" (``load_interp``).  ``train --local-upsample U`` adds ``"upsample": U`` the same way, ONLY for U > 1
(``load_upsample``): the network is then built with a learned upsampling layer of that factor ahead of the projection.
``train --local-mel`` adds ``"mel": {"win": W}``, again ONLY with that flag (``load_mel``): the features are then the log-mel
spectrogram of the audio itself, made on the device (``features.LogMel``: F channels, the hop, that window), and evaluate
and generate can make them from a .wav file with no feature file at all.
``train --local-mel --local-pitch`` adds ``"pitch": {"fmin": .., "fmax": .., "threshold": ..}``, ONLY with that flag
(``load_pitch``): three pitch channels -- voiced, log-F0, aperiodicity (``pitch.pitch_channels``) -- then follow the mel rows
(``acoustic.MelPitch``), ``"channels"`` stays what the network takes, mels + 3, and ``mel_count`` is the number of mel rows.

Linear interpolation reads, at every position, the column after the position's own, so a window needs one more column than it
spans.  The library never clamps: the drivers supply that column by repeating the file's last one (``with_extra_column``);
``file_features`` still asks a file for ceil(samples / hop) columns only."""
from __future__ import annotations

import json
import os
from typing import Optional, Tuple

import numpy as np

FILE = "local.json"
DEFAULT_HOP = 256
DEFAULT_MELS, DEFAULT_WIN = 80, 1024          # train --local-mel without --mels / --win
DEFAULT_PITCH = {"fmin": 60.0, "fmax": 500.0, "threshold": 0.15}      # train --local-pitch without --f0-min / --f0-max / --f0-threshold
PITCH_KEYS = ("fmin", "fmax", "threshold")
PITCH_CHANNELS = 3                            # pitch.PITCH_CHANNELS
INTERP = ("repeat", "linear")


def load_config(model_dir: str) -> Optional[Tuple[int, int]]:
    """(channels, hop) of ``<model_dir>/local.json``, or None when the checkpoint is not locally conditioned."""
    filename = os.path.join(model_dir, FILE)
    if not os.path.isfile(filename):
        return None
    try:
        with open(filename) as f:
            d = json.load(f)
        channels, hop = int(d["channels"]), int(d["hop"])
    except Exception:
        raise Exception("could not load {}".format(filename))
    if channels < 1 or hop < 1:
        raise Exception("{}: expected channels >= 1 and hop >= 1".format(filename))
    return channels, hop


def load_interp(model_dir: str) -> Optional[str]:
    """"repeat" or "linear": how ``<model_dir>/local.json`` says the features reach the sample rate (no "interp" key:
    "repeat"); None when the checkpoint is not locally conditioned."""
    if load_config(model_dir) is None:
        return None
    filename = os.path.join(model_dir, FILE)
    with open(filename) as f:
        interp = json.load(f).get("interp", "repeat")
    if interp not in INTERP:
        raise Exception("{}: \"interp\" must be one of {}, got {!r}".format(filename, list(INTERP), interp))
    return interp


def load_upsample(model_dir: str) -> Optional[int]:
    """U of ``<model_dir>/local.json``: the factor of the learned upsampling layer (no "upsample" key: 1, none); None when
    the checkpoint is not locally conditioned."""
    have = load_config(model_dir)
    if have is None:
        return None
    filename = os.path.join(model_dir, FILE)
    with open(filename) as f:
        u = json.load(f).get("upsample", 1)
    if not isinstance(u, int) or u < 1 or have[1] % u:
        raise Exception("{}: \"upsample\" must be an integer >= 1 that divides the hop {}, got {!r}".format(filename, have[1], u))
    return u


def load_mel(model_dir: str) -> Optional[dict]:
    """{"win": W} of ``<model_dir>/local.json`` when the checkpoint was trained on log-mel features of the audio itself
    (``train --local-mel``); None otherwise."""
    if load_config(model_dir) is None:
        return None
    filename = os.path.join(model_dir, FILE)
    with open(filename) as f:
        mel = json.load(f).get("mel")
    if mel is None:
        return None
    if not isinstance(mel, dict) or not isinstance(mel.get("win"), int):
        raise Exception("{}: \"mel\" must be {{\"win\": W}}, got {!r}".format(filename, mel))
    return {"win": int(mel["win"])}


def load_pitch(model_dir: str) -> Optional[dict]:
    """{"fmin": .., "fmax": .., "threshold": ..} of ``<model_dir>/local.json`` when the checkpoint was trained with pitch
    channels behind its mel rows (``train --local-mel --local-pitch``); None otherwise."""
    if load_config(model_dir) is None:
        return None
    filename = os.path.join(model_dir, FILE)
    with open(filename) as f:
        d = json.load(f)
    pitch = d.get("pitch")
    if pitch is None:
        return None
    ok = isinstance(pitch, dict) and sorted(pitch) == sorted(PITCH_KEYS) and all(
        isinstance(pitch[k], (int, float)) and not isinstance(pitch[k], bool) for k in PITCH_KEYS)
    if not ok or "mel" not in d or int(d["channels"]) <= PITCH_CHANNELS:
        raise Exception("{}: \"pitch\" must be {{\"fmin\": .., \"fmax\": .., \"threshold\": ..}} next to \"mel\", with more than {} "
                        "channels, got {!r}".format(filename, PITCH_CHANNELS, pitch))
    return {k: float(pitch[k]) for k in PITCH_KEYS}


def mel_count(model_dir: str) -> Optional[int]:
    """The mel rows of the checkpoint's features: ``channels``, less the 3 pitch channels when ``"pitch"`` is there; None when
    the checkpoint is not locally conditioned."""
    have = load_config(model_dir)
    if have is None:
        return None
    return have[0] - (PITCH_CHANNELS if load_pitch(model_dir) is not None else 0)


def analysis_settings(mel: Optional[dict], pitch: Optional[dict]) -> Optional[dict]:
    """What the drivers hand on as ``local_mel``: the checkpoint's ``"mel"`` entry, with its ``"pitch"`` entry inside under that
    name when there is one (``file_or_mel_features`` reads both)."""
    if mel is None or pitch is None:
        return mel
    return dict(mel, pitch=dict(pitch))


def mel_features(tokens, rate, channels: int, hop: int, win: int, quantization_steps: int, pitch: Optional[dict] = None) -> np.ndarray:
    """The (F, ceil(samples / hop)) float32 log-mel features of a file's tokens as training reads them, made on the device in
    one launch (``features.LogMel``) and brought back: the array ``features --device`` writes for that file, bit for bit.
    ``pitch`` ({"fmin", "fmax", "threshold"}; None: today's path): ``channels`` counts 3 pitch channels behind the mel rows, and
    the array is ``acoustic.MelPitch``'s -- what ``features --device --pitch`` writes."""
    return feature_analyser(rate, channels, hop, win, pitch)(np.asarray(tokens, dtype=np.int32), quantization_steps).cpu().numpy()


def mel_features_of_files(tokens_per_file, rates, channels: int, hop: int, win: int, quantization_steps: int,
                          pitch: Optional[dict] = None):
    """``mel_features`` of every file of a corpus, up to 64 files (one launch per analyser) at a time: by the log-mel contract --
    a column's bits depend on its own samples only -- the arrays of the single calls, bit for bit."""
    from ..features import LOGMEL_MAX_CLIPS
    out, at = [], 0
    while at < len(tokens_per_file):
        end = at + 1
        while end < len(tokens_per_file) and end - at < LOGMEL_MAX_CLIPS and rates[end] == rates[at]:
            end += 1
        cols = feature_analyser(rates[at], channels, hop, win, pitch).batch(
            [np.asarray(t, dtype=np.int32) for t in tokens_per_file[at:end]], quantization_steps)
        out.extend(c.cpu().numpy() for c in cols)
        at = end
    return out


def mel_analyser(rate, channels: int, hop: int, win: int):
    """The ``features.LogMel`` of these settings on the current device (the last one is kept: a run uses one)."""
    import torch
    from .. import features
    key = (float(rate), int(channels), int(hop), int(win), torch.cuda.current_device())
    if key not in _MEL:
        _MEL.clear()
        _MEL[key] = features.LogMel(rate, n_mels=channels, hop=hop, win=win, device="cuda:%d" % key[-1])
    return _MEL[key]


_MEL = {}


def feature_analyser(rate, channels: int, hop: int, win: int, pitch: Optional[dict] = None):
    """The analyser that makes a network's ``channels`` feature rows: ``mel_analyser`` without ``pitch``, else the
    ``acoustic.MelPitch`` of channels - 3 mels and these pitch settings on the current device (the last one is kept)."""
    if pitch is None:
        return mel_analyser(rate, channels, hop, win)
    import torch
    from .. import acoustic
    key = (float(rate), int(channels), int(hop), int(win), tuple(float(pitch[k]) for k in PITCH_KEYS), torch.cuda.current_device())
    if key not in _MEL_PITCH:
        _MEL_PITCH.clear()
        _MEL_PITCH[key] = acoustic.MelPitch(rate, n_mels=int(channels) - PITCH_CHANNELS, hop=hop, win=win, fmin=key[4][0],
                                            fmax=key[4][1], threshold=key[4][2], device="cuda:%d" % key[-1])
    return _MEL_PITCH[key]


_MEL_PITCH = {}


def check_pitch(rate, hop: int, win: int, pitch: dict) -> None:
    """What ``pitch.Pitch`` would refuse at these settings (the lags, the device kernel's shape), raised as its ValueError with
    nothing built."""
    from .. import pitch as _pitch
    tau_min, tau_max = _pitch.pitch_lags(rate, pitch["fmin"], pitch["fmax"])
    why = _pitch._device_refusal(int(win), int(hop), tau_min, tau_max)
    if why:
        raise ValueError(why)
    if not (pitch["threshold"] > 0):
        raise ValueError("Pitch: threshold = %r; it takes a threshold > 0" % (pitch["threshold"],))


def with_extra_column(features: np.ndarray, interp: Optional[str], upsample: int = 1) -> np.ndarray:
    """The features as the network takes them: with ``interp == "linear"`` the last column once more behind the others (the
    column that the last position's interpolation reads); with a learned upsampling layer (``upsample`` > 1) once more
    again (the layer reads pairs of neighbouring columns: n columns make (n - 1) * upsample fine ones) -- what
    ``coarse_frames_needed`` asks for at the file's end; unchanged otherwise."""
    extra = (1 if interp == "linear" else 0) + (1 if int(upsample) > 1 else 0)
    if not extra:
        return features
    return np.ascontiguousarray(np.concatenate([features] + [features[:, -1:]] * extra, axis=1))


def ensure_config(model_dir: str, channels: int, hop: int, interp: Optional[str] = None,
                  upsample: Optional[int] = None, mel: Optional[dict] = None, pitch: Optional[dict] = None) -> Tuple[int, int]:
    """train --local-dir: write the file on the first run; a resumed run must find the SAME values or it stops.  ``interp``:
    what --local-interp gave (None: not given -- a first run then trains "repeat", a resumed one keeps the file's mode).
    ``upsample``: what --local-upsample gave, likewise (None: a first run trains without the layer, a resumed one keeps the
    file's factor); ``"upsample": U`` is written ONLY for U > 1.  ``mel``: {"win": W} of train --local-mel (None: not given);
    ``"mel"`` is written ONLY then, and a resumed --local-mel run must find the same window.  ``pitch``: {"fmin", "fmax",
    "threshold"} of train --local-mel --local-pitch (None: not given; ``channels`` then counts its 3 channels); ``"pitch"`` is
    written ONLY then, and a resumed --local-mel run must find the same three values -- or none -- and the same mel count."""
    if pitch is not None and mel is None:
        raise SystemExit("--local-pitch goes with --local-mel")
    have = load_config(model_dir)
    if interp is not None and interp not in INTERP:
        raise SystemExit("--local-interp must be one of {}, got {!r}".format(list(INTERP), interp))
    if upsample is not None and (int(upsample) < 1 or int(hop) % int(upsample)):
        raise SystemExit("--local-upsample must be >= 1 and divide the hop {}, got {}".format(int(hop), upsample))
    if have is None:
        os.makedirs(model_dir, exist_ok=True)
        d = {"channels": int(channels), "hop": int(hop)}
        if interp == "linear":
            d["interp"] = "linear"
        if upsample is not None and int(upsample) > 1:
            d["upsample"] = int(upsample)
        if mel is not None:
            d["mel"] = {"win": int(mel["win"])}
        if pitch is not None:
            d["pitch"] = {k: float(pitch[k]) for k in PITCH_KEYS}
        with open(os.path.join(model_dir, FILE), "w") as f:
            json.dump(d, f)
        return int(channels), int(hop)
    if mel is not None and load_mel(model_dir) != {"win": int(mel["win"])}:
        was = load_mel(model_dir)
        raise SystemExit("{}: this checkpoint was trained {}, the command line gives --local-mel --win {}: a resumed run must "
                         "find the same value".format(os.path.join(model_dir, FILE),
                                                      "on feature files (no \"mel\")" if was is None else
                                                      "with --local-mel --win {}".format(was["win"]), int(mel["win"])))
    if mel is not None:
        was, now = load_pitch(model_dir), None if pitch is None else {k: float(pitch[k]) for k in PITCH_KEYS}
        say = lambda p: "without --local-pitch (no \"pitch\")" if p is None else \
            "with --local-pitch --f0-min {} --f0-max {} --f0-threshold {}".format(p["fmin"], p["fmax"], p["threshold"])
        if was != now:
            raise SystemExit("{}: this checkpoint was trained {}, the command line gives --local-mel {}: a resumed run must find "
                             "the same values".format(os.path.join(model_dir, FILE), say(was), say(now)))
        if now is not None and have[0] != int(channels):
            raise SystemExit("{}: this checkpoint was trained with --local-pitch on {} mel channels (and 3 pitch channels), the "
                             "command line gives --mels {}: a resumed run must find the same value".format(
                                 os.path.join(model_dir, FILE), have[0] - PITCH_CHANNELS, int(channels) - PITCH_CHANNELS))
    if upsample is not None and int(upsample) != load_upsample(model_dir):
        raise SystemExit("{}: this checkpoint was trained with --local-upsample {}, the command line gives {}: a resumed run "
                         "must find the same value".format(os.path.join(model_dir, FILE), load_upsample(model_dir), int(upsample)))
    if interp is not None and interp != load_interp(model_dir):
        raise SystemExit("{}: this checkpoint was trained with --local-interp {}, the command line gives {}: a resumed run must "
                         "find the same mode".format(os.path.join(model_dir, FILE), load_interp(model_dir), interp))
    if have != (int(channels), int(hop)):
        raise SystemExit("{}: this checkpoint was trained on {} feature channels at hop {}, the command line gives {} at hop {}: "
                         "a resumed run must find the same values".format(os.path.join(model_dir, FILE), have[0], have[1],
                                                                          int(channels), int(hop)))
    return have


def feature_path(feat_dir: str, wav_name: str) -> str:
    return os.path.join(feat_dir, os.path.splitext(os.path.basename(wav_name))[0] + ".npy")


def read_features(filename: str, channels: Optional[int] = None) -> np.ndarray:
    """A (F, frames) float32 array; stops with a message naming the file when it is missing or has another shape."""
    if not os.path.isfile(filename):
        raise SystemExit("local conditioning: the feature file {} is missing".format(filename))
    a = np.load(filename)
    if a.ndim != 2 or a.shape[1] < 1 or a.dtype.kind != "f":
        raise SystemExit("local conditioning: {} must hold a float (F, frames) array, got {} {}".format(filename, a.dtype, a.shape))
    if channels is not None and a.shape[0] != channels:
        raise SystemExit("local conditioning: {} has {} feature channels, the model takes {}".format(filename, a.shape[0], channels))
    return np.ascontiguousarray(a, dtype=np.float32)


def file_features(feat_dir: str, wav_name: str, n_samples: int, channels: int, hop: int) -> np.ndarray:
    """The features of one .wav file, checked against its ``n_samples`` tokens: at least ceil(n_samples / hop) columns."""
    filename = feature_path(feat_dir, wav_name)
    a = read_features(filename, channels)
    need = (int(n_samples) + hop - 1) // hop
    if a.shape[1] < need:
        raise SystemExit("local conditioning: {} has {} columns, but the {} samples of {} need {} at hop {}".format(
            filename, a.shape[1], n_samples, os.path.basename(wav_name), need, hop))
    return a


def directory_channels(feat_dir: str, wav_names) -> int:
    """F, read from the feature file of the first .wav file."""
    names = list(wav_names)
    if not names:
        raise SystemExit("--local-dir: no .wav file to look up a feature file for")
    return int(read_features(feature_path(feat_dir, names[0])).shape[0])


def directory_features(feat_dir: str):
    """generate --local-dir: the names NAME of the ``NAME.npy`` files of ``feat_dir``, sorted; stops when there is none."""
    if not os.path.isdir(feat_dir):
        raise SystemExit("--local-dir: {} is not a directory".format(feat_dir))
    names = sorted(fn[:-4] for fn in os.listdir(feat_dir) if fn.endswith(".npy"))
    if not names:
        raise SystemExit("--local-dir: no .npy feature file in {}".format(feat_dir))
    return names


def samples_covered(frames: int, hop: int, input_width: int) -> int:
    """How many samples generation can emit from ``frames`` feature columns: they cover the utterance from its first sample,
    the window of ``input_width`` samples included, and the first emitted sample is read off the window's last position."""
    return int(frames) * int(hop) - int(input_width) + 1


def padded(features: np.ndarray, pad_samples: int, hop: int) -> Tuple[np.ndarray, int]:
    """Training pads a file with ``pad_samples`` tokens of silence in front; they read the file's column 0.  Returns the
    features with ceil(pad_samples / hop) copies of column 0 in front, and the shift that takes an index into the padded
    tokens to its position on that feature grid (position // hop = column)."""
    cols = (int(pad_samples) + hop - 1) // hop
    ext = np.concatenate([np.repeat(features[:, :1], cols, axis=1), features], axis=1)
    return np.ascontiguousarray(ext), cols * hop - int(pad_samples)


def file_or_mel_features(local_dir, mel, wav_name: str, tokens, rate, channels: int, hop: int, quantization_steps: int):
    """One file's features from either source: its feature file in ``local_dir`` when a directory is given (it wins), else the
    log-mel of its own tokens (``mel`` = {"win": W}; with a "pitch" entry inside, ``analysis_settings``, the mel rows and the pitch
    channels).  Both hand back the same kind of array."""
    if local_dir is not None:
        return file_features(local_dir, wav_name, np.asarray(tokens).size, channels, hop)
    return mel_features(tokens, rate, channels, hop, mel["win"], quantization_steps, pitch=mel.get("pitch"))


def require_match(config, given: bool, what: str, flag: str):
    """A checkpoint with local.json used without features, or features given to one without it: stop with a clear message."""
    if config is not None and not given:
        raise SystemExit("{}: this checkpoint is locally conditioned ({} feature channels at hop {}): give {}".format(
            what, config[0], config[1], flag))
    if config is None and given:
        raise SystemExit("{}: {} was given, but this checkpoint is not locally conditioned (no {})".format(what, flag, FILE))
