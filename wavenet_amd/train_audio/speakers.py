"""Speaker labels of a multi-speaker corpus (new; the reference's to-do list names "Global conditioning" and "Training on
CSTR VCTK Corpus" and has neither): a file's label is its base name up to the first ``_`` (``p225_001.wav`` -> ``p225``), the
sorted label table and the width of the speaker embedding live in ``<model_dir>/speakers.json`` next to ``wavenet.json``
(which stays the reference's file, untouched), and a label's position in the table is the class id the network is
conditioned on (``WaveNet(..., condition_classes, condition_channels)``)."""
from __future__ import annotations

import json
import os
from typing import List, Optional, Sequence, Tuple

FILE = "speakers.json"


def speaker_label(path: str) -> str:
    """``dir/p225_001.wav`` -> ``p225``; a name without ``_`` is its own label, less the extension."""
    base = os.path.basename(path)
    stem = base[:-4] if base.lower().endswith(".wav") else base
    label = stem.split("_", 1)[0]
    if not label:
        raise ValueError("%s: the file name starts with '_', it has no speaker label" % path)
    return label


def label_table(paths: Sequence[str]) -> List[str]:
    """The sorted distinct labels of ``paths``."""
    return sorted({speaker_label(p) for p in paths})


def save_table(model_dir: str, labels: Sequence[str], condition_channels: int) -> str:
    os.makedirs(model_dir, exist_ok=True)
    filename = os.path.join(model_dir, FILE)
    with open(filename, "w") as f:
        json.dump({"speakers": list(labels), "condition_channels": int(condition_channels)}, f, indent=4)
    return filename


def load_table(model_dir: str) -> Optional[Tuple[List[str], int]]:
    """(labels, condition_channels) of ``<model_dir>/speakers.json``, or None when the checkpoint is unconditioned."""
    filename = os.path.join(model_dir, FILE)
    if not os.path.isfile(filename):
        return None
    try:
        with open(filename) as f:
            d = json.load(f)
        labels, channels = [str(s) for s in d["speakers"]], int(d["condition_channels"])
    except Exception:
        raise Exception("could not load {}".format(filename))
    if not labels or labels != sorted(set(labels)) or channels < 1:
        raise Exception("{}: expected a sorted list of distinct labels and condition_channels >= 1".format(filename))
    return labels, channels


def ensure_table(model_dir: str, labels: Sequence[str], condition_channels: int) -> Tuple[List[str], int]:
    """train --speaker-prefix: write the table on the first run; a resumed run must find the SAME table (the class ids are
    positions in it, and the checkpoint's embedding rows belong to them) or it stops."""
    labels = list(labels)
    if not labels:
        raise SystemExit("--speaker-prefix: no .wav file to take a speaker label from")
    if condition_channels is None or int(condition_channels) < 1:
        raise SystemExit("--speaker-prefix needs --condition-channels H with H >= 1")
    have = load_table(model_dir)
    if have is None:
        save_table(model_dir, labels, condition_channels)
        return labels, int(condition_channels)
    if have[0] != labels or have[1] != int(condition_channels):
        raise SystemExit("{}: this checkpoint was trained on speakers {} with {} condition channels, the command line gives {} "
                         "with {}: a resumed run must find the same table".format(
                             os.path.join(model_dir, FILE), have[0], have[1], labels, int(condition_channels)))
    return have


def class_id(labels: Optional[Sequence[str]], label: Optional[str], what: str) -> Optional[int]:
    """The class id of ``label`` (None for an unconditioned checkpoint); stops with a clear message on every mismatch."""
    if labels is None:
        if label is not None:
            raise SystemExit("{}: speaker {!r} was given, but this checkpoint is not conditioned on speakers (no {})".format(
                what, label, FILE))
        return None
    if label is None:
        raise SystemExit("{}: this checkpoint is conditioned on speakers {}: name one (--speaker LABEL)".format(what, list(labels)))
    if label not in labels:
        raise SystemExit("{}: unknown speaker {!r}; this checkpoint knows {}".format(what, label, list(labels)))
    return list(labels).index(label)


def utterance_speakers(speakers: Optional[Sequence[str]], n: int) -> List[Optional[str]]:
    """``--speaker`` given zero times, once (for all ``n`` utterances) or ``n`` times (one each) -> ``n`` labels."""
    given = list(speakers or [])
    if len(given) not in (0, 1, n):
        raise ValueError("%d --speaker labels for %d utterances: give one for all of them, or one each" % (len(given), n))
    return given * n if len(given) == 1 else given or [None] * n
