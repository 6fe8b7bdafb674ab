"""What ``wn_corpus_gather`` must write, restated in numpy from the pieces the per-file path is made of -- not from the kernel's
index formula: per file, the padded signal of ``train_audio`` (``input_width`` silence tokens in front) and
``local.padded(local.with_extra_column(...))``, then the slices and the clamp of ``_Crops.draw``.  Integers and copied floats:
the kernel equals this bit for bit."""
import numpy as np

from wavenet_amd.train_audio import local as L


def silence_of(quantization_steps):
    return 127 if quantization_steps > 127 else quantization_steps // 2          # train_audio


def gather(tokens_per_file, input_width, quantization_steps, files, starts, target_width, features=None, hop=0, classes=None,
           n_cols=None, interp="repeat", upsample=1):
    """-> (x, tgt, local or None, condition or None, phases or None) of the crops (files[b], starts[b])."""
    iw, tw = int(input_width), int(target_width)
    padded, ext, shift = {}, {}, 0
    xs, tgts, locs, phases = [], [], [], []
    for f, s in zip(files, starts):
        f, s = int(f), int(s)
        if f not in padded:
            padded[f] = np.concatenate([np.full((iw,), silence_of(quantization_steps), dtype=np.int32),
                                        np.asarray(tokens_per_file[f]).astype(np.int32)])            # train.py:53
            if features is not None:
                ext[f], shift = L.padded(L.with_extra_column(np.asarray(features[f], dtype=np.float32), interp, upsample), iw, hop)
        win = padded[f][s + np.arange(iw + tw + 1)]                                                  # _Crops.draw: signal[idx]
        xs.append(win[:iw + tw])
        tgts.append(win[iw + 1:])
        if features is not None:
            pos = s + shift
            phases.append(pos % hop)
            cols = np.minimum(pos // hop + np.arange(int(n_cols)), ext[f].shape[1] - 1)             # ... torch.clamp(max=...)
            locs.append(ext[f][:, cols])
    x, tgt = np.stack(xs).astype(np.int32), np.stack(tgts).astype(np.int32)
    local = np.ascontiguousarray(np.stack(locs), dtype=np.float32) if features is not None else None
    cond = None if classes is None else np.asarray([classes[int(f)] for f in files], dtype=np.int64)
    return x, tgt, local, cond, (np.asarray(phases, dtype=np.int32) if features is not None else None)


def of_corpus(corpus, files, starts, target_width, n_cols=None, interp="repeat", upsample=1):
    """``gather`` on the files a ``Corpus`` packed (its host arrays, cut apart again)."""
    tokens = [corpus.tokens[o:o + n] for o, n in zip(corpus.file_offset, corpus.file_len)]
    feats = None
    if corpus.features is not None:
        feats = [corpus.features[:, o:o + n] for o, n in zip(corpus.col_offset, corpus.col_count)]
    return gather(tokens, corpus.input_width, corpus.quantization_steps, files, starts, target_width, feats, corpus.hop,
                  corpus.file_class, n_cols, interp, upsample)


def legal_starts(n_tokens, input_width, target_width, hop=0, crop="sample"):
    """Every start ``_Crops`` can draw on one file, from its own expressions (train.py ``_Crops.draw``)."""
    n = int(n_tokens) + int(input_width)                     # the padded signal
    hi = n - target_width - input_width - 1
    if hi <= 0:
        return []
    if crop == "sample" or not hop:
        return list(range(hi))
    shift = -(-input_width // hop) * hop - input_width      # local.padded
    r = (-shift) % hop
    if hi - r <= 0:
        return []
    return [r + hop * k for k in range((hi - r + hop - 1) // hop)]
