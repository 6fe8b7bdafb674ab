"""Objective copy-synthesis metrics: how close a resynthesis is to the recording it was made from.

    log_mel_distance   the log-spectral distance on the mel scale, in dB
    f0_metrics         F0 error in cents, gross F0 errors, voiced / unvoiced errors (from two ``pitch.yin`` / ``pitch.Pitch`` arrays)
    copy_synthesis     files -> their resynthesis under their own features in ONE ``generate_batch`` run -> those figures per file
    pick_closest       the candidate with the smallest distance (the counterpart of ``sampling.pick_best``)

Small numpy functions; the analysis itself runs on the device (``features.LogMel``, ``pitch.Pitch``)."""
from __future__ import annotations

import math

import numpy as np

from . import sampling

DB_PER_NAT = 20.0 / math.log(10.0)       # a natural-log magnitude in dB


def _host(a):
    return np.asarray(a.detach().cpu() if hasattr(a, "detach") else a, dtype=np.float64)


def log_mel_distance(a, b):
    """``a``, ``b``: (F, n) natural-log magnitude mel arrays (numpy or tensors).  Per column the root mean square over the F
    channels of (20 / ln 10) (a - b), in dB.  Returns (the mean over columns -- None when n = 0 --, the (n,) float64 vector)."""
    a, b = _host(a), _host(b)
    if a.ndim != 2 or a.shape != b.shape:
        raise ValueError("log_mel_distance: two (F, n) arrays of one shape, got %s and %s" % (a.shape, b.shape))
    diff = DB_PER_NAT * (a - b)
    per_column = np.sqrt(np.mean(diff * diff, axis=0)) if a.shape[0] else np.zeros((a.shape[1],))
    return (float(per_column.mean()) if per_column.size else None), per_column


def f0_metrics(ref, got):
    """``ref``, ``got``: (2, n) pitch arrays (row 0: F0 in Hz, 0 = unvoiced).  Returns
    ``voiced_frames``   frames voiced in both
    ``f0_rmse_cents``   the RMS of 1200 log2(got / ref) over those frames
    ``f0_gross_error``  the share of those frames with |got / ref - 1| > 0.2
    ``vuv_error``       the share of all n frames whose voicing differs
    -- None, not NaN, where there is no frame to average."""
    ref, got = _host(ref), _host(got)
    if ref.ndim != 2 or ref.shape[0] != 2 or ref.shape != got.shape:
        raise ValueError("f0_metrics: two (2, n) arrays of one shape, got %s and %s" % (ref.shape, got.shape))
    n = ref.shape[1]
    vr, vg = ref[0] > 0, got[0] > 0
    both = vr & vg
    out = {"frames": int(n), "voiced_frames": int(both.sum()), "f0_rmse_cents": None, "f0_gross_error": None,
           "vuv_error": float((vr != vg).mean()) if n else None}
    if out["voiced_frames"]:
        ratio = got[0, both] / ref[0, both]
        cents = 1200.0 * np.log2(ratio)
        out["f0_rmse_cents"] = float(np.sqrt(np.mean(cents * cents)))
        out["f0_gross_error"] = float((np.abs(ratio - 1.0) > 0.2).mean())
    return out


def pick_closest(distances) -> int:
    """The index of the smallest of ``distances``, the lowest index on ties.  None and NaN never win: index 0 comes back only
    when every value is one of them."""
    vals = [float("nan") if v is None else float(v) for v in distances]
    if not vals:
        raise ValueError("pick_closest: no candidate")
    return sampling.pick_best(vals)


def first_free_column(window: int, span: int, hop: int) -> int:
    """The first column whose analysis span -- ``span`` samples from k * hop - span // 2 on -- starts at or behind sample
    ``window``: the columns before it read samples of the window."""
    return -(-(int(window) + int(span) // 2) // int(hop))


def copy_synthesis(net, tokens, feats, condition, uniforms, mel, pitch, forced=None, fold=None, **controls):
    """Copy synthesis as ``generate --keep`` frames it, for a list of files at once.  ``tokens[u]``: file u's M_u tokens as
    training reads them; ``feats[u]``: its (F, columns) features as the network takes them, written for the file, so that they fit
    at phase 0; ``condition``: None or a class id per file; ``uniforms[u]``: M_u - W uniforms; ``mel`` / ``pitch``: a
    ``features.LogMel`` and a ``pitch.Pitch`` on the files' column grid; ``forced``: passed on to ``generate_batch`` (None, or per
    file an array over the M_u - W emitted positions); ``controls``: temperature, top_k, top_p.

    The alignment rule.  With W = ``net.input_width``, file u's first W samples are the window; the M_u - W samples behind it
    are drawn under the file's features, all files in ONE ``generate_batch`` call.  The compared signal is the window followed by
    the drawn samples: the file's length, the file's column grid (column k is centred on sample k * hop).  A column whose
    analysis span touches the window is left out -- it would be made of the file's own samples and flatter the result: the mel
    columns compared are k >= ceil((W + win / 2) / hop), the pitch columns k >= ceil((W + S / 2) / hop), S = win + tau_max.

    ``fold`` = (body, overlap, warmup), the arguments of ``FasterWaveNet.generate_folded`` (an int or ``"auto"``; ints or None for
    the method's defaults): the M_u - W samples are drawn folded instead -- every file cut into overlapping segments, all segments
    of all files in ONE batched call, cross-faded -- with the same uniforms, keyed by position.  What comes back is a signal, not
    tokens, so BOTH sides are then analysed as floats, ``pcm / 32768`` through one table (``data.pcm_table``): the file as
    ``table[tokens]``, the resynthesis as ``table[window]`` followed by the folded signal.  The same three figures, on the same
    columns: what a body, an overlap and a warm-up cost on a trained model.  ``nats_per_sample`` is that of the segments owning
    the positions; ``emitted`` holds the int16 signal; a row gains ``fold``: {"segments", "body", "overlap", "warmup",
    "identical_seams"}.  Not with ``forced``.

    Returns one dict per file: ``samples`` (M_u), ``emitted`` (the M_u - W tokens), ``nats_per_sample`` (of the emitted samples,
    from ``chosen``), ``log_mel_distance_db``, ``mel_columns``, ``pitch_columns``, and ``f0_metrics``'s entries."""
    import torch
    Q, W = net.params.quantization_steps, int(net.input_width)
    toks = [np.asarray(t, dtype=np.int32).reshape(-1) for t in tokens]
    N = len(toks)
    if not N or len(feats) != N or len(uniforms) != N or (condition is not None and len(condition) != N):
        raise ValueError("copy_synthesis: one entry per file in tokens, feats, uniforms and condition (%d files)" % N)
    for u, t in enumerate(toks):
        if t.size < W + 2:
            raise ValueError("copy_synthesis: file %d holds %d samples; the window takes %d and the decoder runs two more at least"
                             % (u, t.size, W))
    lengths = [t.size - W for t in toks]
    if fold is not None:
        from . import data
        from . import fold as _fold
        if forced is not None:
            raise ValueError("copy_synthesis: fold= does not go with forced=: given samples are not part of a folded run")
        body, overlap, warmup = fold
        pcm, chosen, segs = net.generate_folded(lengths, [np.asarray(r, dtype=np.float64).reshape(-1) for r in uniforms], body, overlap,
                                                warmup, initial_tokens=np.stack([t[:W] for t in toks]), condition=condition,
                                                local=list(feats), return_chosen=True, return_segments=True, **controls)
        table = torch.as_tensor(data.pcm_table(Q).astype(np.float32)).to(pcm[0].device)
        as_float = lambda t: table[torch.as_tensor(t).to(table.device).long()]
        emitted = pcm
        files = [as_float(t) / 32768.0 for t in toks]
        whole = [torch.cat([as_float(t[:W]), e.to(torch.float32)]) / 32768.0 for t, e in zip(toks, emitted)]
        mels, pits = mel.batch(files + whole), pitch.batch(files + whole)
        folds = [{"segments": len(plan.segments), "body": plan.body, "overlap": plan.overlap, "warmup": plan.warmup,
                  "identical_seams": _fold.identical_seams([r.cpu().numpy() for r in rows], plan)} for plan, rows, _ in segs]
        return _copy_rows(toks, emitted, chosen, mels, pits, W, mel, pitch, folds)
    rows, chosen = net.generate_batch(lengths, [np.asarray(r, dtype=np.float64).reshape(-1) for r in uniforms],
                                      initial_tokens=np.stack([t[:W] for t in toks]), condition=condition, local=list(feats),
                                      return_chosen=True, forced=forced, **controls)
    emitted = [r.to(torch.int32) for r in rows]
    whole = [torch.cat([torch.as_tensor(t[:W]).to(e.device), e]) for t, e in zip(toks, emitted)]
    return _copy_rows(toks, emitted, chosen, mel.batch(toks + whole, Q), pitch.batch(toks + whole, Q), W, mel, pitch)


def _copy_rows(toks, emitted, chosen, mels, pits, W, mel, pitch, folds=None):
    """``copy_synthesis``'s rows from the analysed columns: ``mels`` / ``pits`` hold the N files' arrays, then the N resyntheses'."""
    N, out = len(toks), []
    for u in range(N):
        km = first_free_column(W, mel.win, mel.hop)
        kp = first_free_column(W, pitch.span, pitch.hop)
        dist, per_column = log_mel_distance(mels[u][:, km:], mels[N + u][:, km:])
        row = {"samples": int(toks[u].size), "emitted": emitted[u].cpu().numpy(), "nats_per_sample": sampling.chosen_nll(chosen[u]),
               "log_mel_distance_db": dist, "mel_columns": int(per_column.size)}
        f0 = f0_metrics(pits[u][:, kp:], pits[N + u][:, kp:])
        row["pitch_columns"] = f0.pop("frames")
        row.update(f0)
        if folds is not None:
            row["fold"] = folds[u]
        out.append(row)
    return out


FIGURES = (("log_mel_distance_db", "mel_columns"), ("f0_rmse_cents", "voiced_frames"), ("f0_gross_error", "voiced_frames"),
           ("vuv_error", "pitch_columns"), ("nats_per_sample", "emitted_samples"))


def total(rows):
    """The figures of ``copy_synthesis``'s rows as one: each the mean of the files' values weighted by what it was averaged over
    (compared mel columns, frames voiced in both, compared pitch columns, emitted samples); ``f0_rmse_cents`` the root of the
    weighted mean square.  None where no file has a value."""
    out = {"samples": int(sum(r["samples"] for r in rows)), "voiced_frames": int(sum(r["voiced_frames"] for r in rows))}
    for key, weight in FIGURES:
        acc, n = 0.0, 0
        for r in rows:
            w = len(r["emitted"]) if weight == "emitted_samples" else r[weight]
            if r[key] is None or not w:
                continue
            acc += (r[key] ** 2 if key == "f0_rmse_cents" else r[key]) * w
            n += w
        out[key] = None if not n else (math.sqrt(acc / n) if key == "f0_rmse_cents" else acc / n)
    return out
