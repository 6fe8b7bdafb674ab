"""Generation driver (train_audio/generate.py:9-63): start from ``input_width`` samples of silence (token 127), draw
``int(sampling_rate * seconds) - 1`` samples one at a time from the softmax, write ``<output_dir>/generated.wav``.

Beyond the reference: ``--utterances N`` and ``--prompt FILE.wav`` write ``generated_000.wav`` ... ``generated_{N-1:03d}.wav``,
each continuing its prompt (or silence); with ``--fast`` all of them in one ``FasterWaveNet.generate_batch`` run.
``--fast --local-dir FEAT_DIR`` vocodes a directory: ``<output_dir>/NAME.wav`` for every ``FEAT_DIR/NAME.npy``, each at the
length its own features cover, all in one ragged ``generate_batch`` run.
``--fast --report FILE.json`` writes the negative log-likelihood the model gave every written file (nats and bits per emitted
sample, as ``evaluate`` prints for held-out audio); ``--fast --best-of K`` draws every utterance K times in the same batched
run and keeps the candidate the model found most likely.  Likelihood rewards quiet, predictable audio: it ranks candidates
(most usefully when vocoding from features), it does not measure quality.  ``--fast --from-wav FILE.wav --best-of K --rank mel``
keeps the candidate whose log-mel columns are closest to the recording's own instead (``wavenet_amd/metrics.py``).
``--fast --keep FILE.wav [--redraw A:B ...]`` regenerates stretches of a recording: the file's first ``input_width`` samples are
the window, every later sample is emitted as the file has it (``FasterWaveNet.generate(..., forced=...)``) unless a ``--redraw``
range, in seconds of the file, covers it, and the output is the file with those ranges drawn anew.  Without ``--redraw`` the
run keeps everything and ``--report`` is the decoder's own likelihood of the file; ``--best-of K`` ranks on the figure over all
emitted samples, kept ones included -- a candidate is judged by how the real audio continues from what was drawn into it.
``--fast --local FILE.npy --chunk-frames C [--ring-frames R]`` vocodes as a stream (``FasterWaveNet.open_stream``): C feature
columns at a time go to the decoder, which draws what they allow; ``generated.wav`` grows as it goes, and the time to its first
chunk is printed.
On a checkpoint trained with ``train --local-mel --local-pitch`` the features carry three pitch channels behind the mel rows
(``acoustic.MelPitch`` makes them from a ``--from-wav`` recording, streamed or not), and ``--f0-scale S`` multiplies the pitch of
every voiced column by S before the network sees it (``pitch.scale_f0``).
``--fast --fold SECONDS|auto [--fold-overlap SECONDS] [--fold-warmup SECONDS]`` (a locally conditioned checkpoint; with ``--local``,
``--local-dir`` or ``--from-wav``) decodes every utterance folded: cut into overlapping segments that run side by side in the one
batched call and are cross-faded where they meet (``FasterWaveNet.generate_folded``, ``wavenet_amd/fold.py``), from the uniforms the
command draws without the flag."""
from __future__ import annotations

import json
import math
import os
import sys
import time

import numpy as np
import torch

from .. import data, features, sampling
from ..faster_wavenet import silence_window
from . import args as _args
from . import local as _local
from . import model as _model
from . import speakers as _speakers
from .train import input_width_of


def _host_loop(net, window, n, sampling_rate, generate_sec, temperature, top_k, top_p, condition=None, local=None):
    """The reference's loop (generate.py:24-43) from the given window: one ``forward_one_step`` over the last
    ``input_width`` tokens and one draw per sample, on the host; returns the ``n`` emitted tokens."""
    Q = net.params.quantization_steps
    controls = not sampling.controls_off(temperature, top_k, top_p, Q)
    iw = len(window)
    buf = np.array(window, dtype=np.int32)
    cond = {} if condition is None else {"condition": [condition]}
    hop = net.local_hop if local is not None else 0
    for time_step in range(1, n + 1):
        x = torch.as_tensor(buf[-iw:].reshape(1, -1)).to(net.device)
        if local is not None:
            # the window's first sample is sample time_step - 1 of the utterance (prompt included): local_alignment's rule
            col, ph = divmod(time_step - 1, hop)
            cond["local"], cond["local_phase"] = local[None, :, col:], ph
        if not controls:
            with torch.no_grad():
                softmax = net.forward_one_step(x, apply_softmax=True, as_numpy=True, **cond)[0, :, 0, -1]
            buf = np.append(buf, np.random.choice(np.arange(Q), p=softmax))
        else:
            # the same rule the device applies under --fast, on the host: logits / temperature, softmax, truncation, and
            # choice()'s draw from its one uniform
            with torch.no_grad():
                logits = net.forward_one_step(x, apply_softmax=False, as_numpy=True, **cond)[0, :, 0, -1]
            softmax = sampling.apply_temperature(logits, temperature)
            buf = np.append(buf, sampling.sample(softmax, np.random.random_sample(), top_k, top_p))
        if time_step % 10 == 0:
            sys.stdout.write("\rgenerating {:.2f} msec / {:.2f} msec".format(
                time_step * 1000.0 / sampling_rate, generate_sec * 1000.0))
            sys.stdout.flush()
    return buf[iw:]


def _save(start_time, output_dir, Q, sampling_rate, named):
    """Report the time since ``start_time``, make the directory and write ``<output_dir>/<name>.wav`` for every (name, tokens)
    pair; returns the file names."""
    print("\ndone in {:.3f} sec".format(time.time() - start_time))
    os.makedirs(output_dir, exist_ok=True)
    filenames = ["{}/{}.wav".format(output_dir, name) for name, _ in named]
    for filename, (_, tokens) in zip(filenames, named):
        data.save_audio_file(filename, tokens, Q, format="16bit_pcm", sampling_rate=sampling_rate)
    return filenames


def likelihood_job(args):
    """``generate --report FILE.json / --best-of K``: the checks, made before a model is built.  Returns (K, FILE or None)."""
    K, report = int(args.best_of), args.report
    if K < 1:
        raise SystemExit("generate: --best-of K needs K >= 1, got {}".format(K))
    if (K > 1 or report) and not args.fast:
        raise SystemExit("generate: --report and --best-of read the probability of every emitted sample from the decoder on "
                         "the device: give --fast")
    return K, report


def rank_job(args):
    """``generate --rank likelihood|mel``: the checks, made before a model is built.  Returns whether the candidates are ranked
    on their distance to the recording's mel columns."""
    if args.rank not in ("likelihood", "mel"):
        raise SystemExit("generate: --rank takes likelihood or mel, got {!r}".format(args.rank))
    if args.rank == "likelihood":
        return False
    if not args.from_wav:
        bad = [f for f, on in (("--local", args.local), ("--local-dir", args.local_dir is not None), ("--keep", args.keep)) if on]
        raise SystemExit("generate: --rank mel compares every candidate with the columns of the recording it was made from: give "
                         "--from-wav FILE.wav{}".format(" (it does not go with {})".format(", ".join(bad)) if bad else ""))
    if args.chunk_frames is not None:
        raise SystemExit("generate: --rank mel analyses whole candidates and does not go with --chunk-frames")
    return True


class MelRank(object):
    """``--rank mel``: the candidates of a run against the columns of the recordings they were made from.  A candidate is the
    window followed by its emitted samples, on the recording's column grid (``metrics.copy_synthesis`` states the rule): its
    columns come from one ``LogMel.batch`` call over all candidates, and those whose window touches the generation's window
    are left out, as are those past the shorter of the two.  The window that is put in front is always silence, also where a
    run continues a ``--prompt``: no compared column reads a sample of the window, so what it holds does not matter."""

    def __init__(self, analyser_of, rates, targets, quantization_steps, window):
        """``analyser_of(rate)``: the ``features.LogMel`` of the checkpoint's settings at that rate; ``rates[u]`` / ``targets[u]``:
        the rate recording u was analysed at and its (F, columns) array."""
        self.analyser_of, self.rates, self.targets, self.Q = analyser_of, list(rates), list(targets), int(quantization_steps)
        self.window = np.asarray(window, dtype=np.int32)

    def distances(self, rows, K):
        """The log-mel distance in dB of every row, row ``u * K + c`` against target u (None where no column is compared).  The
        rows of recordings at one rate -- as a rule all of them -- are analysed in one ``LogMel.batch`` call."""
        from .. import metrics
        win = torch.as_tensor(self.window)
        sig = [torch.cat([win, torch.as_tensor(np.asarray(r.cpu() if isinstance(r, torch.Tensor) else r, dtype=np.int32))]) for r in rows]
        out = [None] * len(sig)
        for rate in sorted(set(self.rates)):
            an = self.analyser_of(rate)
            mine = [i for i in range(len(sig)) if self.rates[i // K] == rate and sig[i].numel() > an.win // 2]
            if not mine:
                continue
            k0 = metrics.first_free_column(self.window.size, an.win, an.hop)
            for i, c in zip(mine, an.batch([sig[i] for i in mine], self.Q)):
                t = self.targets[i // K]
                n = min(int(c.shape[1]), int(t.shape[1]))
                out[i] = metrics.log_mel_distance(t[:, k0:n], c[:, k0:n])[0] if n > k0 else None
        return out

    def keep_best(self, tokens, chosen, K):
        """``_keep_best`` with the ranking on the distances: (kept tokens, [(kept index, nats of every candidate)], the kept
        candidates' distances)."""
        from .. import metrics
        nlls = [sampling.chosen_nll(c) for c in chosen]
        dist = self.distances(tokens, K)
        ranked = [(metrics.pick_closest(dist[u * K:(u + 1) * K]), nlls[u * K:(u + 1) * K]) for u in range(len(nlls) // K)]
        kept = [tokens[u * K + k] for u, (k, _) in enumerate(ranked)]
        return ([np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in kept], ranked,
                [dist[u * K + k] for u, (k, _) in enumerate(ranked)])


def f0_scale_job(args):
    """``generate --f0-scale S``: the checks, made before a model is built.  Returns None without the flag, else (S, fmin, fmax,
    F): the scale, the checkpoint's pitch band and its mel count -- rows F .. F + 2 of a feature array are the pitch channels."""
    if "f0_scale" not in vars(args):
        return None
    S = float(args.f0_scale)
    pitch = _local.load_pitch(args.model_dir)
    if pitch is None:
        raise SystemExit("generate: --f0-scale moves the pitch channels of a checkpoint trained with train --local-mel --local-pitch "
                         "({} has no \"pitch\")".format(os.path.join(args.model_dir, _local.FILE)))
    if not (math.isfinite(S) and S > 0):
        raise SystemExit("generate: --f0-scale S needs a finite S > 0, got {}".format(args.f0_scale))
    if args.rank == "mel":
        raise SystemExit("generate: --f0-scale does not go with --rank mel: the recording is no target for a shifted voice")
    if args.keep:
        raise SystemExit("generate: --f0-scale does not go with --keep: the kept samples carry the recording's own pitch")
    return S, pitch["fmin"], pitch["fmax"], _local.mel_count(args.model_dir)


def scaled_f0(feats, f0):
    """A (F + 3, columns) feature array (numpy or tensor) as the network is to see it under ``--f0-scale``: ``pitch.scale_f0`` on
    rows F .. F + 2, the other rows' bits kept; the array itself without the flag or at S = 1."""
    if f0 is None or f0[0] == 1.0:
        return feats
    from ..pitch import scale_f0
    S, fmin, fmax, F = f0
    out = feats.copy() if isinstance(feats, np.ndarray) else feats.clone()
    out[F:] = scale_f0(feats[F:], S, fmin, fmax)
    return out


def tile_job(args):
    """``generate --tile auto|2|4|8|16``: the check, made before a model is built.  Returns None without the flag, else what
    ``FasterWaveNet.batch_tile`` takes: ``"auto"`` or the tile size."""
    if args.tile is None:
        return None
    if not args.fast:
        raise SystemExit("generate: --tile sizes the utterance tiles of the decoder on the device: give --fast")
    if args.tile != "auto" and args.tile not in ("2", "4", "8", "16"):
        raise SystemExit("generate: --tile takes auto, 2, 4, 8 or 16, got {!r}".format(args.tile))
    return "auto" if args.tile == "auto" else int(args.tile)


def _keep_best(tokens, chosen, K):
    """``tokens`` / ``chosen``: N * K rows, row ``u * K + c`` candidate c of utterance u (1-D arrays or device tensors) ->
    (the kept candidate's tokens per utterance as numpy, [(kept index, [nats per sample of every candidate])])."""
    nlls = [sampling.chosen_nll(c) for c in chosen]
    ranked = [(sampling.pick_best(nlls[u * K:(u + 1) * K]), nlls[u * K:(u + 1) * K]) for u in range(len(nlls) // K)]
    kept = [tokens[u * K + k] for u, (k, _) in enumerate(ranked)]
    return [np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t) for t in kept], ranked


def write_report(path, filenames, tokens, ranked, K, distances=None, folds=None):
    """``--report``: per written file {"file", "samples", "nats_per_sample", "bits_per_sample"} (the emitted samples only: no
    prompt, no window) and, with ``--best-of K`` > 1, "candidates" (every candidate's nats per sample) and "kept"; then the
    total weighted by samples, in the layout of ``evaluate --json``.  ``distances`` (``--rank mel``: the kept candidates'): every
    row gains "log_mel_distance_db" and the table "rank": "mel".  Returns the table."""
    rows, nats, samples = [], 0.0, 0
    for i, (fn, t, (k, cand)) in enumerate(zip(filenames, tokens, ranked)):
        row = {"file": os.path.basename(fn), "samples": int(len(t)), "nats_per_sample": cand[k],
               "bits_per_sample": cand[k] / math.log(2.0)}
        if K > 1:
            row["candidates"], row["kept"] = list(cand), int(k)
        if distances is not None:
            row["log_mel_distance_db"] = distances[i]
        if folds is not None:
            row["fold"] = folds[i]
        rows.append(row)
        nats += cand[k] * len(t) if len(t) else 0.0
        samples += int(len(t))
    mean = nats / samples if samples else 0.0
    table = {"files": rows, "total": {"samples": samples, "nats_per_sample": mean, "bits_per_sample": mean / math.log(2.0)}}
    if distances is not None:
        table["rank"] = "mel"
    with open(path, "w") as f:
        json.dump(table, f, indent=2)
    return table


def fold_job(args):
    """``generate --fold SECONDS|auto [--fold-overlap SECONDS] [--fold-warmup SECONDS]``: every check, made before a model is built.
    Returns None without ``--fold``, else (body, overlap, warmup) in samples as ``FasterWaveNet.generate_folded`` takes them: the
    body an int or ``"auto"``, the other two None where the flag was not given (the method's defaults)."""
    given = vars(args)
    if "fold" not in given:
        extra = [f for f, k in (("--fold-overlap", "fold_overlap"), ("--fold-warmup", "fold_warmup")) if k in given]
        if extra:
            raise SystemExit("generate: {} sizes the segments of a folded run: give --fold SECONDS|auto".format(" and ".join(extra)))
        return None
    if not args.fast:
        raise SystemExit("generate: --fold decodes the segments of an utterance in one batched run on the device: give --fast")
    bad = [f for f, on in (("--chunk-frames", args.chunk_frames is not None), ("--keep", args.keep),
                           ("--best-of {}".format(args.best_of), int(args.best_of) > 1), ("--rank", "rank" in given)) if on]
    if bad:
        raise SystemExit("generate: --fold does not go with {}: streams, given samples and ranked candidates are not cut into "
                         "segments".format(", ".join(bad)))
    if _local.load_config(args.model_dir) is None:
        raise SystemExit("generate: --fold needs a locally conditioned checkpoint -- the features are what makes the segments of "
                         "one utterance agree -- and {} is missing".format(os.path.join(args.model_dir, _local.FILE)))
    sr = float(_model.load_params(args.model_dir).sampling_rate)

    def samples(flag, text, least):
        try:
            sec = float(text)
        except (TypeError, ValueError):
            sec = float("nan")
        if not math.isfinite(sec) or int(round(sec * sr)) < least:
            raise SystemExit("generate: {} takes seconds ({} sample{} at least{}), got {!r}".format(
                flag, least, "" if least == 1 else "s", ", or auto" if flag == "--fold" else "", text))
        return int(round(sec * sr))
    body = "auto" if args.fold == "auto" else samples("--fold", args.fold, 1)
    overlap = samples("--fold-overlap", args.fold_overlap, 0) if "fold_overlap" in given else None
    warmup = samples("--fold-warmup", args.fold_warmup, 0) if "fold_warmup" in given else None
    if body != "auto" and overlap is not None and overlap > body:
        raise SystemExit("generate: --fold-overlap {:g} is {} samples, more than the {} of --fold {}: a seam lies inside one body".format(
            args.fold_overlap, overlap, body, args.fold))
    return body, overlap, warmup


def generate_folded_files(net, params, names, lengths, uniforms, prompts, feats, cids, fold, output_dir="generated_audio",
                          temperature=1.0, top_k=0, top_p=1.0, report=None):
    """``generate --fold``: ONE ``FasterWaveNet.generate_folded`` call over the files of the run -- file u of ``lengths[u]`` samples
    behind the window ``prompts[u]``, drawn with ``uniforms[u]`` (the row the command draws without the flag) under
    ``feats[u]`` as speaker ``cids[u]`` -- and ``<output_dir>/<names[u]>.wav`` per file (``data.save_pcm_file``).  ``fold``: what
    ``fold_job`` returned.  ``report``: ``write_report``'s file; a file's nats are those of the segments that own its positions,
    and its row gains "fold": {"segments", "body", "overlap", "warmup", "identical_seams"}.  Returns (filenames, signals)."""
    from .. import fold as _fold
    body, overlap, warmup = fold
    start_time = time.time()
    got = net.generate_folded(list(lengths), list(uniforms), body, overlap, warmup, initial_tokens=np.stack(prompts), condition=cids,
                              local=list(feats), temperature=temperature, top_k=top_k, top_p=top_p, return_chosen=bool(report),
                              return_segments=bool(report))
    pcm = [p.cpu().numpy() for p in (got[0] if report else got)]
    print("\ndone in {:.3f} sec".format(time.time() - start_time))
    os.makedirs(output_dir, exist_ok=True)
    filenames = ["{}/{}.wav".format(output_dir, name) for name in names]
    for filename, signal in zip(filenames, pcm):
        data.save_pcm_file(filename, signal, params.sampling_rate)
    if report:
        ranked = [(0, [sampling.chosen_nll(c)]) for c in got[1]]
        folds = [{"segments": len(plan.segments), "body": plan.body, "overlap": plan.overlap, "warmup": plan.warmup,
                  "identical_seams": _fold.identical_seams([r.cpu().numpy() for r in rows], plan)} for plan, rows, _ in got[2]]
        write_report(report, filenames, pcm, ranked, 1, folds=folds)
    return filenames, pcm


def generate_audio(net, params, sampling_rate=48000, generate_sec=1.0, fast=False, output_dir="generated_audio",
                   temperature=1.0, top_k=0, top_p=1.0, condition=None, local=None, best_of=1, report=None, rank=None, fold=None):
    """``rank``: None (the candidates of ``best_of`` are ranked on their likelihood) or a ``MelRank``; ``fold``: None or what
    ``fold_job`` returned (``generate_folded_files`` with the uniforms drawn here without it)."""
    Q = params.quantization_steps
    sampling.check_controls(temperature, top_k, top_p)
    n = int(sampling_rate * generate_sec) - 1                       # generate.py:24: time_step runs 1 .. n
    silence = silence_window(Q, input_width_of(params))
    if fold is not None and n > 0:
        (filename,), (signal,) = generate_folded_files(net, params, ["generated"], [n], [np.random.random_sample(n)], [silence], [local],
                                                       None if condition is None else [condition], fold, output_dir, temperature,
                                                       top_k, top_p, report)
        return filename, signal
    start_time = time.time()
    ranked = dists = None
    if fast and (best_of > 1 or report or rank is not None):
        lkw = {} if local is None else {"local": local}
        kw = dict(initial_tokens=silence, temperature=temperature, top_k=top_k, top_p=top_p, condition=condition,
                  return_chosen=True, **lkw)
        if n <= 0:
            rows, chosen = [np.zeros((0,), np.int32)] * best_of, [np.zeros((0,), np.float32)] * best_of
        elif best_of == 1:
            rows, chosen = [[v] for v in net.generate(n, np.random.random_sample(n), **kw)]
        else:
            # K candidates of the one utterance are K utterances of a batched run: same prompt, speaker, features, controls
            rows, chosen = net.generate_batch(n, np.random.random_sample((best_of, n)), **kw)
        if rank is None:
            (tokens,), ranked = _keep_best(list(rows), list(chosen), best_of)
        else:
            (tokens,), ranked, dists = rank.keep_best(list(rows), list(chosen), best_of)
    elif n <= 0:
        tokens = np.zeros((0,), np.int32)
    elif fast:
        # one uniform per sample, the draw numpy's choice() makes (generate.py:40); the whole loop runs on the device
        u = np.random.random_sample(n)
        lkw = {} if local is None else {"local": local}
        tokens = net.generate(n, u, initial_tokens=silence, temperature=temperature, top_k=top_k, top_p=top_p,
                              condition=condition, **lkw).cpu().numpy()
    else:
        tokens = _host_loop(net, silence, n, sampling_rate, generate_sec, temperature, top_k, top_p, condition, local)
    filename = _save(start_time, output_dir, Q, sampling_rate, [("generated", tokens)])[0]
    if report:
        write_report(report, [filename], [tokens], ranked, best_of, dists)
    return filename, tokens


def stream_job(args):
    """``generate --chunk-frames C [--ring-frames R]``: the checks, made before a model is built.  Returns (C or None, R or
    None)."""
    C, R = args.chunk_frames, args.ring_frames
    if C is None:
        if R is not None:
            raise SystemExit("generate: --ring-frames sizes the ring of a streamed run: give --chunk-frames C")
        return None, None
    if C < 1:
        raise SystemExit("generate: --chunk-frames C needs C >= 1, got {}".format(C))
    if R is not None and R < 1:
        raise SystemExit("generate: --ring-frames R needs R >= 1, got {}".format(R))
    if not args.fast:
        raise SystemExit("generate: --chunk-frames streams features to the decoder on the device: give --fast")
    if not args.local and not args.from_wav:
        raise SystemExit("generate: --chunk-frames streams the columns of a feature file: give --local FILE.npy")
    if args.utterances is not None or args.prompt or args.keep or args.local_dir is not None:
        raise SystemExit("generate: --chunk-frames vocodes one utterance from silence: --utterances, --prompt, --keep and "
                         "--local-dir do not go with it")
    return int(C), None if R is None else int(R)


class _ArrayColumns(object):
    """The columns of a feature array, handed out in order (``generate_streamed``'s source)."""

    def __init__(self, local):
        self.a = np.asarray(local, dtype=np.float32)
        self.total = int(self.a.shape[1])
        self.at = 0

    def take(self, k, host=False):
        out = self.a[:, self.at:self.at + k]
        self.at += int(out.shape[1])
        return out


class MelColumns(object):
    """The same interface over a recording: its tokens are fed to a streaming analyser (``features.LogMel.stream``) ``chunk_frames``
    hops at a time -- the look-ahead of win / 2 samples means a feed may complete fewer columns than it carries samples for --
    until ``take`` has its columns or the recording ends (``flush``); ``extra`` copies of the last column follow it, what
    ``local.with_extra_column`` appends to a file's array.  The columns are the one-shot call's, bit for bit."""

    def __init__(self, mel, tokens, quantization_steps, chunk_frames, extra=0, f0=None):
        """``mel``: a ``features.LogMel`` or an ``acoustic.MelPitch`` (``stream``, ``hop`` and the stream's ``_empty`` are all that is
        used); ``f0``: what ``f0_scale_job`` returned -- every chunk handed out goes through ``scaled_f0``."""
        self.f0 = f0
        self.an = mel.stream(quantization_steps)
        self.tokens = np.asarray(tokens, dtype=np.int32)
        self.step = int(chunk_frames) * mel.hop
        self.fed, self.extra, self.flushed = 0, int(extra), False
        self.total = features.frame_count(self.tokens.size, mel.hop) + self.extra
        self.have, self._last = [], None                # (F, k) device tensors not handed out yet; the last column made

    def _more(self):
        if self.fed < self.tokens.size:
            part = self.tokens[self.fed:self.fed + self.step]
            self.fed += part.size
            return self.an.feed(part)
        self.flushed = True
        out = self.an.flush()
        last = out[:, -1:] if out.shape[1] else self._last
        return torch.cat([out] + [last] * self.extra, dim=1) if self.extra else out

    def take(self, k, host=False):
        while sum(int(c.shape[1]) for c in self.have) < k and not self.flushed:
            got = self._more()
            if got.shape[1]:
                self._last = got[:, -1:]
                self.have.append(got)
        allc = torch.cat(self.have, dim=1) if self.have else self.an._empty()
        out, rest = allc[:, :k].contiguous(), allc[:, k:]
        self.have = [rest] if rest.shape[1] else []
        out = scaled_f0(out, self.f0)
        return out.cpu().numpy() if host else out


class _GrowingWav(object):
    """``generated.wav`` written chunk by chunk: the bytes ``data.save_audio_file`` writes for the same tokens (16-bit PCM, the
    mono signal in two channels), the header kept current after every chunk."""

    def __init__(self, filename, Q, sampling_rate):
        import wave
        self.Q = Q
        self.f = wave.open(filename, "wb")
        self.f.setnchannels(2)
        self.f.setsampwidth(2)
        self.f.setframerate(int(sampling_rate))

    def append(self, tokens):
        scale, dtype = data._pcm_format("16bit_pcm", True)
        s = data.mulaw_decode(np.asarray(tokens), self.Q, True) * scale
        self.f.writeframes(np.repeat(s.reshape((-1, 1)).astype(dtype), 2, axis=1).astype("<i2").tobytes())

    def close(self):
        self.f.close()


def generate_streamed(net, params, local, chunk_frames, ring_frames=None, generate_sec=1.0, output_dir="generated_audio",
                      temperature=1.0, top_k=0, top_p=1.0, condition=None, best_of=1, report=None, max_pull=4096):
    """``generate --chunk-frames C``: one utterance from silence through ``FasterWaveNet.open_stream``.  The stream is opened with
    the first max(C, columns of the window) columns of ``local`` and fed C more at a time; after every feed everything
    ``available()`` is pulled, ``max_pull`` samples at a time at most, and appended to ``generated.wav``.  Uniforms: the
    ``random_sample`` draws of the command without the flag, so with C >= the columns -- one projection over the same array --
    the file is the same, byte for byte.  ``best_of`` = K > 1: the K candidates are K utterances of the stream, ``chosen`` is
    collected per pull, and the file is written at the end, when the ranking is known.  ``local`` may be a ``MelColumns``
    (``--from-wav``): the columns are then made from the recording as the loop asks for them."""
    from ..faster_wavenet import stream_frames
    from ..wavenet import coarse_frames_needed
    Q, sr = params.quantization_steps, params.sampling_rate
    sampling.check_controls(temperature, top_k, top_p)
    n = int(sr * generate_sec) - 1
    K, want = int(best_of), best_of > 1 or bool(report)
    if n <= 0:
        if isinstance(local, MelColumns):
            local = local.take(local.total, host=True)
        return generate_audio(net, params, sr, generate_sec, True, output_dir, temperature, top_k, top_p, condition, local, best_of, report)
    silence = silence_window(Q, input_width_of(params))
    start_time = time.time()
    os.makedirs(output_dir, exist_ok=True)
    filename = "{}/generated.wav".format(output_dir)
    u = np.reshape(np.random.random_sample(n) if K == 1 else np.random.random_sample((K, n)), (K, n))
    src = local if isinstance(local, MelColumns) else _ArrayColumns(local)       # a feature array, or columns made as the audio arrives
    cols, C, U = src.total, int(chunk_frames), net.local_upsample
    # the window's own columns come with the call that opens the stream: the prefill reads them
    first = min(cols, max(C, coarse_frames_needed(len(silence), net.local_hop, U, 0, net.local_interp)))
    if ring_frames is None:            # one feed, and what the largest pull reads at once
        ring_frames = max(first, C) * U + stream_frames(net.local_fine_hop, net.local_interp == "linear", 0, pull=max_pull).min_ring
    wav = _GrowingWav(filename, Q, sr) if K == 1 else None
    toks, chosen, done, at = [], [], 0, first
    try:
        with net.open_stream(utterances=K, initial_tokens=silence, condition=condition, local=src.take(first, host=True),
                             temperature=temperature, top_k=top_k, top_p=top_p, return_chosen=want, ring_frames=ring_frames,
                             max_pull=max_pull) as st:
            while True:
                while done < n:
                    m = min(min(st.available()), n - done, max_pull)
                    if st.book.two_steps:                              # the nine-workgroup decoder runs two steps at least per launch:
                        if n - done - m == 1:                          # ... leave no single step for the end,
                            m -= 1
                        if st.book.steps_of(m) == 1:                   # ... and run none now (more rows are coming)
                            m -= 1
                    if m < 1:
                        break
                    got = st.pull(m, u[:, done:done + m])
                    t, c = got if want else (got, None)
                    t = t.cpu().numpy()
                    toks.append(t)
                    if c is not None:
                        chosen.append(c.cpu().numpy())
                    if wav is not None:
                        wav.append(t[0])
                    if not done:
                        print("first chunk ({} samples) after {:.3f} sec".format(m, time.time() - start_time))
                    done += m
                if done >= n or at >= cols:
                    break
                k = min(C, cols - at)
                part = src.take(k)
                st.push(part if K == 1 else [part] * K)
                at += k
    finally:
        if wav is not None:
            wav.close()
    if done < n:
        raise SystemExit("generate: the stream ended after {} of {} samples: what is left is a single decoder step, and the "
                         "nine-workgroup decoder runs two at least".format(done, n))
    tokens = np.concatenate(toks, axis=1)
    ranked = None
    if want:
        (kept,), ranked = _keep_best(list(tokens), list(np.concatenate(chosen, axis=1)), K)
    else:
        kept = tokens[0]
    print("\ndone in {:.3f} sec".format(time.time() - start_time))
    if wav is None:
        data.save_audio_file(filename, kept, Q, format="16bit_pcm", sampling_rate=sr)
    if report:
        write_report(report, [filename], [kept], ranked, K)
    return filename, kept


def from_wav_job(args, config, n_utt, chunk_frames, f0=None):
    """``generate --fast --from-wav FILE.wav``: every file read as training reads it and its log-mel features made on the device with
    the checkpoint's "mel" settings -> (one (F, frames) array per utterance, None), or with ``--chunk-frames`` (None, the streamed
    run's ``MelColumns``: nothing is computed yet, the column count follows from the file's length).  ``--resample``: the file is
    brought to the model's rate first, in one call also for a streamed run -- the silence trim needs the file's end.  Stops
    before a model is built when the checkpoint was not trained with ``train --local-mel``.  A checkpoint with "pitch": the
    analyser is ``acoustic.MelPitch`` (mel rows, then pitch channels); ``f0`` (``f0_scale_job``) is handed to the streamed source,
    the arrays of the one-shot path are scaled by the caller."""
    mel = _local.load_mel(args.model_dir)
    pitch = _local.load_pitch(args.model_dir)
    if mel is None:
        raise SystemExit("generate: --from-wav makes the features from the recording and needs a checkpoint trained with "
                         "train --local-mel ({} has no \"mel\")".format(os.path.join(args.model_dir, _local.FILE)))
    Q = _model.load_params(args.model_dir).quantization_steps
    distinct = {}
    with torch.cuda.device(args.gpu_device):
        for f in sorted(set(args.from_wav)):
            if not os.path.isfile(f):
                raise SystemExit("generate: --from-wav {} is missing".format(f))
            tokens, rate = data.load_audio_file(f, quantization_steps=Q, **read_kw(args, _model.load_params(args.model_dir)))
            if chunk_frames is not None:                 # streamed (one file): the analyser makes the columns as they are asked for
                extra = (1 if _local.load_interp(args.model_dir) == "linear" else 0) + (1 if _local.load_upsample(args.model_dir) > 1 else 0)
                return None, MelColumns(_local.feature_analyser(rate, config[0], config[1], mel["win"], pitch), tokens, Q, chunk_frames,
                                        extra, f0)
            distinct[f] = _local.mel_features(tokens, rate, config[0], config[1], mel["win"], Q, pitch=pitch)
    files = args.from_wav * n_utt if len(args.from_wav) == 1 else args.from_wav
    return [distinct[f] for f in files], None


def _wav_rate(path) -> int:
    """The sampling rate a .wav file's header states."""
    from scipy.io import wavfile
    return int(wavfile.read(path, mmap=True)[0])


def read_kw(args, params):
    """The keywords of ``data.load_audio_file`` that ``--resample`` adds: the model's rate, and the device that converts."""
    if not args.resample:
        return {}
    return dict(rate=int(params.sampling_rate), device="cuda:%d" % args.gpu_device)


def read_prompt(path, params, rkw={}):
    """The window a generation continues from: the file's tokens as training reads them (``data.load_audio_file``: mu-law,
    silence trimmed; ``rkw``, the keywords of ``read_kw``: at the model's rate), their last ``input_width``, left-padded with
    the silence token when the file is shorter."""
    Q = params.quantization_steps
    iw = input_width_of(params)
    tokens, _ = data.load_audio_file(path, quantization_steps=Q, **rkw)
    tokens = np.asarray(tokens, dtype=np.int32)[-iw:]
    return np.concatenate([silence_window(Q, iw - tokens.size), tokens])


def generate_utterances(net, params, prompt_files, sampling_rate=48000, generate_sec=1.0, fast=False, output_dir="generated_audio",
                        temperature=1.0, top_k=0, top_p=1.0, conditions=None, locals_=None, best_of=1, report=None, rkw={},
                        rank=None, fold=None):
    """``len(prompt_files)`` utterances, utterance u continuing ``prompt_files[u]`` (None: silence), written to
    ``generated_000.wav`` ...; with ``fast`` one ``generate_batch`` run, otherwise the host loop per utterance.
    ``best_of`` = K > 1 (``fast`` only): N * K candidates in that run, row ``u * K + c`` candidate c of utterance u, the
    most likely one of every utterance written under the utterance's name; ``report``: ``write_report``'s file; ``rank``: None or a
    ``MelRank`` (the candidate closest to its recording's columns is written instead); ``fold``: None or what ``fold_job``
    returned (``generate_folded_files`` with the uniforms drawn here without it)."""
    Q = params.quantization_steps
    sampling.check_controls(temperature, top_k, top_p)
    N = len(prompt_files)
    n = int(sampling_rate * generate_sec) - 1
    silence = silence_window(Q, input_width_of(params))
    read = {f: read_prompt(f, params, rkw) for f in set(prompt_files) if f is not None}
    prompts = np.stack([silence if f is None else read[f] for f in prompt_files])
    if fold is not None and n > 0:
        return generate_folded_files(net, params, ["generated_{:03d}".format(i) for i in range(N)], [n] * N,
                                     list(np.random.random_sample((N, n))), list(prompts), locals_, conditions, fold, output_dir,
                                     temperature, top_k, top_p, report)
    start_time = time.time()
    ranked = dists = None
    if fast and (best_of > 1 or report or rank is not None):
        K = best_of
        if n <= 0:
            rows, chosen = [np.zeros((0,), np.int32)] * (N * K), [np.zeros((0,), np.float32)] * (N * K)
        else:
            u = np.random.random_sample((N * K, n))
            lkw = {} if locals_ is None else {"local": [f for f in locals_ for _ in range(K)]}
            rows, chosen = net.generate_batch(n, u, initial_tokens=np.repeat(prompts, K, axis=0), temperature=temperature,
                                              top_k=top_k, top_p=top_p, return_chosen=True,
                                              condition=None if conditions is None else [c for c in conditions for _ in range(K)],
                                              **lkw)
        if rank is None:
            tokens, ranked = _keep_best(list(rows), list(chosen), K)
        else:
            tokens, ranked, dists = rank.keep_best(list(rows), list(chosen), K)
        tokens = np.stack(tokens)
    elif n <= 0:
        tokens = np.zeros((N, 0), np.int32)
    elif fast:
        u = np.random.random_sample((N, n))
        lkw = {} if locals_ is None else {"local": list(locals_)}
        tokens = net.generate_batch(n, u, initial_tokens=prompts, temperature=temperature, top_k=top_k, top_p=top_p,
                                    condition=conditions, **lkw).cpu().numpy()
    else:
        tokens = np.stack([_host_loop(net, prompts[i], n, sampling_rate, generate_sec, temperature, top_k, top_p,
                                      None if conditions is None else conditions[i],
                                      None if locals_ is None else locals_[i]) for i in range(N)])
    filenames = _save(start_time, output_dir, Q, sampling_rate, [("generated_{:03d}".format(i), tokens[i]) for i in range(N)])
    if report:
        write_report(report, filenames, list(tokens), ranked, best_of, dists)
    return filenames, tokens


def directory_job(args, seconds_given, f0=None):
    """``generate --fast --local-dir FEAT_DIR``: every check that needs no model, made before one is built.  Returns
    (names, features as the network takes them, samples to emit per file, class id per file or None)."""
    what = "generate --local-dir"
    if not args.fast:
        raise SystemExit("{}: vocoding a directory is one batched run on the device: give --fast".format(what))
    if args.utterances is not None or args.prompt or args.speaker:
        raise SystemExit("{}: one utterance per feature file, from silence, labelled by its file name: --utterances, --prompt "
                         "and --speaker do not go with it".format(what))
    config = _local.load_config(args.model_dir)
    _local.require_match(config, True, "generate", "--local-dir FEAT_DIR")
    names = _local.directory_features(args.local_dir)
    # a speaker-conditioned checkpoint labels every file by its name, as evaluate does; an unknown label stops here
    table = _speakers.load_table(args.model_dir)
    cids = [_speakers.class_id(table[0], _speakers.speaker_label(name), name + ".npy") for name in names] if table else None
    params = _model.load_params(args.model_dir)
    iw = input_width_of(params)
    cap = int(params.sampling_rate * args.seconds) - 1 if seconds_given else None
    if cap is not None and cap < 1:
        raise SystemExit("{}: -s {} asks for {} samples".format(what, args.seconds, cap))
    interp, upsample = _local.load_interp(args.model_dir), _local.load_upsample(args.model_dir)
    feats, lengths = [], []
    for name in names:
        f = _local.read_features(os.path.join(args.local_dir, name + ".npy"), config[0])
        # the rule of one --local file without -s, per file: what the features cover behind the window; -s caps it
        cover = _local.samples_covered(f.shape[1], config[1], iw)
        if cover < 1:
            raise SystemExit("generate: the features of {}.npy cover {} samples, fewer than the {} of the window".format(
                name, cover + iw - 1, iw))
        lengths.append(cover if cap is None else min(cover, cap))
        feats.append(_local.with_extra_column(scaled_f0(f, f0), interp, upsample))
    return names, feats, lengths, cids


def generate_directory(net, params, names, feats, lengths, cids, seed=None, output_dir="generated_audio", temperature=1.0,
                       top_k=0, top_p=1.0, best_of=1, report=None, fold=None):
    """One ragged ``generate_batch`` run over the whole directory, from silence; ``<output_dir>/NAME.wav`` per feature file,
    each at its own length.  With a seed every file draws what its own ``generate --fast --local NAME.npy`` run draws.
    ``best_of`` = K > 1: K candidates per file in that run (``random_sample((K, n_file))`` behind the file's seed), the most
    likely one written; ``report``: ``write_report``'s file."""
    Q = params.quantization_steps
    sampling.check_controls(temperature, top_k, top_p)
    silence = silence_window(Q, input_width_of(params))
    uniforms = []
    for n in lengths:
        if seed is not None:
            np.random.seed(seed)
        uniforms.append(np.random.random_sample(n) if best_of == 1 else np.random.random_sample((best_of, n)))
    if fold is not None:                   # (``fold_job``'s answer: the same files and uniforms, every file cut into segments)
        return generate_folded_files(net, params, names, lengths, uniforms, [silence] * len(names), feats, cids, fold, output_dir,
                                     temperature, top_k, top_p, report)
    start_time = time.time()
    if best_of == 1 and not report:
        rows = net.generate_batch(list(lengths), uniforms, initial_tokens=silence, temperature=temperature, top_k=top_k, top_p=top_p,
                                  condition=cids, local=list(feats))
        tokens = [r.cpu().numpy() for r in rows]
        return _save(start_time, output_dir, Q, params.sampling_rate, list(zip(names, tokens))), tokens
    K = best_of
    rows, chosen = net.generate_batch([n for n in lengths for _ in range(K)], [r for u in uniforms for r in np.reshape(u, (K, -1))],
                                      initial_tokens=silence, temperature=temperature, top_k=top_k, top_p=top_p,
                                      condition=None if cids is None else [c for c in cids for _ in range(K)],
                                      local=[f for f in feats for _ in range(K)], return_chosen=True)
    tokens, ranked = _keep_best(rows, chosen, K)
    filenames = _save(start_time, output_dir, Q, params.sampling_rate, list(zip(names, tokens)))
    if report:
        write_report(report, filenames, tokens, ranked, K)
    return filenames, tokens


def parse_redraw(text):
    """``--redraw A:B`` -> (A, B) in seconds; SystemExit for anything malformed, empty or with A >= B."""
    parts = str(text).split(":")
    try:
        a, b = (float(v) for v in parts) if len(parts) == 2 else (None, None)
    except ValueError:
        a = b = None
    if a is None or not (math.isfinite(a) and math.isfinite(b)) or a < 0.0:
        raise SystemExit("generate: --redraw takes A:B, two times in seconds of the kept file, got {!r}".format(text))
    if a >= b:
        raise SystemExit("generate: --redraw {} is empty: A:B needs A < B".format(text))
    return a, b


def keep_mask(M, W, ranges, sr):
    """The forced template of a kept file of ``M`` samples behind a window of ``W``: an int32 array over the ``M - W`` emitted
    positions (position i is file sample ``W + i``), 0 where the file's sample is kept and -1 where a range redraws it.
    ``ranges``: (A, B) pairs in seconds; each covers samples ``[round(A sr), round(B sr))``, cut off at M; ranges may touch or
    overlap.  A range that starts inside the window stops with the earliest time that can be redrawn."""
    template = np.zeros((max(int(M) - int(W), 0),), dtype=np.int32)
    for a, b in ranges:
        lo, hi = int(round(a * sr)), min(int(round(b * sr)), int(M))
        if lo < W:
            raise SystemExit("generate: --redraw {:g}:{:g} starts at sample {} of the file, inside the window of {} samples that "
                             "seeds the run: the earliest time that can be redrawn is {:.6f} s".format(a, b, lo, W, W / float(sr)))
        if hi > lo:
            template[lo - W:hi - W] = -1
    return template


def keep_job(args, seconds_given):
    """``generate --keep FILE.wav [--redraw A:B ...]``: every check, made before a model is built.  Returns None without
    ``--keep``, else (kept file of each utterance, its tokens, its forced array over the emitted positions, single) --
    ``single``: one utterance written as ``generated.wav``."""
    if args.redraw and not args.keep:
        raise SystemExit("generate: --redraw A:B says what to draw anew of a kept recording: give --keep FILE.wav")
    if not args.keep:
        return None
    if not args.fast:
        raise SystemExit("generate: --keep hands the kept samples to the decoder on the device: give --fast")
    if args.prompt or seconds_given or args.local_dir is not None:
        raise SystemExit("generate: --keep takes the window, the length and the samples from the kept file: --prompt, -s and "
                         "--local-dir do not go with it")
    ranges = [parse_redraw(r) for r in (args.redraw or [])]
    n_utt, files = _args.kept_files(args)
    params = _model.load_params(args.model_dir)
    Q, W, sr = params.quantization_steps, input_width_of(params), params.sampling_rate
    read = {}
    for f in files:
        if f not in read:
            t = np.asarray(data.load_audio_file(f, quantization_steps=Q, **read_kw(args, params))[0], dtype=np.int32)
            if t.size < W + 2:
                raise SystemExit("generate: --keep {} holds {} samples as training reads it; the window takes {} and the decoder "
                                 "runs two more at least: {} are needed".format(f, t.size, W, W + 2))
            template = keep_mask(t.size, W, ranges, sr)
            read[f] = (t, np.where(template < 0, -1, t[W:]).astype(np.int32))
    return files, [read[f][0] for f in files], [read[f][1] for f in files], args.utterances is None and len(files) == 1


def generate_kept(net, params, files, tokens, forced, single, output_dir="generated_audio", temperature=1.0, top_k=0, top_p=1.0,
                  conditions=None, locals_=None, best_of=1, report=None):
    """One ``generate_batch`` run over the kept files: utterance u starts from its file's first ``input_width`` samples, emits
    ``forced[u]`` where that is a token and draws where it is -1, and is written as those samples followed by what was emitted --
    the file, with the ``--redraw`` ranges regenerated.  Uniforms: utterance after utterance, ``random_sample((K, n_u))``, row c
    candidate c's.  ``best_of`` = K > 1: rows ``u * K + c`` of the run; the figure ranked on (and reported) is over all ``n_u``
    emitted samples, kept ones included."""
    Q, W, K = params.quantization_steps, input_width_of(params), best_of
    sampling.check_controls(temperature, top_k, top_p)
    lengths = [len(f) for f in forced]
    uniforms = [row for n in lengths for row in np.random.random_sample((K, n))]
    start_time = time.time()
    rep_k = lambda xs: [x for x in xs for _ in range(K)]
    lkw = {} if locals_ is None else {"local": rep_k(locals_)}
    want = K > 1 or bool(report)
    got = net.generate_batch(rep_k(lengths), uniforms, initial_tokens=np.stack(rep_k([t[:W] for t in tokens])),
                             temperature=temperature, top_k=top_k, top_p=top_p, condition=None if conditions is None else rep_k(conditions),
                             return_chosen=want, forced=rep_k(forced), **lkw)
    ranked = None
    if want:
        emitted, ranked = _keep_best(list(got[0]), list(got[1]), K)
    else:
        emitted = [r.cpu().numpy() for r in got]
    whole = [np.concatenate([t[:W], e.astype(np.int32)]) for t, e in zip(tokens, emitted)]
    names = ["generated"] if single else ["generated_{:03d}".format(i) for i in range(len(files))]
    filenames = _save(start_time, output_dir, Q, params.sampling_rate, list(zip(names, whole)))
    if report:
        write_report(report, filenames, emitted, ranked, K)
    return (filenames[0], whole[0]) if single else (filenames, whole)


def _seconds_given(argv) -> bool:
    """Whether the command line names -s / --seconds (its default, 1.0, is a length like any other when it is given)."""
    import argparse
    import sys as _sys
    probe = argparse.ArgumentParser(add_help=False)
    probe.add_argument("-s", "--seconds", type=float, default=None)
    return probe.parse_known_args(_sys.argv[1:] if argv is None else list(argv))[0].seconds is not None


def main(argv=None):
    args = _args.parse(argv)
    if args.gpus != 1:
        raise SystemExit("generate: --gpus {} belongs to train and evaluate; generation runs on one device".format(args.gpus))
    best_of, report = likelihood_job(args)
    chunk_frames, ring_frames = stream_job(args)
    tile = tile_job(args)
    fold = fold_job(args)
    rank_mel = rank_job(args)
    f0 = f0_scale_job(args)
    seconds_given = _seconds_given(argv)
    kept = keep_job(args, seconds_given)
    if args.local_dir is not None:
        names, feats, lengths, cids = directory_job(args, seconds_given, f0)
        params, net = _model.build(args)
        if tile is not None:
            net.batch_tile = tile
        return generate_directory(net, params, names, feats, lengths, cids, seed=args.seed, output_dir=args.output_dir,
                                  temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, best_of=best_of, report=report,
                                  fold=fold)
    n_utt, prompt_files = _args.utterance_prompts(args)
    if kept is not None:
        n_utt = len(kept[0])
    # the speaker of every utterance, checked against the checkpoint's table before the model is built: an unknown label,
    # --speaker on an unconditioned checkpoint and its absence on a conditioned one all stop here with a clear message
    table = _speakers.load_table(args.model_dir)
    names = _speakers.utterance_speakers(args.speaker, n_utt or 1)
    cids = [_speakers.class_id(table[0] if table else None, s, "generate") for s in names]
    # features: checked against the checkpoint's local.json before the model is built, like the speakers
    config = _local.load_config(args.model_dir)
    _local.require_match(config, bool(args.local) or bool(args.from_wav), "generate",
                         "--from-wav FILE.wav" if args.from_wav else "--local FILE.npy")
    feats, mel_src = None, None
    if args.from_wav:
        feats, mel_src = from_wav_job(args, config, n_utt or 1, chunk_frames, f0)
    elif config is not None:
        distinct = {f: _local.read_features(f, config[0]) for f in set(args.local)}
        feats = [distinct[f] for f in (args.local * (n_utt or 1) if len(args.local) == 1 else args.local)]
    mels = _local.mel_count(args.model_dir)              # (pitch channels behind the mel rows are no part of a mel distance)
    targets = [f[:mels] for f in feats] if rank_mel else None         # the recordings' own columns, one array per utterance
    if feats is not None:
        feats = [scaled_f0(f, f0) for f in feats]
    params, net = _model.build(args)
    if tile is not None:               # every generate_batch / open_stream call of this run decodes in tiles
        net.batch_tile = tile
    rank = None
    if rank_mel:
        win = _local.load_mel(args.model_dir)["win"]
        files = args.from_wav * len(targets) if len(args.from_wav) == 1 else args.from_wav

        def analyser_of(rate):
            with torch.cuda.device(args.gpu_device):
                return _local.mel_analyser(rate, mels, config[1], win)

        rank = MelRank(analyser_of, [int(params.sampling_rate) if args.resample else _wav_rate(f) for f in files], targets,
                       params.quantization_steps, silence_window(params, input_width_of(params)))
    np.random.seed(args.seed)
    if feats is not None or mel_src is not None:
        # the features cover an utterance from its first sample, the window of input_width samples included; the length
        # generated defaults to what they cover (-s left at its default), and more than that is refused before anything runs
        iw = input_width_of(params)
        columns = [f.shape[1] for f in feats] if mel_src is None else [mel_src.total - mel_src.extra]
        cover = min(columns) * config[1] - iw + 1                            # samples that can be emitted
        # (linear interpolation: the column behind the last is the driver's to supply -- the file's last one again -- so n
        # columns still give n * hop samples)
        # (a learned upsampling layer reads pairs of columns: one more copy of the last, likewise)
        if feats is not None:
            feats = [_local.with_extra_column(f, _local.load_interp(args.model_dir), _local.load_upsample(args.model_dir)) for f in feats]
        if cover < 1:
            raise SystemExit("generate: the features cover {} samples, fewer than the {} of the window".format(cover + iw - 1, iw))
        if kept is not None:
            short = [f for f, fd in zip(kept[0], kept[2]) if len(fd) > cover]
            if short:
                raise SystemExit("generate: --keep {} emits {} samples behind its window, the features cover {}".format(
                    short[0], max(len(fd) for fd in kept[2]), cover))
        elif not seconds_given:
            args.seconds = (cover + 1.5) / float(params.sampling_rate)            # int(rate * seconds) - 1 == cover
        elif int(params.sampling_rate * args.seconds) - 1 > cover:
            raise SystemExit("generate: -s {} asks for {} samples, the features cover {}".format(
                args.seconds, int(params.sampling_rate * args.seconds) - 1, cover))
    if kept is not None:
        return generate_kept(net, params, *kept, output_dir=args.output_dir, temperature=args.temperature, top_k=args.top_k,
                             top_p=args.top_p, conditions=cids if table else None, locals_=feats, best_of=best_of, report=report)
    if chunk_frames is not None:
        return generate_streamed(net, params, mel_src if mel_src is not None else feats[0], chunk_frames, ring_frames, generate_sec=args.seconds, output_dir=args.output_dir,
                                 temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, condition=cids[0],
                                 best_of=best_of, report=report)
    if n_utt is not None:
        return generate_utterances(net, params, prompt_files, sampling_rate=params.sampling_rate, generate_sec=args.seconds,
                                   fast=args.fast, output_dir=args.output_dir, temperature=args.temperature, top_k=args.top_k,
                                   top_p=args.top_p, conditions=cids if table else None, locals_=feats, best_of=best_of,
                                   report=report, rkw=read_kw(args, params), rank=rank, fold=fold)
    return generate_audio(net, params, sampling_rate=params.sampling_rate, generate_sec=args.seconds, fast=args.fast,
                          output_dir=args.output_dir, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                          condition=cids[0], local=None if feats is None else feats[0], best_of=best_of, report=report, rank=rank,
                          fold=fold)


if __name__ == "__main__":
    main()
