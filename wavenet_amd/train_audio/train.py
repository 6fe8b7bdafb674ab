"""Training driver (train_audio/train.py:24-135): for every epoch, for every .wav file, ``repeat`` updates on random crops
of ``input_width + train_width`` samples with next-sample targets; checkpoint after every file and every epoch.

``--corpus`` (new): the files stay on the device (``wavenet_amd.corpus.Corpus``) and every batch is drawn uniformly over all
training windows of all files, so a batch mixes files and speakers; an epoch keeps its ``len(files) * repeat`` updates and its
checkpoints.  Both paths run the one update loop, ``run_updates``."""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

from .. import TrainStepGraph, data
from ..corpus import Corpus, check_shard, columns_per_crop
from ..graph import default_loss
from ..wavenet import coarse_frames_needed
from . import args as _args
from . import model as _model
from .evaluate import evaluate_dir
from . import launch as _launch
from . import local as _local
from . import speakers as _speakers


HEALTH_EVERY = 100      # updates between two reads of WaveNet.last_update_applied() (a host synchronisation each)


def input_width_of(params) -> int:
    """train.py:36-44: receptive field of the residual stack plus one column per causal layer."""
    per_block = params.residual_conv_filter_width ** len(params.residual_conv_channels)
    return (per_block - 1) * params.residual_num_blocks + 1 + len(params.causal_conv_channels)


class _Crops(object):
    """train.py:14-22 with the signal resident on the device: the start offsets are drawn on the host from numpy's
    global generator (the draw the reference makes, so ``--seed`` selects the same crops), the gather runs on the GPU."""

    def __init__(self, signal: np.ndarray, input_width: int, target_width: int, device, features=None, hop=0, shift=0,
                 extra_column=False, crop="frame", columns=None):
        """``features`` (F, columns) on the grid ``local.padded`` describes (index into ``signal`` + ``shift`` = position,
        position // hop = column): starts are then drawn so that every crop begins on a column border (phase 0), and ``draw``
        also returns the crops' (B, F, ceil((input_width + target_width) / hop)) columns -- one more with ``extra_column``
        (linear interpolation; ``features`` then ends with the repeated last column of ``local.with_extra_column``).
        ``crop="sample"`` (``--local-crop sample``): starts are drawn as they are without features -- any sample, the very
        ``np.random.randint`` call, so one ``--seed`` selects the same crops with and without features -- and ``draw`` also
        returns every crop's phase (start + shift) % hop; the columns run from (start + shift) // hop on and there are as
        many as the worst phase needs, ceil((input_width + target_width + hop - 1) / hop) (one more with ``extra_column``),
        the file's last column repeated where that runs past the file.  ``columns``: the column count itself, when another
        rule gives it (a learned upsampling layer: ``coarse_frames_needed``)."""
        if crop not in ("frame", "sample"):
            raise Exception("crop must be 'frame' or 'sample', got %r" % (crop,))
        self.hop, self.shift, self.crop = int(hop), int(shift), crop
        self.features = None
        if features is not None:
            self.features = torch.as_tensor(features).to(device)
            worst = hop - 1 if crop == "sample" else 0
            ncol = (input_width + target_width + worst + hop - 1) // hop + int(extra_column)
            self.fcol = torch.arange(ncol if columns is None else int(columns), device=device)
        self.n = int(signal.size)
        self.iw, self.tw = input_width, target_width
        if self.n - target_width - input_width - 1 <= 0:
            raise Exception("signal too short for input_width + train_width")
        self.signal = torch.as_tensor(signal.astype(np.int32)).to(device)
        self.col = torch.arange(input_width + target_width + 1, device=device)
        self.last_draw = None

    def draw(self, batch_size: int, shard=None):
        """``shard`` = (lo, hi), a rank of a data-parallel run: the ``randint`` call is the global one all the same --
        ``batch_size`` starts, all of them kept in ``last_draw`` -- and crops lo .. hi - 1 of it are gathered."""
        hi = self.n - self.tw - self.iw - 1
        feats = None
        phases = None

        def mine(drawn):
            self.last_draw = drawn
            if shard is None:
                return drawn
            lo, up = check_shard(shard, batch_size)
            return drawn[lo:up]
        if self.features is None:
            starts = mine(np.random.randint(0, hi, size=batch_size))
        elif self.crop == "sample":
            starts = mine(np.random.randint(0, hi, size=batch_size))  # the feature-less draw: same seed, same crops
            pos = starts + self.shift
            phases = (pos % self.hop).astype(np.int32)
            first = torch.as_tensor(pos // self.hop).to(self.col.device)
            # the worst-case column count may run past the file's columns: the last one is repeated, never an index beyond
            cols = torch.clamp(first[:, None] + self.fcol[None, :], max=int(self.features.shape[1]) - 1)
            feats = self.features[:, cols].permute(1, 0, 2).contiguous()
        else:
            # starts r, r + hop, r + 2 hop, ... below hi, r the first index whose position is a multiple of the hop: one draw,
            # as above
            r = (-self.shift) % self.hop
            if hi - r <= 0:
                raise Exception("signal too short for a crop that starts on a feature column")
            starts = mine(r + self.hop * np.random.randint(0, (hi - r + self.hop - 1) // self.hop, size=batch_size))
            first = torch.as_tensor((starts + self.shift) // self.hop).to(self.col.device)
            feats = self.features[:, first[:, None] + self.fcol[None, :]].permute(1, 0, 2).contiguous()
        idx = torch.as_tensor(starts).to(self.col.device)[:, None] + self.col[None, :]
        win = self.signal[idx]                                     # (B, iw + tw + 1)
        x, tgt = win[:, :self.iw + self.tw].contiguous(), win[:, self.iw + 1:].contiguous()
        if phases is not None:
            return x, tgt, feats, phases
        return (x, tgt) if self.features is None else (x, tgt, feats)


def read_file(path, params, device=None, resample=False):
    """(tokens, rate) of a .wav file as training reads it; ``resample``: brought to the model's sampling_rate on ``device``
    first (``--resample``), and that rate is the one returned."""
    if not resample:
        return data.load_audio_file(path, quantization_steps=params.quantization_steps)
    return data.load_audio_file(path, quantization_steps=params.quantization_steps, rate=int(params.sampling_rate), device=device)


def train_audio(net, params, path_to_file, batch_size=16, train_width=16, repeat=1000, use_graph=True, state=None,
                local_dir=None, local_crop="frame", local_mel=None, resample=False):
    """One file: returns the summed loss of its ``repeat`` updates (train.py:24-90).  ``local_dir``: where the file's feature
    file lies (a locally conditioned model); crops then start on a feature column border (``local_crop="frame"``) or at any
    sample, each with its own phase (``"sample"``: the crops a run without features draws).  ``local_mel`` ({"win": W},
    ``--local-mel``): no feature file -- the log-mel features of the file's tokens, made on the device here, once per call;
    from there on the array takes the feature file's path.  ``resample``: the file is read at the model's rate (``read_file``)."""
    signals, rate = read_file(path_to_file, params, net.device, resample)
    iw = input_width_of(params)
    silence = 127 if params.quantization_steps > 127 else params.quantization_steps // 2
    local = getattr(net, "local", None)
    _local.require_match(local, local_dir is not None or local_mel is not None, "train", "--local-dir FEAT_DIR or --local-mel")
    fkw = {}
    if local is not None:
        feats = _local.file_or_mel_features(local_dir, local_mel, path_to_file, signals, rate, local[0], local[1],
                                            params.quantization_steps)
        interp = getattr(net, "local_interp", "repeat")
        U = getattr(net, "local_upsample", 1)
        ext, shift = _local.padded(_local.with_extra_column(feats, interp, U), iw, local[1])
        fkw = dict(features=ext, hop=local[1], shift=shift, extra_column=interp == "linear", crop=local_crop)
        if U > 1:                                                  # the learned layer reads pairs of neighbouring columns
            fkw["columns"] = coarse_frames_needed(iw + train_width, local[1], U, None if local_crop == "sample" else 0, interp)
    signals = np.concatenate([np.full((iw,), silence, dtype=np.int32), signals.astype(np.int32)])   # train.py:53
    crops = _Crops(signals, iw, train_width, net.device, **fkw)
    # a conditioned model: every crop carries the label of the file it came from
    labels = getattr(net, "speakers", None)
    cond = None
    shard = rank_shard(net, batch_size)
    skw = {} if shard is None else {"shard": shard}
    if labels is not None:
        cid = _speakers.class_id(labels, _speakers.speaker_label(path_to_file), os.path.basename(path_to_file))
        cond = torch.full((batch_size if shard is None else shard[1] - shard[0],), cid, device=net.device, dtype=torch.int64)

    def draw():
        drawn = crops.draw(batch_size, **skw)
        lkw = {} if local is None else {"local": drawn[2]}
        if len(drawn) > 3:
            lkw["local_phase"] = drawn[3]                           # a phase per crop (--local-crop sample)
        return drawn[0], drawn[1], cond, lkw

    return run_updates(net, params, draw, repeat, (batch_size, iw + train_width), use_graph, state,
                       os.path.basename(path_to_file), signals.size)


def run_updates(net, params, draw, repeat, key, use_graph, state, name, width):
    """``repeat`` updates, each on the batch ``draw()`` hands back -- (x, tgt, condition or None, the ``local=`` /
    ``local_phase=`` keywords of the step) -- through the replayed graph of shape ``key`` (kept in ``state``) or op by op;
    returns their summed loss.  ``name`` and ``width`` are what the progress line says of the source.  The one update loop of
    the per-file path (``train_audio``) and of the corpus path (``train_corpus``).  On a data-parallel network ``draw()`` hands
    back this rank's shard of each global batch, and the sum returned is the global batch's, the same on every rank."""
    sum_loss = torch.zeros((), device=net.device, dtype=torch.float64)
    graph = None
    skipped = 0
    for batch_index in range(repeat):
        x, tgt, cond, lkw = draw()
        if use_graph and str(params.optimizer).lower() != "eve":     # Eve needs the loss on the host every update
            graph = None if state is None else state.get(key)
            if graph is None:
                graph = TrainStepGraph(net, x, tgt, condition=cond, **lkw)
                if state is not None:
                    state[key] = graph
            loss = graph.step(x, tgt, condition=cond, **lkw)
        else:
            loss = default_loss(net, x, tgt, condition=cond, **lkw)
            net.backprop(loss)
            loss = loss.detach()
        sum_loss += loss                                            # on the device: no host sync per update
        # health check (one word read back, every HEALTH_EVERY updates and after the last one): a step whose gradient norm was
        # not finite is SKIPPED on the device (wn_adam_step, ABI 4) -- say so instead of training on in silence.  The guard
        # lives in the clipping hook: with gradient_clipping <= 0 there is no norm and nothing is ever skipped.
        if (batch_index % HEALTH_EVERY == HEALTH_EVERY - 1 or batch_index == repeat - 1) and not net.last_update_applied():
            skipped += 1
            sys.stdout.write("\n\twarning: update {} of {} was skipped on the device (gradient norm not finite; loss {}); "
                             "{} such checks failed so far\n".format(batch_index, name, float(loss), skipped))
            if skipped >= 5:
                raise Exception("the gradient norm was not finite at {} consecutive health checks: the run is doing no work "
                                "(lower --lr, or set exec_flags |= WN_EXEC_NO_MULTI_LAYER_BWD if another process shares the "
                                "GPU)".format(skipped))
        elif batch_index % HEALTH_EVERY == HEALTH_EVERY - 1:
            skipped = 0
        if batch_index % 10 == 0:
            sys.stdout.write("\r\t{} - {} width; {}/{}".format(name, width, batch_index, repeat))
            sys.stdout.flush()
    total = float(sum_loss.item())
    # data parallel: every rank summed the losses of its own shards; one mean over ranks per call, none per update
    return total if net._dp_group is None else net._dp_group.mean_loss(total)


def rank_shard(net, batch_size):
    """The crops [lo, hi) of a global batch that this process trains on: None without data parallelism
    (``WaveNet.enable_data_parallel``), else ``dp.shard``'s equal share -- a batch that does not divide by the ranks stops."""
    return None if net._dp_group is None else net._dp_group.shard(batch_size)


def load_corpus(net, params, wav_dir, files, local_dir=None, local_mel=None, resample=False):
    """``--corpus``: every .wav file of ``files`` loaded once -- its tokens, its features (the feature file of ``local_dir``, or
    the log-mel of its own tokens made on the device, up to 64 files per launch: the bits of the single calls) and its
    speaker's class id -- packed into a ``Corpus`` on the network's device.  ``resample``: the files are read at the model's rate,
    converted on the device 64 per launch (``data.load_audio_files``)."""
    local = getattr(net, "local", None)
    _local.require_match(local, local_dir is not None or local_mel is not None, "train", "--local-dir FEAT_DIR or --local-mel")
    paths = [os.path.join(wav_dir, fn) for fn in files]
    if resample:
        rate = int(params.sampling_rate)
        loaded = [(t, rate) for t in data.load_audio_files(paths, rate, params.quantization_steps, net.device)]
    else:
        loaded = [data.load_audio_file(p, quantization_steps=params.quantization_steps) for p in paths]
    tokens, rates = [t.astype(np.int32) for t, _ in loaded], [r for _, r in loaded]
    feats = None
    if local is not None and local_dir is not None:
        feats = [_local.file_features(local_dir, fn, t.size, local[0], local[1]) for fn, t in zip(files, tokens)]
    elif local is not None:
        feats = _local.mel_features_of_files(tokens, rates, local[0], local[1], local_mel["win"], params.quantization_steps,
                                             pitch=local_mel.get("pitch"))
    labels = getattr(net, "speakers", None)
    classes = None if labels is None else [_speakers.class_id(labels, _speakers.speaker_label(fn), fn) for fn in files]
    return Corpus(tokens, input_width_of(params), params.quantization_steps, net.device, features=feats,
                  hop=local[1] if local is not None else 0, classes=classes)


def train_corpus(net, params, corpus, batch_size=16, train_width=16, repeat=1000, use_graph=True, state=None,
                 local_crop="frame"):
    """``repeat`` updates on batches drawn uniformly over all training windows of the corpus, every crop with its own file's
    class id, feature columns and phase; returns their summed loss.  The rules are ``train_audio``'s: the column count per
    crop, the int phase 0 of ``local_crop="frame"`` against one phase per crop (``"sample"``), the graph kept by shape."""
    iw = corpus.input_width
    n_cols = None
    if corpus.features is not None:
        n_cols = columns_per_crop(iw, train_width, corpus.hop, local_crop, getattr(net, "local_interp", "repeat"),
                                  getattr(net, "local_upsample", 1))

    shard = rank_shard(net, batch_size)
    skw = {} if shard is None else {"shard": shard}

    def draw():
        x, tgt, feats, cond, phases = corpus.draw(batch_size, train_width, local_crop, n_cols, **skw)
        lkw = {} if feats is None else {"local": feats}
        if feats is not None and local_crop == "sample":
            lkw["local_phase"] = phases
        return x, tgt, cond, lkw

    return run_updates(net, params, draw, repeat, (batch_size, iw + train_width), use_graph, state, "corpus",
                       int(corpus.tokens.size))


def validate(net, params, wav_dir, epoch, local_dir=None, local_mel=None, resample=False, shard=None):
    """The held-out negative log-likelihood after an epoch: one line for the weights being trained and, when a weight
    average is kept, one for the averaged weights.  ``shard`` = (rank, world): the held-out files are scored by the ranks in
    turn (``evaluate_dir``); every rank forms both lines."""
    skw = {} if shard is None else {"shard": shard}

    def line(what, total):
        sys.stdout.write("epoch: {} - held-out {}: {:.6f} nats/sample  {:.6f} bits/sample  ({} samples)\n".format(
            epoch, what, total["nats_per_sample"], total["bits_per_sample"], total["samples"]))
    line("weights", evaluate_dir(net, params, wav_dir, verbose=False, local_dir=local_dir, local_mel=local_mel, resample=resample, **skw)["total"])
    if net.ema_enabled:
        with net.ema_weights():
            line("ema weights", evaluate_dir(net, params, wav_dir, verbose=False, local_dir=local_dir, local_mel=local_mel, resample=resample, **skw)["total"])
    sys.stdout.flush()


def main(argv=None):
    args = _args.parse(argv)
    if args.ema:
        raise Exception("--ema belongs to generate and evaluate; train keeps an average with --ema-decay")
    if args.corpus:
        if args.batch_size < 1 or args.train_width < 1 or args.repeat < 1:
            raise SystemExit("train --corpus: --batch-size, --train-width and --repeat must be at least 1, got {}, {} and {}".format(
                args.batch_size, args.train_width, args.repeat))
        if not os.path.isdir(args.wav_dir) or not any(fn.endswith(".wav") for fn in os.listdir(args.wav_dir)):
            raise SystemExit("train --corpus: no .wav file in {}".format(args.wav_dir))
    if args.f0_scale != 1.0:
        raise SystemExit("train: --f0-scale belongs to generate")
    if args.local_pitch:                                            # Pitch's refusals at the run's rate, hop and window, before a model is built
        _model.local_pitch_settings(args, _model.load_params(args.model_dir))
    if args.gpus > 1:
        # --gpus N: this process checks, starts the N ranks of this very command line as a child (train_audio/launch.py) and
        # hands their exit code on; it builds no model and touches no device.  A rank finds WORLD_SIZE set and trains
        try:
            _launch.check_batch(args.batch_size, args.gpus)
        except ValueError as e:
            raise SystemExit("train: {}".format(e))
        if not _launch.in_rank():
            code = _launch.run("wavenet_amd.train_audio.train", sys.argv[1:] if argv is None else list(argv), args.gpus)
            if code:
                raise SystemExit(code)
            return None
    rank, world = _launch.join(args)                                # before a model is built; (0, 1) without --gpus
    with _launch.rank_stdout(rank):                                 # rank 0 alone prints
        average_loss = train(args, rank, world)
    _launch.leave(world)                                            # a barrier precedes exit
    return average_loss


def train(args, rank=0, world=1):
    """The run of one process: all of it without ``--gpus``, one rank of ``world`` with it (``launch.join`` has been called).  The
    ranks make the same draws from one seed and each gathers its shard (``rank_shard``); rank 0 alone writes files."""
    args.seed = _launch.shared_seed(args.seed, rank, world)
    params, net = _launch.build_in_turn(lambda: _model.build(args, train=True), rank, world)
    if world > 1:
        net.enable_data_parallel()                                  # rank 0's weights, optimiser state and weight average
    _local.require_match(net.local, args.local_dir is not None or args.local_mel, "train", "--local-dir FEAT_DIR or --local-mel")
    # (--local-dir on such a checkpoint: the feature files win); a "pitch" entry rides inside: mel rows, then pitch channels
    local_mel = _local.analysis_settings(net.local_mel, getattr(net, "local_pitch", None)) if args.local_mel else None
    np.random.seed(args.seed)
    net.update_laerning_rate(args.lr)
    files = sorted(fn for fn in os.listdir(args.wav_dir) if fn.endswith(".wav"))
    for fn in files:
        print("loading", fn)
    iw = input_width_of(params)
    rf = iw - len(params.causal_conv_channels)
    print("receptive field width:", int(rf * 1000.0 / params.sampling_rate), "[millisecond]")
    print("receptive field width:", rf, "[step]")
    print("files: {} batch_size: {} train_width: {}".format(len(files), args.batch_size, args.train_width))
    if not files:
        raise Exception("no .wav file in {}".format(args.wav_dir))
    corpus = None
    if args.corpus:
        corpus = load_corpus(net, params, args.wav_dir, files, local_dir=args.local_dir, local_mel=local_mel,
                             resample=args.resample)
        counts = corpus.windows(args.train_width, args.local_crop or "frame")
        for fn, n, c in zip(files, corpus.file_len, counts):
            if c == 0:
                print("leaving out {}: its {} samples hold no crop of input_width + train_width".format(fn, int(n)))
        if int(counts.sum()) == 0:
            raise Exception("signal too short for input_width + train_width: no file of {} holds a crop".format(args.wav_dir))
        print("corpus: {} samples and {} training windows in {} files, {} bytes on the device".format(
            int(corpus.tokens.size), int(counts.sum()), int((counts > 0).sum()), corpus.device_bytes()))

    def save():
        if rank == 0:
            net.save(args.model_dir)
    vkw = {} if world == 1 else {"shard": (rank, world)}
    start_time = time.time()
    graphs = {}
    average_loss = None
    for epoch in range(1, args.max_epoch):                          # train.py:118: epochs 1 .. max_epoch - 1
        average_loss = 0.0
        for fn in files:
            if corpus is not None:                                  # as many updates, and checkpoints, as the per-file loop makes
                average_loss += train_corpus(net, params, corpus, batch_size=args.batch_size, train_width=args.train_width,
                                             repeat=args.repeat, use_graph=not args.no_graph, state=graphs,
                                             local_crop=args.local_crop or "frame")
                save()
                continue
            average_loss += train_audio(net, params, os.path.join(args.wav_dir, fn), batch_size=args.batch_size,
                                        train_width=args.train_width, repeat=args.repeat,
                                        use_graph=not args.no_graph, state=graphs, local_dir=args.local_dir,
                                        local_crop=args.local_crop or "frame", local_mel=local_mel, resample=args.resample)
            save()
        average_loss /= len(files)
        sys.stdout.write("\033[2K\repoch: {} - {:.4e} loss - {} min\n".format(
            epoch, average_loss, int((time.time() - start_time) / 60)))
        sys.stdout.flush()
        save()
        if args.valid_wav_dir:
            validate(net, params, args.valid_wav_dir, epoch, local_dir=args.local_dir, local_mel=local_mel, resample=args.resample,
                     **vkw)
    return average_loss


if __name__ == "__main__":
    main()
