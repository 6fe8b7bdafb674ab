"""Training driver (train_audio/train.py:24-135): for every epoch, for every .wav file, ``repeat`` updates on random crops
of ``input_width + train_width`` samples with next-sample targets; checkpoint after every file and every epoch."""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

from .. import TrainStepGraph, data
from ..graph import default_loss
from ..wavenet import coarse_frames_needed
from . import args as _args
from . import model as _model
from .evaluate import evaluate_dir
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

    def draw(self, batch_size: int):
        hi = self.n - self.tw - self.iw - 1
        feats = None
        phases = None
        if self.features is None:
            starts = np.random.randint(0, hi, size=batch_size)
        elif self.crop == "sample":
            starts = np.random.randint(0, hi, size=batch_size)        # the feature-less draw: same seed, same crops
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
            starts = r + self.hop * np.random.randint(0, (hi - r + self.hop - 1) // self.hop, size=batch_size)
            first = torch.as_tensor((starts + self.shift) // self.hop).to(self.col.device)
            feats = self.features[:, first[:, None] + self.fcol[None, :]].permute(1, 0, 2).contiguous()
        idx = torch.as_tensor(starts).to(self.col.device)[:, None] + self.col[None, :]
        win = self.signal[idx]                                     # (B, iw + tw + 1)
        x, tgt = win[:, :self.iw + self.tw].contiguous(), win[:, self.iw + 1:].contiguous()
        if phases is not None:
            return x, tgt, feats, phases
        return (x, tgt) if self.features is None else (x, tgt, feats)


def train_audio(net, params, path_to_file, batch_size=16, train_width=16, repeat=1000, use_graph=True, state=None,
                local_dir=None, local_crop="frame", local_mel=None):
    """One file: returns the summed loss of its ``repeat`` updates (train.py:24-90).  ``local_dir``: where the file's feature
    file lies (a locally conditioned model); crops then start on a feature column border (``local_crop="frame"``) or at any
    sample, each with its own phase (``"sample"``: the crops a run without features draws).  ``local_mel`` ({"win": W},
    ``--local-mel``): no feature file -- the log-mel features of the file's tokens, made on the device here, once per call;
    from there on the array takes the feature file's path."""
    signals, rate = data.load_audio_file(path_to_file, quantization_steps=params.quantization_steps)
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
    if labels is not None:
        cid = _speakers.class_id(labels, _speakers.speaker_label(path_to_file), os.path.basename(path_to_file))
        cond = torch.full((batch_size,), cid, device=net.device, dtype=torch.int64)
    sum_loss = torch.zeros((), device=net.device, dtype=torch.float64)
    graph = None
    skipped = 0
    name = os.path.basename(path_to_file)
    for batch_index in range(repeat):
        drawn = crops.draw(batch_size)
        x, tgt = drawn[0], drawn[1]
        lkw = {} if local is None else {"local": drawn[2]}
        if len(drawn) > 3:
            lkw["local_phase"] = drawn[3]                           # a phase per crop (--local-crop sample)
        if use_graph and str(params.optimizer).lower() != "eve":     # Eve needs the loss on the host every update
            key = (batch_size, iw + train_width)
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
            sys.stdout.write("\r\t{} - {} width; {}/{}".format(name, signals.size, batch_index, repeat))
            sys.stdout.flush()
    return float(sum_loss.item())


def validate(net, params, wav_dir, epoch, local_dir=None, local_mel=None):
    """The held-out negative log-likelihood after an epoch: one line for the weights being trained and, when a weight
    average is kept, one for the averaged weights."""
    def line(what, total):
        sys.stdout.write("epoch: {} - held-out {}: {:.6f} nats/sample  {:.6f} bits/sample  ({} samples)\n".format(
            epoch, what, total["nats_per_sample"], total["bits_per_sample"], total["samples"]))
    line("weights", evaluate_dir(net, params, wav_dir, verbose=False, local_dir=local_dir, local_mel=local_mel)["total"])
    if net.ema_enabled:
        with net.ema_weights():
            line("ema weights", evaluate_dir(net, params, wav_dir, verbose=False, local_dir=local_dir, local_mel=local_mel)["total"])
    sys.stdout.flush()


def main(argv=None):
    args = _args.parse(argv)
    if args.ema:
        raise Exception("--ema belongs to generate and evaluate; train keeps an average with --ema-decay")
    params, net = _model.build(args, train=True)
    _local.require_match(net.local, args.local_dir is not None or args.local_mel, "train", "--local-dir FEAT_DIR or --local-mel")
    local_mel = net.local_mel if args.local_mel else None      # (--local-dir on such a checkpoint: the feature files win)
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
    start_time = time.time()
    graphs = {}
    average_loss = None
    for epoch in range(1, args.max_epoch):                          # train.py:118: epochs 1 .. max_epoch - 1
        average_loss = 0.0
        for fn in files:
            average_loss += train_audio(net, params, os.path.join(args.wav_dir, fn), batch_size=args.batch_size,
                                        train_width=args.train_width, repeat=args.repeat,
                                        use_graph=not args.no_graph, state=graphs, local_dir=args.local_dir,
                                        local_crop=args.local_crop or "frame", local_mel=local_mel)
            net.save(args.model_dir)
        average_loss /= len(files)
        sys.stdout.write("\033[2K\repoch: {} - {:.4e} loss - {} min\n".format(
            epoch, average_loss, int((time.time() - start_time) / 60)))
        sys.stdout.flush()
        net.save(args.model_dir)
        if args.valid_wav_dir:
            validate(net, params, args.valid_wav_dir, epoch, local_dir=args.local_dir, local_mel=local_mel)
    return average_loss


if __name__ == "__main__":
    main()
