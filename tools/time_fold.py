"""Time ``FasterWaveNet.generate_folded`` -- one long utterance as S overlapping segments of one batched call -- against
``generate()`` of the same utterance in the same process.

  python tools/time_fold.py [--shapes cfg4,small] [--reps 3] [--out profiles/fold.json]

Shapes: ``cfg4`` -- BASELINE config 4's shape (4 x 10 layers, 32 / 32 / 256 channels, the specialised decoder), 80 feature
channels at hop 256, one utterance of 160,000 samples, S about 7, 14, 28 and 56; ``small`` -- tools/time_batched_decode.py's model
(2 x 8 layers, 64 / 64 / 128), 80 channels at hop 64 (so that a body of 80,000 / 1,024 samples still holds a seam of one column),
one utterance of 80,000 samples, S = 16, 64, 256 and 1,024, with tiles off and with ``tile="auto"``.  Overlap and warm-up are the
method's defaults: one feature column and ``input_width`` samples.  A body is ceil((n - O) / S), so the plan has S segments or, where the rounding adds up, a few fewer (1,012 for 1,024).

Protocol: fp32, seed 1234, random features and uniforms from seed 0.  Per row one untimed call (code objects loaded, handles
created), then ``--reps`` timed calls, each ending in a device synchronise on the host's clock -- the whole call: prefills,
handle work, launches, unfold -- and one more call with a probe on ``wn_decoder_run_batch`` that synchronises the device ahead of
the first decode launch and reads the clock: ``share_before_first_launch`` is that call's time up to there over its whole time
(plans, uploads, one handle update and one batch-1 prefill per segment).  ``bound`` is the derived
min(S, capacity) * B / (B + W + O): the speed-up over one chain if every segment ran at the chain's own rate and nothing else
cost time.  ``generate()`` of the whole utterance is timed once per shape, after a short untimed call.  Every row carries the
checksum of its signal and the number of seams whose two sides agree.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (model, hop, samples, segment counts, tiles)
    "cfg4": (dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10, residual_num_blocks=4,
                  softmax_conv_channels=[256, 256]), 256, 160000, (7, 14, 28, 56), (0,)),
    "small": (dict(quantization_steps=256, causal_conv_channels=[64], residual_conv_channels=[64] * 8, residual_num_blocks=2,
                   softmax_conv_channels=[128, 256]), 64, 80000, (16, 64, 256, 1024), (0, "auto")),
}
FEATS = 80


class _FirstLaunch(object):
    """A probe on ``wn_decoder_run_batch``: ahead of the first launch inside the ``with`` the device is synchronised and the clock read."""

    def __init__(self, lib, torch):
        self.lib, self.torch, self.inner, self.at = lib, torch, lib.wn_decoder_run_batch, None

    def __enter__(self):
        def probed(*a):
            if self.at is None:
                self.torch.cuda.synchronize()
                self.at = time.perf_counter()
            return self.inner(*a)
        self.lib.wn_decoder_run_batch = probed
        return self

    def __exit__(self, *exc):
        self.lib.wn_decoder_run_batch = self.inner


def measure(name, reps):
    import numpy as np
    import torch
    from wavenet_amd import FasterWaveNet, Params, _lib, fold
    from wavenet_amd.wavenet import coarse_frames_needed
    model, hop, n, counts, tiles = SHAPES[name]
    net = FasterWaveNet(Params(model), seed=1234, local_channels=FEATS, local_hop=hop)
    net.to_gpu()
    W, O = int(net.input_width), hop
    rs = np.random.RandomState(0)
    h = rs.standard_normal((FEATS, coarse_frames_needed(W + n - 1, hop, 1, 0, "repeat"))).astype(np.float32)
    u = rs.random_sample(n)
    sync = torch.cuda.synchronize
    res = {"shape": name, "model": model, "local_channels": FEATS, "hop": hop, "samples": n, "input_width": W, "overlap": O,
           "warmup": W, "reps": reps, "device": torch.cuda.get_device_name(0),
           "n_cu": int(torch.cuda.get_device_properties(0).multi_processor_count), "rows": []}
    net.generate(2000, u, local=h)                          # untimed: code objects loaded, the batch-1 handle created
    sync()
    t0 = time.perf_counter()
    chain = net.generate(n, u, local=h)
    sync()
    res["generate_seconds"] = round(time.perf_counter() - t0, 6)
    res["generate_samples_per_s"] = round(n / res["generate_seconds"], 1)
    sys.stderr.write("%s generate(%d): %.3f s\n" % (name, n, res["generate_seconds"]))
    for S in counts:
        B = -(-(n - O) // S)
        plan = fold.fold_plan(n, B, O, W)
        for tile in tiles:
            cap = net.fold_capacity(tile)
            kw = dict(local=h, tile=tile)
            net.generate_folded(n, u, B, **kw)              # untimed
            sync()
            ts = []
            for _ in range(reps):
                sync()
                t0 = time.perf_counter()
                pcm = net.generate_folded(n, u, B, **kw)
                sync()
                ts.append(time.perf_counter() - t0)
            with _FirstLaunch(_lib.lib(), torch) as probe:
                sync()
                t0 = time.perf_counter()
                pcm, (_, rows, _) = net.generate_folded(n, u, B, return_segments=True, **kw)
                sync()
                t1 = time.perf_counter()
            med = statistics.median(ts)
            row = {"segments": len(plan.segments), "body": B, "tile": tile or "off", "capacity": cap,
                   "decoded_steps": int(sum(g.e - g.s for g in plan.segments)), "useful_share": round(fold.useful_share(plan), 4),
                   "seconds": [round(t, 6) for t in ts], "median_seconds": round(med, 6),
                   "samples_per_s": round(n / med, 1), "over_generate": round(res["generate_seconds"] / med, 3),
                   "bound": round(min(len(plan.segments), cap) * B / float(B + W + O), 3),
                   "share_before_first_launch": round((probe.at - t0) / (t1 - t0), 4), "probed_seconds": round(t1 - t0, 6),
                   "identical_seams": fold.identical_seams([r.cpu().numpy() for r in rows], plan),
                   "segment_0_is_the_chain": bool(torch.equal(rows[0][:B], chain[:B])),
                   "signal_checksum": int(pcm.to(torch.int64).sum().item())}
            res["rows"].append(row)
            sys.stderr.write("%s %s\n" % (name, json.dumps(row)))
            sys.stderr.flush()
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cfg4,small")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_fold.py needs a GPU")
    doc = {"shapes": [measure(s, a.reps) for s in a.shapes.split(",")]}
    line = json.dumps(doc)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
