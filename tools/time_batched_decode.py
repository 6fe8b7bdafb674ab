"""Time ``FasterWaveNet.generate_batch`` on a model the specialised decoder does not take, for a growing number of utterances.

  python tools/time_batched_decode.py [--steps 2000] [--batches 1,16,64,256] [--reps 5] [--out FILE.json] [--label NAME]

Model: 2 blocks x 8 layers, 64 residual / 64 dilated / 128 skip channels, 256-way head, fp32, seed 1234 -- every utterance is
one workgroup of the any-shape decode kernel.  Each figure is the median (and the best) of ``--reps`` timed calls after one
untimed call of the same shape (code objects loaded, decoder handles created); a call ends in a device synchronise, the clock
is the host's.  A call includes its prefill (one full forward over the 512-sample window per distinct prompt: one here) as a
user pays for it.  Run on a tree whose ``generate_batch`` loops over ``generate()`` for such a model (an older commit:
``WAVENET_AMD_TREE=<checkout>``) the script times that loop, so the same file measures both sides of a comparison.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("WAVENET_AMD_TREE", ROOT))

import numpy as np      # noqa: E402
import torch            # noqa: E402

MODEL = dict(quantization_steps=256, causal_conv_channels=[64], residual_conv_channels=[64] * 8, residual_num_blocks=2,
             softmax_conv_channels=[128, 256])


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_batched_decode.py needs a GPU")
    import wavenet_amd
    from wavenet_amd import FasterWaveNet, Params
    net = FasterWaveNet(Params(MODEL), seed=1234)
    net.to_gpu()
    calls = [0]
    inner = net.generate

    def counted(*args, **kw):
        calls[0] += 1
        return inner(*args, **kw)
    net.generate = counted                                  # how many single runs a generate_batch call made: 0 = one launch
    rs = np.random.RandomState(0)
    res = {"label": a.label, "tree": os.path.dirname(os.path.dirname(os.path.abspath(wavenet_amd.__file__))), "model": MODEL,
           "steps": a.steps, "reps": a.reps, "device": torch.cuda.get_device_name(0), "batches": {}}
    first_row = None
    for N in [int(v) for v in a.batches.split(",")]:
        u = rs.random_sample((N, a.steps))
        calls[0] = 0
        last = [None]

        def call():
            last[0] = net.generate_batch(a.steps, u)
        ts = timed(call, a.reps)
        toks = last[0]
        if first_row is None:
            first_row = int(toks[0].sum().item())
        res["batches"][str(N)] = {
            "seconds": [round(t, 6) for t in ts], "tokens": N * a.steps,
            "median_tokens_per_s": round(N * a.steps / statistics.median(ts), 1),
            "best_tokens_per_s": round(N * a.steps / min(ts), 1),
            "generate_calls_per_call": calls[0] // (a.reps + 1), "token_checksum": int(toks.sum().item())}
        sys.stderr.write("N = %d: %s\n" % (N, json.dumps(res["batches"][str(N)])))
        sys.stderr.flush()
    res["utterance0_checksum"] = first_row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
