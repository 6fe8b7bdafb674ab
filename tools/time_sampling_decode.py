"""Time on-device generation with the sampling controls off and on (temperature 0.8, top-k 40, top-p 0.9).

  python tools/time_sampling_decode.py [--steps 16000] [--batch 28] [--reps 5] [--out FILE.json] [--label NAME]

Model: BASELINE config 4 (4 x 10 layers of 32 channels, 256-way head), seed 1234 -- bench.py's decode workload.  Each figure
is the best and the median of ``--reps`` timed calls after one untimed call of the same shape (code objects loaded, decoder
handles created); a call ends in a device synchronise, the clock is the host's.  ``generate`` includes its prefill (one full
forward over the 4,094-sample window) as a user pays for it.  Run on a tree without the controls (an older commit) the script
times what that tree has and leaves the "on" entries out, so the same file measures both sides of a comparison.
Needs a GPU; there is no fallback."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("WAVENET_AMD_TREE", ROOT))

import numpy as np      # noqa: E402
import torch            # noqa: E402

CFG4 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10,
            residual_num_blocks=4, softmax_conv_channels=[256, 256])
ON = dict(temperature=0.8, top_k=40, top_p=0.9)


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
    ap.add_argument("--steps", type=int, default=16000)
    ap.add_argument("--batch", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="tree")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_sampling_decode.py needs a GPU")
    from wavenet_amd import FasterWaveNet, Params
    p = Params(CFG4)
    net = FasterWaveNet(p, seed=1234)
    net.to_gpu()
    has_controls = "temperature" in inspect.signature(net.generate).parameters
    rs = np.random.RandomState(0)
    u1 = rs.random_sample(a.steps)
    ub = rs.random_sample((a.batch, a.steps))
    res = {"label": a.label, "steps": a.steps, "batch": a.batch, "reps": a.reps, "has_controls": has_controls,
           "device": torch.cuda.get_device_name(0), "controls_on": ON}
    modes = [("off", {})] + ([("on", ON)] if has_controls else [])
    for rnd in range(2):                                  # off, on, off, on: both modes see the same drift of the box
        for name, kw in modes:
            t1 = timed(lambda: net.generate(a.steps, u1, **kw), a.reps)
            tb = timed(lambda: net.generate_batch(a.steps, ub, **kw), a.reps)
            for key, ts, ntok in (("generate", t1, a.steps), ("generate_batch", tb, a.steps * a.batch)):
                e = res.setdefault("%s_%s" % (key, name), {"seconds": []})
                e["seconds"] += [round(t, 6) for t in ts]
                e["tokens"] = ntok
    for key, e in res.items():
        if isinstance(e, dict) and "seconds" in e:
            e["best_tokens_per_s"] = round(e["tokens"] / min(e["seconds"]), 1)
            e["median_tokens_per_s"] = round(e["tokens"] / statistics.median(e["seconds"]), 1)
    if has_controls:
        for key in ("generate", "generate_batch"):
            res["%s_on_over_off_time" % key] = round(statistics.median(res[key + "_on"]["seconds"]) /
                                                     statistics.median(res[key + "_off"]["seconds"]), 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
