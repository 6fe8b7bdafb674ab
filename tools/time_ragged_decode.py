"""Time ``FasterWaveNet.generate_batch`` with a length per utterance, and check that the word per utterance costs the
equal-length call nothing.

  python tools/time_ragged_decode.py [--parent-lib libwavenet_hip.so] [--reps 20] [--out profiles/ragged_decode.json]

Model of profiles/batched_decode_any_shape.json (tools/time_batched_decode.py): 2 blocks x 8 layers, 64 residual / 64 dilated /
128 skip channels, 256-way head, fp32, seed 1234; 64 utterances whose lengths are drawn once, uniformly in [500, 2000], from
seed 0.  Measured, each call ending in a device synchronise on the host's clock, a call including its prefill:

1. the ragged call, its launch's handles passed longest first and in the caller's order (``batch_longest_first``);
2. the loop over ``generate()`` at the same lengths, and the longest utterance alone;
3. the equal-length int call at 2,000 samples.

``--parent-lib``: the library built from the parent commit.  The int call of (3), and config 4's 28-utterance launch (nine
workgroups per utterance, 2,000 samples), are then timed on both libraries in this one process -- a model object per library,
calls interleaved A B A B ..., median of ``--reps`` after one untimed call each (tools/time_batched_decode.py's protocol) --
and the difference of the medians is compared with the spread (max - min) of the runs.  (The parent library reads the
descriptor without ``step_limit``; with the field 0 and no frame table the two layouts hold the same values.)
Needs a GPU; there is no fallback."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

MODEL = dict(quantization_steps=256, causal_conv_channels=[64], residual_conv_channels=[64] * 8, residual_num_blocks=2,
             softmax_conv_channels=[128, 256])
CFG4 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10, residual_num_blocks=4,
            softmax_conv_channels=[256, 256])
N_UTT, LO, HI = 64, 500, 2000


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed(fn, reps):
    fn()
    return [clock(fn) for _ in range(reps)]


def figures(ts, samples):
    med = statistics.median(ts)
    return {"seconds": [round(t, 6) for t in ts], "median_s": round(med, 6), "min_s": round(min(ts), 6), "max_s": round(max(ts), 6),
            "spread_s": round(max(ts) - min(ts), 6), "samples": samples, "median_samples_per_s": round(samples / med, 1)}


def ab(sides, reps, samples):
    """sides: [(name, use, fn)].  One untimed call each, then ``reps`` rounds of one timed call per side, interleaved."""
    for _, use, fn in sides:
        use()
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _, _ in sides}
    for _ in range(reps):
        for name, use, fn in sides:
            use()
            ts[name].append(clock(fn))
    out = {name: figures(t, samples) for name, t in ts.items()}
    if len(sides) == 2:
        a, b = (out[name] for name, _, _ in sides)
        diff = a["median_s"] - b["median_s"]
        out["median_difference_s"] = round(diff, 6)
        out["median_difference_percent"] = round(100.0 * diff / b["median_s"], 3)
        out["inside_the_spread"] = bool(abs(diff) <= max(a["spread_s"], b["spread_s"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ragged-reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ragged_decode.py needs a GPU")
    from wavenet_amd import FasterWaveNet, Params, _lib
    branch_lib = _lib.lib()
    parent_lib = None
    if a.parent_lib:
        _lib._lib, _lib.LIB_PATH, keep = None, os.path.abspath(a.parent_lib), _lib.LIB_PATH
        parent_lib = _lib.lib()
        _lib._lib, _lib.LIB_PATH = branch_lib, keep

    def use(lib):
        def switch():
            _lib._lib = lib
        return switch

    rs = np.random.RandomState(0)
    lengths = [int(v) for v in rs.randint(LO, HI + 1, N_UTT)]
    u = rs.random_sample((N_UTT, HI))
    res = {"what": __doc__.split("\n\n")[0], "model": MODEL, "utterances": N_UTT, "lengths": lengths, "samples": int(sum(lengths)),
           "device": torch.cuda.get_device_name(0), "reps": a.reps}
    net = FasterWaveNet(Params(MODEL), seed=1234)
    net.to_gpu()
    # 1. the ragged call, both orders of a launch's handles
    rows = {}
    for name, flag in (("longest_first", True), ("caller_order", False)):
        net.batch_longest_first = flag
        last = [None]

        def call():
            last[0] = net.generate_batch(lengths, u)
        res["ragged_" + name] = figures(timed(call, a.ragged_reps), sum(lengths))
        rows[name] = [int(r.sum().item()) for r in last[0]]
    net.batch_longest_first = True
    res["ragged_orders_give_the_same_tokens"] = rows["longest_first"] == rows["caller_order"]
    # 2. the loop over generate() at the same lengths, and the longest utterance alone
    longest = int(np.argmax(lengths))
    res["longest_alone"] = figures(timed(lambda: net.generate(lengths[longest], u[longest]), a.ragged_reps), lengths[longest])
    single = [None] * N_UTT

    def loop():
        for i in range(N_UTT):
            single[i] = net.generate(lengths[i], u[i])
    res["loop_over_generate"] = figures([clock(loop) for _ in range(a.loop_reps)], sum(lengths))
    res["ragged_rows_equal_the_loop"] = rows["longest_first"] == [int(r.sum().item()) for r in single]
    res["ragged_time_over_longest_alone"] = round(res["ragged_longest_first"]["median_s"] / res["longest_alone"]["median_s"], 3)
    res["ragged_rate_over_loop_rate"] = round(res["ragged_longest_first"]["median_samples_per_s"] /
                                              res["loop_over_generate"]["median_samples_per_s"], 2)
    # 3. the equal-length int call; with --parent-lib on both libraries, and config 4's 28-utterance launch likewise
    libs = [("branch", branch_lib)] + ([("parent", parent_lib)] if parent_lib is not None else [])
    for key, cfg, N, n in (("equal_length_int_call", MODEL, N_UTT, HI), ("cfg4_28_utterances", CFG4, 28, HI)):
        uu = np.random.RandomState(1).random_sample((N, n))
        sides, nets, sums = [], [], {}
        for name, lib in libs:
            use(lib)()
            m = net if (cfg is MODEL and name == "branch") else FasterWaveNet(Params(cfg), seed=1234)
            if m is not net:
                m.to_gpu()
            nets.append((lib, m))

            def call(m=m, name=name):
                sums[name] = int(m.generate_batch(n, uu).sum().item())
            sides.append((name, use(lib), call))
        res[key] = ab(sides, a.reps, N * n)
        res[key]["utterances"], res[key]["n_samples"] = N, n
        res[key]["same_tokens_on_both_libraries"] = len(set(sums.values())) == 1
        for lib, m in nets:                                     # a library's handles are destroyed by that library
            if m is not net:
                use(lib)()
                m.close()
        del nets, sides
        gc.collect()
    use(branch_lib)()
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
