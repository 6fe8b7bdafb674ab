"""What the exponential moving average of the weights (WaveNet.enable_ema) costs a replayed training step.

  python tools/time_ema_step.py [--reps 20] [--warmup 65] [--commit ID] [--out profiles/ema_step.json]

One process, one box: BASELINE config 2's step on the batch bench.py times (``bench.make_batch``), captured twice from one
seed -- the average off, then on -- each as a TrainStepGraph with ``keep_graph=True`` so that its kernel nodes can be counted.
Each figure is the median (and the minimum) of ``--reps`` replays timed with device events after ``--warmup`` untimed ones.
The expectation from the code: one more kernel node, reading the 2.46 MB weight arena and reading and writing the average
(3 x 2.46 MB), near the launch floor; the averaging launch is also timed by itself, outside the graph (``ema_launch_alone``).
The off figure means something only next to the on figure of the same run.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch            # noqa: E402

LAUNCH_FLOOR_US = 4.6   # one kernel node of a replayed graph on this GPU (wavenet_amd/graph.py); "a few" = 3 of them


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=65)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ema_step.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    import bench
    from wavenet_amd import FasterWaveNet, Params, TrainStepGraph
    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "workload": "BASELINE config 2, the batch of bench.make_batch, one replay of TrainStepGraph per step",
           "timing": "device events around one replay; the average off, then on, in one process", "decay": a.decay}
    for name, on in (("ema_off", False), ("ema_on", True)):
        net = FasterWaveNet(Params(bench.CFG2), seed=1234)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        if on:
            net.enable_ema(a.decay)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        graph = TrainStepGraph(net, x, tgt, keep_graph=True)
        for _ in range(a.warmup):
            graph.step()
        torch.cuda.synchronize()
        res[name] = stats([event_ms(graph.step) for _ in range(a.reps)])
        res[name]["kernel_nodes"] = graph.node_counts()["kernel"]
        res[name]["arena_floats"] = int(net._arena.numel())
        if on:
            res[name]["ema_t"] = net._ema_t
            res[name]["max_abs_weights_minus_average"] = float((net._arena - net._ema_arena).abs().max())
            # the averaging launch by itself, outside the graph: what of the difference below is the kernel
            for _ in range(5):
                net._ema_step()
            res["ema_launch_alone"] = stats([event_ms(net._ema_step) for _ in range(a.reps)])
        del graph, net
    diff_us = (res["ema_on"]["median_ms"] - res["ema_off"]["median_ms"]) * 1e3
    res["difference_of_medians_us"] = round(diff_us, 2)
    res["extra_kernel_nodes"] = res["ema_on"]["kernel_nodes"] - res["ema_off"]["kernel_nodes"]
    res["launch_floor_us"] = LAUNCH_FLOOR_US
    res["more_than_a_few_launch_floors"] = bool(diff_us > 3 * LAUNCH_FLOOR_US)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
