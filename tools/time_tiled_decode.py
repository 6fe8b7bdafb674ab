"""Time ``FasterWaveNet.generate_batch`` on any-shape models with utterance tiles off and at every tile size that fits.

  python tools/time_tiled_decode.py --shape small|cfg5 [--steps K] [--batches 16,64,256,1024] [--reps 5]
                                    [--parent-lib PARENT/libwavenet_hip.so] [--out FILE.json]

Shapes: ``small`` -- tools/time_batched_decode.py's model (2 blocks x 8 layers, 64 residual / 64 dilated / 128 skip channels,
Q = 256), 2,000 samples by default, so the figures line up with profiles/batched_decode_any_shape.json; ``cfg5`` -- BASELINE
config 5's shape (4 x 10 layers, 128 / 128 / 512), 300 samples by default.  The protocol is time_batched_decode.py's: fp32,
seed 1234, one untimed call per N (code objects loaded, handles created), then ``--reps`` timed calls per tile size, each
ending in a device synchronise on the host's clock; a call includes its prefill.  Every figure carries the checksum of its
tokens: tiled and untiled must agree.

One process measures one library.  With ``--parent-lib`` the script measures nothing itself: it starts a child process per
pass -- the parent commit's library (``WAVENET_HIP_LIB``; untiled calls only: the older library knows no tile), this tree's
(everything), the parent's again --, one after another, and stops at the first that fails.  The untiled rate over the parent's
is then held against the spread of the parent's own two passes.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "small": (dict(quantization_steps=256, causal_conv_channels=[64], residual_conv_channels=[64] * 8, residual_num_blocks=2,
                   softmax_conv_channels=[128, 256]), 2000),
    "cfg5": (dict(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 10, residual_num_blocks=4,
                  softmax_conv_channels=[512, 256]), 300),
}


def measure(a):
    """One library, one process: {N: {tile: figures}}."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_tiled_decode.py needs a GPU")
    from wavenet_amd import FasterWaveNet, Params, _lib
    from wavenet_amd.faster_wavenet import pick_tile, tile_fit
    model, steps = SHAPES[a.shape][0], a.steps or SHAPES[a.shape][1]
    net = FasterWaveNet(Params(model), seed=1234)
    net.to_gpu()
    fit = tile_fit(net.params)
    n_cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    tiles = [0] + ([U for U in (2, 4, 8, 16) if U <= fit] if a.tiles == "all" else [])
    rs = np.random.RandomState(0)
    res = {"label": a.label, "library": _lib.LIB_PATH, "shape": a.shape, "model": model, "steps": steps, "reps": a.reps,
           "device": torch.cuda.get_device_name(0), "n_cu": n_cu, "tile_fit": fit, "batches": {}}
    for N in [int(v) for v in a.batches.split(",")]:
        u = rs.random_sample((N, steps))
        net.generate_batch(steps, u)                        # untimed: handles created, code objects loaded
        torch.cuda.synchronize()
        row = {}
        for U in tiles:
            ts, toks = [], None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks = net.generate_batch(steps, u, tile=U)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            row["off" if not U else str(U)] = {
                "seconds": [round(t, 6) for t in ts], "tokens": N * steps,
                "median_tokens_per_s": round(N * steps / statistics.median(ts), 1),
                "best_tokens_per_s": round(N * steps / min(ts), 1), "token_checksum": int(toks.sum().item())}
            sys.stderr.write("%s %s N = %d tile %s: %s\n" % (a.label, a.shape, N, U or "off", json.dumps(row["off" if not U else str(U)])))
            sys.stderr.flush()
        row["auto_picks"] = pick_tile(N, n_cu, fit)
        res["batches"][str(N)] = row
    return res


def compare(a):
    """Three child processes -- parent, this tree, parent -- and the comparison of their figures."""
    passes = []
    for label, lib, tiles in (("parent_pass1", a.parent_lib, "off"), ("tree", None, "all"), ("parent_pass2", a.parent_lib, "off")):
        env = dict(os.environ)
        env.pop("WAVENET_HIP_LIB", None)
        if lib:
            env["WAVENET_HIP_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", a.shape, "--batches", a.batches, "--reps", str(a.reps),
               "--tiles", tiles, "--label", label] + (["--steps", str(a.steps)] if a.steps else [])
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=a.pass_timeout)
        if r.returncode != 0:
            raise SystemExit("time_tiled_decode.py: the %s pass ended with status %d: nothing more is started" % (label, r.returncode))
        passes.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    p1, tree, p2 = passes
    doc = {"shape": a.shape, "model": tree["model"], "steps": tree["steps"], "reps": a.reps, "device": tree["device"], "n_cu": tree["n_cu"],
           "tile_fit": tree["tile_fit"], "batches": {}}
    for N, row in tree["batches"].items():
        r1, r2 = p1["batches"][N]["off"], p2["batches"][N]["off"]
        lo, hi = sorted([r1["median_tokens_per_s"], r2["median_tokens_per_s"]])
        rates = {k: v["median_tokens_per_s"] for k, v in row.items() if isinstance(v, dict)}
        best = max(rates, key=rates.get)
        sums = {v["token_checksum"] for v in row.values() if isinstance(v, dict)} | {r1["token_checksum"], r2["token_checksum"]}
        doc["batches"][N] = dict(row, parent_pass1=r1, parent_pass2=r2,
                                 parent_spread=round(hi / lo - 1.0, 4),
                                 off_over_parent_mean=round(rates["off"] / (0.5 * (lo + hi)), 4),
                                 off_inside_parent_spread=bool(lo <= rates["off"] <= hi),
                                 best=best, best_over_off=round(rates[best] / rates["off"], 3),
                                 auto_over_best=round(rates[str(row["auto_picks"]) if row["auto_picks"] else "off"] / rates[best], 4),
                                 checksums_equal=len(sums) == 1)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="small")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--batches", default="16,64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tiles", choices=["all", "off"], default="all")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pass-timeout", type=int, default=900)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = compare(a) if a.parent_lib else measure(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
