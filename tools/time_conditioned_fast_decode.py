"""Time generation of a locally conditioned model of config 4's shape, which WN_DECODER_GATE_ROWS puts on the specialised
decoder, against the unconditioned model on the same kernels and against another build of the library.

  python tools/time_conditioned_fast_decode.py [--samples 16000] [--reps 5] [--slow-reps 2] [--other-lib PATH/libwavenet_hip.so]
                                               [--cases unconditioned,local_repeat,local_linear] [--out FILE.json]

Model: BASELINE config 4 -- 4 blocks x 10 layers of 32 channels, 256 skip channels, head 256 -> 256, fp32, seed 1234 --, with
5 feature channels at hop 256 where conditioned (random features, one array for all utterances of a call, so a call has one
prefill whatever its batch; every utterance holds its own copy of the table and draws with its own uniforms).  Cases: the
unconditioned model, the conditioned one in repeat and in linear mode; each for one utterance (``generate``) and for 28
utterances in one launch (``generate_batch``).  A call ends in a device synchronise and includes its prefill, as a user pays
for it; the clock is the host's.  Each figure is the median (and the spread) of ``--reps`` timed calls behind one untimed call
of 256 samples (code objects loaded, handles created).  A case whose second 256-sample call takes more than 0.08 s -- the
any-shape decoder, one workgroup per utterance: what a library without the flag gives the conditioned model -- is timed
``--slow-reps`` times instead (a call takes many seconds there, and a persistent kernel's time does not vary).  Next to the rate
of the whole call stands the MARGINAL rate, (samples - 256) / (median call - median 256-sample call): what a decode step costs
with the call's fixed part taken out -- the prefill (a conditioned one runs every layer as its own launch) and the handle updates
(a conditioned call re-packs every handle it gives a table: ~170 small launches per utterance).

``--other-lib``: the same cases once more in a fresh child process that loads that build of the library (``WAVENET_HIP_LIB``)
under this tree's Python -- a build from before the flag ignores it.  The result holds both, the ratios, and for the
unconditioned cases whether this tree's median lies inside the other build's own spread.  Token checksums: the unconditioned
ones must agree between the builds; the conditioned ones may differ where the other build decodes on the any-shape kernels
(another summation order: a near-tie of the cumulative distribution can fall the other way).
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG4 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10, residual_num_blocks=4,
            softmax_conv_channels=[256, 256])
FEATS, HOP, BATCH = 5, 256, 28


def measure(a):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_conditioned_fast_decode.py needs a GPU")
    import wavenet_amd
    from wavenet_amd import FasterWaveNet, Params, _lib
    from wavenet_amd.wavenet import frames_needed
    res = {"library": _lib.LIB_PATH, "device": torch.cuda.get_device_name(0), "samples": a.samples, "reps": a.reps,
           "slow_reps": a.slow_reps, "cases": {}}
    rs = np.random.RandomState(0)
    u = rs.random_sample((BATCH, a.samples))
    for name, interp in (("unconditioned", None), ("local_repeat", "repeat"), ("local_linear", "linear")):
        if name not in a.cases.split(","):
            continue
        kw = {} if interp is None else dict(local_channels=FEATS, local_hop=HOP, local_interp=interp)
        net = FasterWaveNet(Params(CFG4), seed=1234, **kw)
        net.to_gpu()
        W = net.input_width
        call_kw = {}
        if interp is not None:
            h = np.random.RandomState(1).standard_normal((FEATS, frames_needed(W + a.samples - 1, HOP, 0, interp))).astype(np.float32)
            call_kw = dict(local=h)
        for N in (1, BATCH):
            last = [None]

            def call(n):
                last[0] = net.generate(n, u[0, :n], **call_kw) if N == 1 else net.generate_batch(n, u[:, :n], **call_kw)
                torch.cuda.synchronize()
            call(min(256, a.samples))                     # untimed: code objects, handles
            t0 = time.perf_counter()
            call(min(256, a.samples))
            reps = a.reps if time.perf_counter() - t0 <= 0.08 or a.samples <= 256 else a.slow_reps
            ts, short = [], []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(min(256, a.samples))
                short.append(time.perf_counter() - t0)
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(a.samples)
                ts.append(time.perf_counter() - t0)
            tok = N * a.samples
            res["cases"]["%s/%d" % (name, N)] = {
                "seconds": [round(t, 6) for t in ts], "samples_per_s_median": round(tok / statistics.median(ts), 1),
                "samples_per_s_min": round(tok / max(ts), 1), "samples_per_s_max": round(tok / min(ts), 1),
                "seconds_256_samples_median": round(statistics.median(short), 6),
                "marginal_samples_per_s": round(N * (a.samples - 256) / (statistics.median(ts) - statistics.median(short)), 1)
                if a.samples > 256 else None,
                "token_checksum": int(last[0].sum().item())}
            sys.stderr.write("%s, N = %d: %s\n" % (name, N, json.dumps(res["cases"]["%s/%d" % (name, N)])))
            sys.stderr.flush()
        net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-reps", type=int, default=2)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--cases", default="unconditioned,local_repeat,local_linear")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)))
        return
    res = {"protocol": __doc__.split("\n\n")[2].replace("\n", " "), "sampling_rate": 16000, "tree": measure(a)}
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    if a.other_lib:
        env = dict(os.environ, WAVENET_HIP_LIB=os.path.abspath(a.other_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--reps", str(a.reps),
                            "--slow-reps", str(a.slow_reps), "--cases", a.cases], env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            raise SystemExit("the run with %s failed (%d)" % (a.other_lib, r.returncode))
        other = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res["other"] = other
        cmp_ = {}
        for k, t in res["tree"]["cases"].items():
            o = other["cases"][k]
            cmp_[k] = {"tree_over_other": round(t["samples_per_s_median"] / o["samples_per_s_median"], 4),
                       "tree_median_inside_the_others_spread": o["samples_per_s_min"] <= t["samples_per_s_median"] <= o["samples_per_s_max"],
                       "same_tokens": t["token_checksum"] == o["token_checksum"]}
        res["tree_against_other"] = cmp_
    t = res["tree"]["cases"]
    # what the rows cost: 1 - conditioned rate / unconditioned rate, same process, same kernels
    cond = [k for k in ("local_repeat", "local_linear") if k + "/1" in t]
    if "unconditioned/1" in t:
        for key, field in (("rows_cost", "samples_per_s_median"), ("rows_cost_marginal", "marginal_samples_per_s")):
            res[key] = {"%s/%d" % (k, N): round(1.0 - t["%s/%d" % (k, N)][field] / t["unconditioned/%d" % N][field], 4)
                        for k in cond for N in (1, BATCH) if t["%s/%d" % (k, N)][field]}
    res["one_utterance_faster_than_real_time"] = {k: t["%s/1" % k]["samples_per_s_median"] > res["sampling_rate"] for k in cond}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
