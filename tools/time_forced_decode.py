"""Time generation with given samples in the decode loop (WN_DECODER_FORCED_TOKENS), and the unflagged rate against another
build of the library.

  python tools/time_forced_decode.py [--samples 16000] [--reps 5] [--parent-lib PATH/libwavenet_hip.so] [--out FILE.json]

Model: BASELINE config 4 -- 4 blocks x 10 layers of 32 channels, 256 skip channels, head 256 -> 256, fp32, seed 1234 --, from
silence.  Cases, each for one utterance (``generate``) and for 28 utterances in one launch (``generate_batch``): ``unflagged``
(no ``forced=``, the call everybody made before the flag), and on flagged handles ``none`` (``forced`` all -1: every sample
drawn), ``all`` (every sample given: the tokens the unflagged call emitted) and ``gap`` (everything given but a stretch of a
tenth of the samples in the middle, which is drawn).  A call ends in a device synchronise and includes its prefill, as a user
pays for it; the clock is the host's.  Each figure is the median (and the spread, min .. max) of ``--reps`` timed calls behind
one untimed call of 256 samples (code objects loaded, handles created in the case's form).

``--parent-lib``: the two unflagged cases once more in fresh child processes that load that build (``WAVENET_HIP_LIB``) under
this tree's Python, one pass before this tree's cases and one after: the min .. max of all the parent's timed calls is the
spread this tree's unflagged median is held against ("unflagged calls pay nothing").  Only unflagged cases run on the other
build.  The token checksums of the unflagged cases must agree between the builds; in this tree ``none`` and ``all`` must emit
the unflagged tokens.
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
BATCH, Q = 28, 256


def measure(a, cases):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_forced_decode.py needs a GPU")
    from wavenet_amd import FasterWaveNet, Params, _lib
    res = {"library": os.path.relpath(_lib.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0), "samples": a.samples, "reps": a.reps, "cases": {}}
    u = np.random.RandomState(0).random_sample((BATCH, a.samples))
    net = FasterWaveNet(Params(CFG4), seed=1234)
    net.to_gpu()
    free = {}                                                   # the unflagged tokens: what ``all`` and ``gap`` are given
    for name in cases:
        form, N = name.split("/")
        N = int(N)
        last = [None]

        def forced_of(n):
            if form == "unflagged":
                return {}
            if form == "none":
                f = np.full((N, n), -1, np.int32)
            else:
                f = free[N][:, :n].copy()
                if form == "gap":
                    f[:, n // 2 - n // 20:n // 2 - n // 20 + n // 10] = -1
            return {"forced": f[0] if N == 1 else list(f)}

        def call(n):
            kw = forced_of(n)
            last[0] = net.generate(n, u[0, :n], **kw) if N == 1 else net.generate_batch(n, u[:, :n], **kw)
            torch.cuda.synchronize()
        call(min(256, a.samples))
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(a.samples)
            ts.append(time.perf_counter() - t0)
        tokens = last[0]
        if form == "unflagged":
            free[N] = tokens.cpu().numpy().reshape(N, a.samples).astype(np.int32)
        tok = N * a.samples
        row = {"seconds": [round(t, 6) for t in ts], "samples_per_s_median": round(tok / statistics.median(ts), 1),
               "samples_per_s_min": round(tok / max(ts), 1), "samples_per_s_max": round(tok / min(ts), 1),
               "token_checksum": int(tokens.sum().item())}
        res["cases"][name] = row
        sys.stderr.write("%s: %s\n" % (name, json.dumps(row)))
        sys.stderr.flush()
    net.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    unflagged = ["unflagged/1", "unflagged/%d" % BATCH]
    if a.child:
        print("RESULT " + json.dumps(measure(a, unflagged)))
        return

    def parent_pass():
        env = dict(os.environ, WAVENET_HIP_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--reps", str(a.reps)],
                           env=env, capture_output=True, text=True)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            raise SystemExit("the run with %s failed (%d)" % (a.parent_lib, r.returncode))
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()), "sampling_rate": 16000}
    passes = [parent_pass()] if a.parent_lib else []
    flagged = ["%s/%d" % (f, N) for N in (1, BATCH) for f in ("none", "all", "gap")]
    res["tree"] = measure(a, unflagged + flagged)
    if a.parent_lib:
        passes.append(parent_pass())
        res["parent_passes"] = passes
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    t = res["tree"]["cases"]
    # (a) the unflagged rate against the parent's, next to the spread the parent shows over its own two passes
    if passes:
        cmp_ = {}
        for k in unflagged:
            med = [p["cases"][k]["samples_per_s_median"] for p in passes]
            lo = min(p["cases"][k]["samples_per_s_min"] for p in passes)
            hi = max(p["cases"][k]["samples_per_s_max"] for p in passes)
            mean = sum(med) / len(med)
            cmp_[k] = {"tree_over_parent": round(t[k]["samples_per_s_median"] / mean, 4),
                       "parent_pass_medians": med, "parent_pass_to_pass": round(abs(med[0] - med[-1]) / mean, 4),
                       "parent_min_max_over_its_mean_median": [round(lo / mean, 4), round(hi / mean, 4)],
                       "tree_median_inside_the_parents_spread": lo <= t[k]["samples_per_s_median"] <= hi,
                       "same_tokens": all(p["cases"][k]["token_checksum"] == t[k]["token_checksum"] for p in passes)}
        res["unflagged_against_parent"] = cmp_
    # (b) the flagged rates, each a ratio to the unflagged rate of the same process
    res["flagged_over_unflagged"] = {f: {str(N): round(t["%s/%d" % (f, N)]["samples_per_s_median"] /
                                                       t["unflagged/%d" % N]["samples_per_s_median"], 4) for N in (1, BATCH)}
                                     for f in ("none", "all", "gap")}
    res["same_tokens_none_all_and_unflagged"] = all(t["%s/%d" % (f, N)]["token_checksum"] == t["unflagged/%d" % N]["token_checksum"]
                                                    for N in (1, BATCH) for f in ("none", "all"))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
