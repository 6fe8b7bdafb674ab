"""Time streaming synthesis (``FasterWaveNet.open_stream``, WN_DECODER_FRAME_RING) of a locally conditioned model of config 4's
shape against the one-shot calls, and the one-shot calls against another build of the library.

  python tools/time_stream_decode.py [--samples 16000] [--reps 5] [--stream-reps 3] [--pulls 256,1024,4096]
                                     [--other-lib PATH/libwavenet_hip.so] [--out FILE.json]

Model: BASELINE config 4 -- 4 blocks x 10 layers of 32 channels, 256 skip channels, head 256 -> 256, fp32, seed 1234 --, with 5
feature channels at hop 256, in repeat and in linear mode (random features, one array for all utterances of a call; every
utterance draws with its own uniforms).  A timed call ends in a device synchronise; the clock is the host's.
(a) flat: ``generate`` for one utterance and ``generate_batch`` for 28, unflagged flat-table handles, prefill included -- the
median and the spread of ``--reps`` calls behind one untimed call of 256 samples.  With ``--other-lib`` the same flat cases run in
a fresh child process that loads that build (``WAVENET_HIP_LIB``) BEFORE and AFTER this tree's: the other build's own two passes
give the spread that this tree's ratio is held against (every repetition of both passes, over the mean of their medians).
(b) streamed: the same workload through ``open_stream`` -- the stream opened with the window's columns, then per pull of P
samples a ``push`` of the P / hop feature columns behind it (the projection runs per push) and a ``pull(P)``; the whole of it,
from the opening call to the last token on the host, ``--stream-reps`` times per P; the rate, its ratio to (a) of the same
process, and the rate of the part behind the opening call.
(c) the time from the opening call to the first pulled chunk on the host, next to the one-shot call's median.
Token checksums: a stream's tokens are compared with the one-shot call's, element by element (``same_tokens``); rows made by
``push`` come from projections over fewer columns, so a difference at a near-tie is possible and is reported, not asserted.
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


def _rates(tok, ts):
    return {"seconds": [round(t, 6) for t in ts], "samples_per_s_median": round(tok / statistics.median(ts), 1),
            "samples_per_s_min": round(tok / max(ts), 1), "samples_per_s_max": round(tok / min(ts), 1)}


def measure(a, stream):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_stream_decode.py needs a GPU")
    from wavenet_amd import FasterWaveNet, Params, _lib
    from wavenet_amd.wavenet import frames_needed
    res = {"library": _lib.LIB_PATH, "device": torch.cuda.get_device_name(0), "samples": a.samples, "reps": a.reps, "flat": {},
           "stream": {}}
    n = a.samples
    u = np.random.RandomState(0).random_sample((BATCH, n))
    pulls = [int(p) for p in a.pulls.split(",")]
    for interp in ("repeat", "linear"):
        net = FasterWaveNet(Params(CFG4), seed=1234, local_channels=FEATS, local_hop=HOP, local_interp=interp)
        net.to_gpu()
        W = net.input_width
        h = np.random.RandomState(1).standard_normal((FEATS, frames_needed(W + n - 1, HOP, 0, interp))).astype(np.float32)
        cw = frames_needed(W, HOP, 0, interp)
        for N in (1, BATCH):
            key = "local_%s/%d" % (interp, N)
            last = [None]

            def call(m):
                last[0] = net.generate(m, u[0, :m], local=h) if N == 1 else net.generate_batch(m, u[:, :m], local=h)
                torch.cuda.synchronize()
            call(min(256, n))                             # untimed: code objects, handles
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(n)
                ts.append(time.perf_counter() - t0)
            want = last[0].reshape(N, n).cpu()
            res["flat"][key] = dict(_rates(N * n, ts), token_checksum=int(want.sum().item()))
            sys.stderr.write("flat %s: %s\n" % (key, json.dumps(res["flat"][key])))
            if not stream:
                continue
            for P in pulls:
                def run(m_total):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got, done, col, t_first = [], 0, cw, None
                    with net.open_stream(utterances=N, local=h[:, :cw], max_pull=max(P, 2)) as st:
                        t_open = time.perf_counter() - t0
                        while done < m_total:
                            m = min(P, m_total - done)
                            # the columns behind the next m samples, as far as the ring takes them
                            while col < h.shape[1] and min(st.available()) < m:
                                k = min(max(1, P // HOP), h.shape[1] - col)
                                st.push(h[:, col:col + k] if N == 1 else [h[:, col:col + k]] * N)
                                col += k
                            m = min(m, min(st.available()))
                            if st.book.two_steps and m_total - done - m == 1:
                                m -= 1
                            if m < 1:
                                raise SystemExit("the features do not cover %d samples" % m_total)
                            got.append(st.pull(m, u[:N, done:done + m]).cpu())
                            if t_first is None:
                                t_first = time.perf_counter() - t0
                            done += m
                        torch.cuda.synchronize()
                    return time.perf_counter() - t0, t_open, t_first, torch.cat(got, dim=1), st.ring_frames
                run(min(2 * P + 2, n))                    # untimed: the stream's shapes
                runs = [run(n) for _ in range(a.stream_reps)]
                ts = [r[0] for r in runs]
                med = statistics.median(ts)
                behind = statistics.median([r[0] - r[1] for r in runs])
                flat_med = statistics.median(res["flat"][key]["seconds"])
                diff = (runs[-1][3] != want)
                res["stream"]["%s/pull_%d" % (key, P)] = dict(
                    _rates(N * n, ts), ring_frames=runs[-1][4], over_flat=round(flat_med / med, 4),
                    samples_per_s_behind_the_opening_call=round(N * n / behind, 1),
                    seconds_opening_call_median=round(statistics.median([r[1] for r in runs]), 6),
                    seconds_to_first_chunk_median=round(statistics.median([r[2] for r in runs]), 6),
                    seconds_flat_call_median=round(flat_med, 6),
                    same_tokens=not bool(diff.any()), utterances_that_differ=int(diff.any(dim=1).sum().item()))
                sys.stderr.write("stream %s pull %d: %s\n" % (key, P, json.dumps(res["stream"]["%s/pull_%d" % (key, P)])))
                sys.stderr.flush()
        net.close()
    return res


def _child(a, lib):
    env = dict(os.environ, WAVENET_HIP_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--samples", str(a.samples), "--reps", str(a.reps)],
                       env=env, capture_output=True, text=True)
    sys.stderr.write(r.stderr)
    if r.returncode != 0:
        raise SystemExit("the run with %s failed (%d)" % (lib, r.returncode))
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream-reps", type=int, default=3)
    ap.add_argument("--pulls", default="256,1024,4096")
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a, False)))
        return
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()), "sampling_rate": 16000}
    if a.other_lib:
        res["other_pass_1"] = _child(a, a.other_lib)
    res["tree"] = measure(a, True)
    if a.other_lib:
        res["other_pass_2"] = _child(a, a.other_lib)
        cmp_ = {}
        for k, t in res["tree"]["flat"].items():
            o1, o2 = res["other_pass_1"]["flat"][k], res["other_pass_2"]["flat"][k]
            mean = 0.5 * (o1["samples_per_s_median"] + o2["samples_per_s_median"])
            lo, hi = min(o1["samples_per_s_min"], o2["samples_per_s_min"]) / mean, max(o1["samples_per_s_max"], o2["samples_per_s_max"]) / mean
            ratio = t["samples_per_s_median"] / mean
            cmp_[k] = {"tree_over_other": round(ratio, 4), "others_own_spread": [round(lo, 4), round(hi, 4)],
                       "others_two_medians": [o1["samples_per_s_median"], o2["samples_per_s_median"]],
                       "inside_the_others_spread": lo <= ratio <= hi,
                       "same_tokens": t["token_checksum"] == o1["token_checksum"] == o2["token_checksum"]}
        res["flat_tree_against_other"] = cmp_
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
