"""Time the rate converter on the device (``resample.Resampler``, wn_resample) against the numpy definition on the same data,
and record its accuracy on the test ratios.

  python tools/time_resample.py [--out profiles/resample.json] [--timeout 240]

For 48 -> 16 kHz and 44.1 -> 16 kHz, int16 PCM in and float32 out, (a) one 60 s signal and (b) 64 clips of 48,000 samples in one
``batch`` call: the time per call on the stream between two HIP events (median of 20 calls behind 5 untimed ones; the samples are
on the device already; the events bracket the whole ``batch`` call -- output allocation, input checks, the descriptor array -- so
the figure bounds the call from above and is not the kernel's own time), the number of kernel launches per call, the bytes the
call reads and writes (2 per input sample, 4 per output) over that time, for orientation, the wall time of ``resample.resample``
on the same data on the host (median of 3) and, where scipy.signal imports, that of ``resample_poly`` with the same taps.
(c) accuracy: for every ratio of tests/resample_ref.py, on the input of tests/test_gpu_resample.py, the largest
|device - definition| next to that of the float32 numpy restatement and the bar of the test.  Every step runs in a child process
of its own under ``--timeout`` seconds; a step that fails ends the run.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PAIRS = {"48k": (48000, 16000), "44k1": (44100, 16000)}
STEPS = ("one_signal_60s_48k", "batch_64x48000_48k", "one_signal_60s_44k1", "batch_64x48000_44k1", "accuracy")


def _timed(rs, clips, host_clips, rates):
    import torch
    from wavenet_amd import resample
    for _ in range(5):
        rs.batch(clips)
    before = rs.launches
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rs.batch(clips)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    launches = (rs.launches - before) // 20
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for c in host_clips:
            resample.resample(c, *rates)
        host.append(1e3 * (time.perf_counter() - t0))
    n_in = sum(int(c.size) for c in host_clips)
    n_out = sum(rs.count(int(c.size)) for c in host_clips)
    med = statistics.median(ms)
    res = {"device_ms_median": round(med, 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
           "launches_per_call": launches, "numpy_definition_ms_median": round(statistics.median(host), 3),
           "clips": len(clips), "samples_per_clip": int(host_clips[0].size), "outputs": n_out,
           "bytes_read_and_written": 2 * n_in + 4 * n_out, "gbytes_per_s_over_the_call": round((2 * n_in + 4 * n_out) / med / 1e6, 2),
           "taps_per_output": rs.T}
    try:
        from scipy.signal import resample_poly
    except Exception:
        res["scipy_resample_poly_ms_median"] = None
    else:
        h = resample.prototype(rs.L, rs.M) / rs.L
        sp = []
        for _ in range(3):
            t0 = time.perf_counter()
            for c in host_clips:
                resample_poly(c.astype("float64") / 32768.0, rs.L, rs.M, window=h)
            sp.append(1e3 * (time.perf_counter() - t0))
        res["scipy_resample_poly_ms_median"] = round(statistics.median(sp), 3)
    return res


def step(name):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_resample.py needs a GPU")
    import resample_ref as R
    from wavenet_amd import resample
    if name == "accuracy":
        rows = []
        tile = resample.RESAMPLE_TILE
        for rates in R.RATIOS:
            L, M = resample.ratio(*rates)
            n = -(-(2 * tile + 37) * M // L)
            x = R.pcm16(n, rates[0], seed=n)
            bar, ref_err = R.bar(x, *rates)
            got = resample.Resampler(*rates, device="cuda")(x).cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - resample.resample(x, *rates)).max())
            rows.append({"rate_in": rates[0], "rate_out": rates[1], "samples": n, "device_max_abs_error": err,
                         "float32_restatement_max_abs_error": ref_err, "bar": bar})
        return rows
    shape, pair = name.rsplit("_", 1)
    rates = PAIRS[pair]
    rs = resample.Resampler(*rates, device="cuda")
    n, count = (60 * rates[0], 1) if shape == "one_signal_60s" else (48000, 64)
    host = [R.pcm16(n, rates[0], seed=c) for c in range(count)]
    return dict(_timed(rs, [torch.as_tensor(c).cuda() for c in host], host, rates), device=torch.cuda.get_device_name(0),
                rate_in=rates[0], rate_out=rates[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step(a.child)))
        return
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split())}
    for name in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], capture_output=True, text=True,
                               timeout=a.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("step %s ran into its time limit of %d s: nothing more is started" % (name, a.timeout))
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            raise SystemExit("step %s failed (%d): nothing more is started" % (name, r.returncode))
        res[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        sys.stderr.write("%s: %s\n" % (name, json.dumps(res[name])))
    line = json.dumps(res, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
