"""Time the pitch tracker on the device (``pitch.Pitch``, wn_pitch) against numpy's ``pitch.yin`` on the same data, and record its
accuracy on the test shapes.

  python tools/time_pitch.py [--out profiles/pitch.json] [--timeout 300] [--kernel-stats STEP=kernel_stats.csv ...]

At win 1024 / hop 256 / 60-500 Hz (lags 32 .. 267), 16 kHz, for (a) one 60 s signal and (b) 64 clips of 16,000 samples in one
``batch`` call: the time per call on the stream between two HIP events (median of 20 calls behind 5 untimed ones; the samples
are on the device already; the events bracket the WHOLE ``batch`` call -- output allocation, input checks, the descriptor array --
so the figure bounds the call from above and is not the kernel's own time), the number of kernel launches per call, the wall
time of ``yin`` on the same data on the host (once: it takes seconds), and, counted from the shapes, the subtract + fma pairs
(frames x (tau_max + 1) x win; "issued" counts the lags of the last, partly filled group too), the waves (workgroups x waves of
ceil(ft x groups / 64)) and the LDS words the lanes read (two per lane and j: the broadcast sample and one new word of the lag
window).
(c) accuracy: for every shape of tests/pitch_ref.py, the largest |device - yin_curve| over all cells next to that of the float32
numpy restatement and the bar of tests/test_gpu_pitch.py, and the frames whose tau* or voicing differ from the definition's.
Every step runs in a child process of its own under ``--timeout`` seconds; a step that fails ends the run.

The kernel's own time comes from a run of its own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_pitch.py
--child STEP  -- and ``--kernel-stats STEP=DIR/.../*_kernel_stats.csv`` then adds, per step, k_pitch's average time next to two
lower bounds from the instructions of the built hot loop (per lane and j: 7 v_sub_f32 and 7 v_fmac_f32 -- the compiler packs
nothing at 7 lags -- and two LDS words in ds_read2_b32 pairs): VALU issue, a wave instruction taking 4 cycles of its SIMD, 256 CUs
x 4 SIMDs at 2.4 GHz; and the LDS array, which the four SIMDs of a CU share, at 2 cycles per conflict-free ds_read_b32 wave
access (ds_read2_b32: 4), the lag window being read 7 words apart on neighbouring lanes (odd: no bank conflict within a frame).
``--counters STEP=DIR/.../*_counter_collection.csv`` (rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VALU, again
a run of its own) adds the counters' sums over k_pitch's dispatches and the share of LDS-array cycles that are conflict cycles.
Needs a GPU; there is no fallback."""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RATE, HOP, WIN, FMIN, FMAX = 16000, 256, 1024, 60.0, 500.0
STEPS = ("one_signal_60s", "batch_64x16000", "accuracy")
CUS, CLOCK_HZ = 256, 2.4e9
VALU_CYCLES_PER_WAVE_INSTRUCTION = 4      # 64 lanes on a 16-lane SIMD
LDS_CYCLES_PER_READ_B32 = 2               # conflict-free: two groups of 32 lanes, one LDS cycle each


def counted(p, clips):
    from wavenet_amd import features, pitch
    counts = [features.frame_count(int(c.numel() if hasattr(c, "numel") else c.size), p.hop) for c in clips]
    frames = sum(counts)
    lags = pitch.PITCH_LAGS_PER_LANE
    groups = (p.tau_max + lags) // lags
    ft = pitch.pitch_tile_frames(p.tau_max)
    # a full tile has ceil(ft groups / 64) waves (at most 4); a clip's last tile may have fewer frames
    waves = sum((n // ft) * min(4, -(-ft * groups // 64)) + (min(4, -(-(n % ft) * groups // 64)) if n % ft else 0) for n in counts)
    return {"frames": frames, "lags_per_lane": lags, "tile_frames": ft, "sub_fma_pairs": frames * (p.tau_max + 1) * p.win,
            "sub_fma_pairs_issued": frames * groups * lags * p.win, "waves": waves, "lds_words_read_per_lane_and_j": 2}


def _timed(p, clips, host_clips):
    import torch
    from wavenet_amd import pitch
    for _ in range(5):
        p.batch(clips)
    before = p.launches
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        p.batch(clips)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    launches = (p.launches - before) // 20
    t0 = time.perf_counter()
    for c in host_clips:
        pitch.yin(c, RATE, HOP, WIN, FMIN, FMAX)
    host = 1e3 * (time.perf_counter() - t0)
    return dict({"whole_batch_call_ms_median": round(statistics.median(ms), 4), "whole_batch_call_ms_min": round(min(ms), 4),
                 "whole_batch_call_ms_max": round(max(ms), 4), "launches_per_call": launches, "numpy_yin_ms": round(host, 1),
                 "clips": len(clips), "samples_per_clip": int(host_clips[0].size)}, **counted(p, clips))


def step(name):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_pitch.py needs a GPU")
    import pitch_ref as P
    from wavenet_amd import pitch
    if name == "accuracy":
        rows = []
        for (rate, win, hop, fmin, fmax, n), (tau_min, tau_max) in zip(P.SHAPES, P.LAGS):
            x = P.chirp_signal(n, tau_min, tau_max).astype(np.float32)
            bar, ref_err = P.bar(x, hop, win, tau_max)
            out, curve = pitch.Pitch(rate, hop, win, fmin, fmax, P.THRESHOLD).analyse(x)
            out, curve = out.cpu().numpy(), curve.cpu().numpy()
            c64 = pitch.yin_curve(x, rate, hop, win, fmin, fmax)
            t64, o64 = pitch.yin_select(c64, tau_min, P.THRESHOLD, rate)
            tdev, _ = pitch.yin_select(curve, tau_min, P.THRESHOLD, rate, np.float32)
            rows.append({"win": win, "hop": hop, "tau_min": tau_min, "tau_max": tau_max, "samples": n, "frames": int(t64.size),
                         "voiced_frames": int((o64[0] > 0).sum()),
                         "device_max_abs_curve_error": float(np.abs(curve.astype(np.float64) - c64).max()),
                         "float32_restatement_max_abs_curve_error": ref_err, "bar": bar,
                         "frames_deciding_otherwise": int(((tdev != t64) | ((out[0] > 0) != (o64[0] > 0))).sum())})
        return rows
    p = pitch.Pitch(RATE, HOP, WIN, FMIN, FMAX)
    n, count = (60 * RATE, 1) if name == "one_signal_60s" else (16000, 64)
    base = np.tile(P.chirp_signal(16000, p.tau_min, p.tau_max), n // 16000).astype(np.float32)
    host = [base * np.float32(1.0 - 0.005 * c) for c in range(count)]
    return dict(_timed(p, [torch.as_tensor(c).cuda() for c in host], host), device=torch.cuda.get_device_name(0))


def kernel_row(path, res, win=WIN):
    """k_pitch's row of a rocprofv3 kernel_stats.csv, and the two lower bounds the built hot loop gives for the counted waves."""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "k_pitch" in r.get("Name", "")]
    if not rows:
        raise SystemExit("%s has no k_pitch row" % path)
    us = float(rows[0]["AverageNs"]) / 1e3
    wave_js = res["waves"] * win                                     # hot-loop iterations, per wave
    valu = wave_js * 2 * res["lags_per_lane"] * VALU_CYCLES_PER_WAVE_INSTRUCTION / (CUS * 4 * CLOCK_HZ) * 1e6
    lds = wave_js * res["lds_words_read_per_lane_and_j"] * LDS_CYCLES_PER_READ_B32 / (CUS * CLOCK_HZ) * 1e6
    out = {"kernel_us_average": round(us, 2), "kernel_calls": int(rows[0]["Calls"]),
           "valu_issue_us_lower_bound": round(valu, 2), "lds_array_us_lower_bound": round(lds, 2),
           "valu_issue_share_of_kernel_time": round(valu / us, 4), "lds_array_share_of_kernel_time": round(lds / us, 4)}
    out["bound_by"] = "fp32 VALU issue" if valu >= lds else "LDS array"
    return out


def counter_row(path):
    """Sums of the counters of a rocprofv3 counter_collection.csv over k_pitch's dispatches."""
    sums, calls = {}, set()
    with open(path) as f:
        for r in csv.DictReader(f):
            if "k_pitch" in r.get("Kernel_Name", ""):
                sums[r["Counter_Name"]] = sums.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
                calls.add(r.get("Dispatch_Id"))
    if not sums:
        raise SystemExit("%s has no k_pitch row" % path)
    n = max(1, len(calls))
    out = {"dispatches": len(calls), "per_dispatch": {k: round(v / n) for k, v in sorted(sums.items())}}
    if sums.get("SQ_LDS_IDX_ACTIVE"):
        out["bank_conflict_share_of_lds_cycles"] = round(sums.get("SQ_LDS_BANK_CONFLICT", 0.0) / sums["SQ_LDS_IDX_ACTIVE"], 4)
        out["lds_array_us_if_spread_over_every_cu"] = round(sums["SQ_LDS_IDX_ACTIVE"] / n / (CUS * CLOCK_HZ) * 1e6, 2)
    if sums.get("SQ_INSTS_VALU"):
        out["valu_issue_us_if_spread_over_every_simd"] = round(
            sums["SQ_INSTS_VALU"] / n * VALU_CYCLES_PER_WAVE_INSTRUCTION / (CUS * 4 * CLOCK_HZ) * 1e6, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="STEP=CSV")
    ap.add_argument("--counters", action="append", default=[], metavar="STEP=CSV")
    ap.add_argument("--merge", default=None, metavar="JSON", help="take the steps' results from this file of an earlier run instead "
                                                                  "of running them (to add --kernel-stats / --counters)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step(a.child)))
        return
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()),
           "shape": {"rate": RATE, "hop": HOP, "win": WIN, "fmin": FMIN, "fmax": FMAX, "tau_min": 32, "tau_max": 267}}
    if a.merge:
        with open(a.merge) as f:
            res.update({k: v for k, v in json.load(f).items() if k in STEPS})
        import numpy as np
        from wavenet_amd import pitch
        p = pitch.Pitch(RATE, HOP, WIN, FMIN, FMAX, device="cpu")        # the shapes only: nothing is launched
        for name in STEPS[:2]:
            res[name].pop("lds_bytes_read", None)
            res[name].update(counted(p, [np.zeros(res[name]["samples_per_clip"], np.float32)] * res[name]["clips"]))
    for name in () if a.merge else STEPS:
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
    for item in a.kernel_stats:
        name, path = item.split("=", 1)
        res[name]["kernel"] = kernel_row(path, res[name])
        res["kernel_protocol"] = " ".join(__doc__.split("\n\n")[3].split())
    for item in a.counters:
        name, path = item.split("=", 1)
        res[name]["counters"] = counter_row(path)
    line = json.dumps(res, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
