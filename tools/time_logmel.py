"""Time the log-mel front end on the device (``features.LogMel``, wn_logmel) against numpy's ``features.log_mel`` on the same
data, and record its accuracy on the test shapes.

  python tools/time_logmel.py [--out profiles/logmel.json] [--timeout 240]

At 80 mels / hop 256 / win 1024, 16 kHz, for (a) one 60 s signal and (b) 64 clips of 16,000 samples in one ``batch`` call:
the time per call on the stream between two HIP events (median of 20 calls behind 5 untimed ones; the samples are on the
device already; the events bracket the whole ``batch`` call -- output allocation, input checks, the descriptor array -- so the
figure bounds the call from above and is not the kernel's own time), the number of kernel launches per call, and the wall
time of ``log_mel`` on the same data on the host (median of 3).
(c) accuracy: for every shape of tests/logmel_ref.py, the largest |device - log_mel| over all cells next to that of the float32
numpy restatement and the bar of tests/test_gpu_logmel.py.  Every step runs in a child process of its own under ``--timeout``
seconds; a step that fails ends the run.  Needs a GPU; there is no fallback."""
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

RATE, MELS, HOP, WIN = 16000, 80, 256, 1024
STEPS = ("one_signal_60s", "batch_64x16000", "accuracy")


def _timed(mel, clips, host_clips):
    import torch
    from wavenet_amd import features
    for _ in range(5):
        mel.batch(clips)
    before = mel.launches
    ms = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mel.batch(clips)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    launches = (mel.launches - before) // 20
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for c in host_clips:
            features.log_mel(c, RATE, MELS, HOP, WIN)
        host.append(1e3 * (time.perf_counter() - t0))
    return {"device_ms_median": round(statistics.median(ms), 4), "device_ms_min": round(min(ms), 4), "device_ms_max": round(max(ms), 4),
            "launches_per_call": launches, "numpy_log_mel_ms_median": round(statistics.median(host), 3),
            "clips": len(clips), "samples_per_clip": int(host_clips[0].size)}


def step(name):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_logmel.py needs a GPU")
    import logmel_ref as L
    from wavenet_amd import features
    if name == "accuracy":
        rows = []
        for win, hop, n_mels, n in L.SHAPES:
            x = L.chirp_signal(n).astype(np.float32)
            bar, ref_err = L.bar(x, win, hop, n_mels)
            got = features.LogMel(L.RATE, n_mels, hop, win)(x).cpu().numpy()
            err = float(np.abs(got.astype(np.float64) - features.log_mel(x, L.RATE, n_mels, hop, win)).max())
            rows.append({"win": win, "hop": hop, "n_mels": n_mels, "samples": n, "device_max_abs_log_error": err,
                         "float32_restatement_max_abs_log_error": ref_err, "bar": bar})
        return rows
    mel = features.LogMel(RATE, MELS, HOP, WIN)
    n, count = (60 * RATE, 1) if name == "one_signal_60s" else (16000, 64)
    host = [L.chirp_signal(n).astype(np.float32) * (1.0 - 0.005 * c) for c in range(count)]
    return dict(_timed(mel, [torch.as_tensor(c).cuda() for c in host], host), device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logmel.json"))
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step(a.child)))
        return
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()), "shape": {"rate": RATE, "n_mels": MELS, "hop": HOP, "win": WIN}}
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
