"""What pitch channels beside the log-mel cost: the analyser call that makes them, and the three extra channels in the step.

  python tools/time_pitch_condition.py [--reps 20] [--warmup 5] [--step-warmup 65] [--commit ID] [--out profiles/pitch_condition.json]

``analysis``: the whole ``acoustic.MelPitch.batch`` call (one ``LogMel`` launch and one ``Pitch`` launch per 64 clips, the channel
map, one ``cat`` per clip) against ``features.LogMel.batch`` alone, on one 60 s signal and on 64 clips of 16,000 samples, at
16 kHz with the default settings (80 mels, hop 256, window 1,024, F0 60 .. 500 Hz).  The inputs are float32 tensors on the
device.  Device events around the whole call; the median of ``--reps`` calls behind ``--warmup`` untimed ones.

``step``: BASELINE config 2's replayed training step (the batch of ``bench.make_batch``, ``TrainStepGraph``), locally conditioned
at hop 256 with 80 channels, then 83, then 80 again, in one process.  The spread of the two 80-channel passes stands next to
the difference, so that the difference can be told from the noise of the box.

Timing needs a GPU; there is no fallback.  No threshold is set: the file records what was measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def measure(a, torch):
    import numpy as np
    import bench
    from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, acoustic, features
    from wavenet_amd.wavenet import frames_needed

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def timed(fn, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        return stats([event_ms(fn) for _ in range(a.reps)])

    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0)}
    rs = np.random.RandomState(0)

    # ---- (a) the analyser call
    rate = 16000
    both = acoustic.MelPitch(rate)
    mel = features.LogMel(rate)
    t = np.arange(64 * rate) / float(rate)                  # 64 s: the first 60 are the one signal, all of it the 64 clips
    voice = 0.3 * sum(np.sin(2 * np.pi * h * (120.0 + 40.0 * np.sin(2 * np.pi * 0.5 * t)) * t) / h for h in (1, 2, 3))
    whole = torch.as_tensor((voice * (np.sin(2 * np.pi * 0.25 * t) > -0.3) + 0.01 * rs.standard_normal(t.size)).astype(np.float32)).cuda()
    inputs = (("one_60s_signal", [whole[:60 * rate].clone()]), ("64_clips_of_16000", [whole[i * 16000:(i + 1) * 16000].clone() for i in range(64)]))
    assert all(c.numel() == 16000 for c in inputs[1][1]) and inputs[0][1][0].numel() == 960000
    sec = {"rate": rate, "n_mels": both.n_mels, "hop": both.hop, "win": both.win, "fmin": both.pitch.fmin, "fmax": both.pitch.fmax,
           "tau_max": both.pitch.tau_max, "warmup": a.warmup,
           "timing": "device events around the whole batch call (launches, channel map and cats included); float32 inputs on the device"}
    for name, clips in inputs:
        row = {"clips": len(clips), "samples": int(sum(c.numel() for c in clips)),
               "columns": int(sum(features.frame_count(c.numel(), both.hop) for c in clips))}
        row["logmel_batch"] = timed(lambda: mel.batch(clips), a.warmup)
        row["mel_pitch_batch"] = timed(lambda: both.batch(clips), a.warmup)
        row["pitch_batch_alone"] = timed(lambda: both.pitch.batch(clips), a.warmup)
        row["mel_pitch_over_logmel"] = round(row["mel_pitch_batch"]["median_ms"] / row["logmel_batch"]["median_ms"], 3)
        row["extra_ms"] = round(row["mel_pitch_batch"]["median_ms"] - row["logmel_batch"]["median_ms"], 4)
        row["voiced_share"] = round(float((both.batch(clips[:1])[0][both.n_mels] == 1).float().mean()), 4)
        sec[name] = row
    res["analysis"] = sec

    # ---- (b) the replayed step: 80, 83, 80 channels
    step = {"workload": "BASELINE config 2, the batch of bench.make_batch, one replay of TrainStepGraph per step, locally conditioned",
            "local_hop": a.hop, "warmup": a.step_warmup, "order": [80, 83, 80],
            "timing": "device events around one replay; the three models one after another in one process"}
    passes = []
    for feats in step["order"]:
        net = FasterWaveNet(Params(bench.CFG2), seed=1234, local_channels=feats, local_hop=a.hop)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        B, T = int(x.shape[0]), int(x.shape[1])
        local = torch.as_tensor(rs.standard_normal((B, feats, frames_needed(T, a.hop))).astype(np.float32)).to(x.device)
        graph = TrainStepGraph(net, x, tgt, local=local)
        row = timed(graph.step, a.step_warmup)
        row.update(local_channels=feats, batch=[B, T], loss=float(graph.loss))
        passes.append(row)
        del graph, net
    step["passes"] = passes
    m80a, m83, m80b = (p["median_ms"] for p in passes)
    step["spread_of_the_two_80_channel_passes_ms"] = round(abs(m80a - m80b), 4)
    step["83_minus_mean_of_80_ms"] = round(m83 - 0.5 * (m80a + m80b), 4)
    step["83_over_80"] = round(m83 / (0.5 * (m80a + m80b)), 4)
    res["step"] = step
    res["unmeasured"] = ("whether F0 channels lower f0_rmse_cents of a copy synthesis: that needs a trained model and a corpus, and "
                         "neither was at hand")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5, help="untimed analyser calls before the timed ones")
    ap.add_argument("--step-warmup", type=int, default=65, help="untimed replays before the timed ones")
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_condition.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_pitch_condition.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    text = json.dumps(measure(a, torch), indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
