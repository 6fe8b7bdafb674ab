"""Updates per second of ``train --corpus`` from the command line, with ``--gpus`` off and on, on whatever the box has.

  python tools/time_dp_cli.py [--out profiles/dp_cli.json] [--timeout 600]

BASELINE config 2 (the 4 x 10 stack of 32 channels) at bench.py's shape, a global batch of 8 crops of 16,384 samples, on two
synthetic files of 4 seconds at 16 kHz.  A command's wall time holds its start-up (imports, the ranks' rendezvous, graph capture,
the checkpoints), so every configuration is run twice, with ``--repeat`` 100 and 1,100 -- 200 and 2,200 updates, the same number
of checkpoints -- and the rate is the 2,000 updates between them over the difference of the two wall times.  With one device the
``--gpus 2`` run is the rehearsal (WAVENET_DP_SHARE_GPU=1: both ranks on that device, gloo): it can only show the overhead of the
plumbing, never scaling.  With several, ``--gpus min(devices, 8)`` runs one rank per device over RCCL.  Every command is a child
process under ``--timeout`` seconds; one that fails ends the run.  The figures are merged into the output file under "timing";
what else the file holds (the tests' "largest_weight_difference") stays.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR, SECONDS, BATCH, T = 16000, 4, 8, 16384
REPEATS = (100, 1100)
N_FILES = 2


def _child(cmd, timeout, env=None):
    t0 = time.perf_counter()
    # a session of its own: at the time limit the launcher AND its ranks are ended, not the direct child alone
    child = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, env=env, start_new_session=True)
    try:
        out, err = child.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(child.pid, signal.SIGKILL)
        child.communicate()
        raise SystemExit("%s ran into its time limit of %d s: nothing more is started" % (" ".join(cmd[:4]), timeout))
    if child.returncode != 0:
        sys.stderr.write(out[-2000:] + err[-4000:])
        raise SystemExit("%s failed (%d): nothing more is started" % (" ".join(cmd[:4]), child.returncode))
    return time.perf_counter() - t0, out


def _rate(tmp, name, extra, timeout, env):
    import bench
    from wavenet_amd.train_audio.train import input_width_of
    from wavenet_amd import Params
    cfg = dict(bench.CFG2, sampling_rate=SR)
    tw = T - input_width_of(Params(cfg))
    wall = []
    for repeat in REPEATS:
        model = os.path.join(tmp, "%s_%d" % (name, repeat))
        os.makedirs(model)
        with open(os.path.join(model, "wavenet.json"), "w") as f:
            json.dump(cfg, f)
        cmd = [sys.executable, "-m", "wavenet_amd.train_audio.train", "-w", os.path.join(tmp, "wav"), "-m", model, "--corpus",
               "--seed", "1", "--batch-size", str(BATCH), "--train-width", str(tw), "--repeat", str(repeat), "--max-epoch", "2"] + extra
        wall.append(_child(cmd, timeout, env)[0])
        sys.stderr.write("%s --repeat %d: %.2f s\n" % (name, repeat, wall[-1]))
    updates = N_FILES * (REPEATS[1] - REPEATS[0])
    return {"wall_s": [round(w, 3) for w in wall], "updates_between": updates,
            "updates_per_s": round(updates / (wall[1] - wall[0]), 2), "batch": [BATCH, T]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_cli.json"))
    ap.add_argument("--timeout", type=int, default=600)
    a = ap.parse_args()
    import numpy as np
    from scipy.io import wavfile
    from wavenet_amd import data
    # the device count and name come from a child: this process starts launchers and keeps off the GPU itself
    _, out = _child([sys.executable, "-c", "import torch; print(torch.cuda.device_count()); "
                                           "print(torch.cuda.get_device_name(0) if torch.cuda.is_available() else '')"], a.timeout)
    count, device = int(out.splitlines()[0]), out.splitlines()[1]
    if count < 1:
        raise SystemExit("time_dp_cli.py needs a GPU")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "WAVENET_DP_SHARE_GPU"):
        env.pop(k, None)
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "wav"))
        for i, clip in enumerate(data.synthetic_waveform(N_FILES, SR * SECONDS, SR)):
            wavfile.write(os.path.join(tmp, "wav", "f%d.wav" % i), SR, np.round(clip * 32767).astype(np.int16))
        res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()), "devices": count, "device": device}
        res["gpus_off"] = _rate(tmp, "off", [], a.timeout, env)
        if count == 1:
            n, res["backend"] = 2, "gloo, both ranks on the one device (rehearsal: overhead only, no scaling)"
            env = dict(env, WAVENET_DP_SHARE_GPU="1")
        else:
            n, res["backend"] = min(count, 8), "nccl (RCCL), one rank per device"
        res["gpus"] = n
        res["gpus_on"] = _rate(tmp, "on", ["--gpus", str(n)], a.timeout, env)
    whole = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            whole = json.load(f)
    whole["timing"] = res
    line = json.dumps(whole, indent=1, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
