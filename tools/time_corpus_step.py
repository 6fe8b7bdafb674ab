"""Time one training update -- the draw of a batch of crops plus the replayed step -- with the per-file sampler
(``train_audio.train._Crops``: a handful of H2D copies and about ten torch indexing launches per draw) against the corpus
sampler (``wavenet_amd.Corpus``: one H2D copy of the draw table and one ``wn_corpus_gather`` launch), in the same process on
one box.

  python tools/time_corpus_step.py [--out profiles/corpus_sampler.json] [--timeout 300]

BASELINE config 2 at two shapes -- the command line's default (16 crops of input_width + 500) and bench.py's (8 x 16,384) --
unconditioned and with 80 feature channels at hop 256 in ``sample`` crop mode (a phase per crop).  The audio is synthetic: 8
files of 10 to 17 seconds at 16 kHz; ``_Crops`` holds the first one, the corpus all eight.  Per sampler, the wall time of
``draw(); graph.step(); synchronize()``: median of 200 updates behind 20 untimed ones ("update_ms"), the draw's own share up
to the moment it returns ("draw_host_ms": host time only, the launches are asynchronous), and the time per update of 200 more
run as the training loop runs them, with one synchronisation at the end ("loop_ms_per_update").  Order: per-file, corpus,
per-file again -- the spread between the two per-file passes is the noise floor the difference is to be read against.  Every
step runs in a child process of its own under ``--timeout`` seconds; a step that fails ends the run.  Needs a GPU; there is no
fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, HOP = 80, 256
REPS, WARMUP = 200, 20
STEPS = ("cli_default_plain", "cli_default_features", "bench_shape_plain", "bench_shape_features")


def _pass(draw, graph, torch):
    """-> the figures of one pass of REPS updates behind WARMUP untimed ones."""
    def update():
        t0 = time.perf_counter()
        x, tgt, lkw = draw()
        t1 = time.perf_counter()
        graph.step(x, tgt, **lkw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)

    for _ in range(WARMUP):
        update()
    ms = [update() for _ in range(REPS)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        x, tgt, lkw = draw()
        graph.step(x, tgt, **lkw)
    torch.cuda.synchronize()
    loop = 1e3 * (time.perf_counter() - t0) / REPS
    total = [m[0] for m in ms]
    return {"update_ms": round(statistics.median(total), 4), "update_ms_min": round(min(total), 4),
            "update_ms_max": round(max(total), 4), "draw_host_ms": round(statistics.median(m[1] for m in ms), 4),
            "loop_ms_per_update": round(loop, 4), "reps": REPS}


def step(name):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_corpus_step.py needs a GPU")
    import bench
    from wavenet_amd import Corpus, FasterWaveNet, Params, TrainStepGraph
    from wavenet_amd.corpus import columns_per_crop, silence_token
    from wavenet_amd.train_audio import local as L
    from wavenet_amd.train_audio.train import _Crops

    featured = name.endswith("_features")
    net = FasterWaveNet(Params(bench.CFG2), seed=1234, **(dict(local_channels=F, local_hop=HOP) if featured else {}))
    net.to_gpu()
    net.update_laerning_rate(0.001)
    iw = net.input_width
    B, tw = (16, 500) if name.startswith("cli_default") else (bench.B_PER_GPU, bench.T - iw)
    rs = np.random.RandomState(3)
    lengths = [160000 + 16000 * i for i in range(8)]
    tokens = [rs.randint(0, 256, size=n).astype(np.int32) for n in lengths]
    feats = [rs.standard_normal((F, -(-n // HOP))).astype(np.float32) for n in lengths] if featured else None

    fkw = {}
    if featured:
        ext, shift = L.padded(feats[0], iw, HOP)
        fkw = dict(features=ext, hop=HOP, shift=shift, crop="sample")
    crops = _Crops(np.concatenate([np.full((iw,), silence_token(256), dtype=np.int32), tokens[0]]), iw, tw, net.device, **fkw)
    corpus = Corpus(tokens, iw, 256, net.device, features=feats, hop=HOP if featured else 0)
    n_cols = columns_per_crop(iw, tw, HOP, "sample") if featured else None

    def per_file():
        d = crops.draw(B)
        return d[0], d[1], ({"local": d[2], "local_phase": d[3]} if featured else {})

    def across():
        x, tgt, local, _, phases = corpus.draw(B, tw, "sample", n_cols)
        return x, tgt, ({"local": local, "local_phase": phases} if featured else {})

    np.random.seed(0)
    x, tgt, lkw = per_file()
    graph = TrainStepGraph(net, x, tgt, **lkw)
    res = {"batch": [B, iw + tw], "input_width": iw, "feature_columns_per_crop": n_cols, "device": torch.cuda.get_device_name(0),
           "corpus_files": len(lengths), "corpus_device_bytes": corpus.device_bytes(),
           "per_file_device_bytes": int(crops.signal.numel()) * 4 + (int(crops.features.numel()) * 4 if featured else 0)}
    res["per_file_first_pass"] = _pass(per_file, graph, torch)
    res["corpus"] = _pass(across, graph, torch)
    res["per_file_second_pass"] = _pass(per_file, graph, torch)
    a, b, c = (res[k]["update_ms"] for k in ("per_file_first_pass", "per_file_second_pass", "corpus"))
    res["corpus_minus_per_file_ms"] = round(c - (a + b) / 2, 4)
    res["per_file_pass_spread_ms"] = round(abs(a - b), 4)
    a, b, c = (res[k]["loop_ms_per_update"] for k in ("per_file_first_pass", "per_file_second_pass", "corpus"))
    res["loop_corpus_minus_per_file_ms"] = round(c - (a + b) / 2, 4)
    res["loop_per_file_pass_spread_ms"] = round(abs(a - b), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corpus_sampler.json"))
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(step(a.child)))
        return
    res = {"protocol": " ".join(__doc__.split("\n\n")[2].split()), "features": {"channels": F, "hop": HOP, "crop": "sample"}}
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
