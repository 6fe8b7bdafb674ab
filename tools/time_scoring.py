"""Time the two forms of per-sample scoring: the fused row form of the head (wn_head_xent under WN_EXEC_HEAD_ROW_NLL) against
the fallback (wn_pointwise_fwd, then logsumexp - gather in torch).

  python tools/time_scoring.py [--reps 30] [--warmup 3] [--samples 1000000] [--commit ID] [--out profiles/scoring.json]

Two measurements, one process, the two forms alternating inside every repetition so that both see the same drift of the box:
  head   BASELINE config 2's head shape alone: 131,072 rows, 256 -> 256, ReLU, bias; rows in, per-row NLL out
  score  WaveNet.score of a synthetic signal (two sines + noise, mu-law) on config 2's topology (4 x 10 layers of 32
         channels, head [256, 256]) with the default knobs, net.fuse_head_loss on and off
Each figure is the median (and the minimum) of ``--reps`` repetitions timed with device events after ``--warmup`` untimed ones.
The two forms' results are compared before anything is timed.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np      # noqa: E402
import torch            # noqa: E402

CFG2 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10,
            residual_num_blocks=4, softmax_conv_channels=[256, 256])


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(forms, warmup, reps):
    """{name: [ms, ...]}: every repetition runs each form once, in turn."""
    for _ in range(warmup):
        for _, fn in forms:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:
            ms[name].append(event_ms(fn))
    return ms


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoring.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_scoring.py needs a GPU")
    if a.reps < 20:
        raise SystemExit("--reps must be at least 20")
    from wavenet_amd import Params, WaveNet, _lib, data
    from wavenet_amd._lib import check, ptr
    lib = _lib.lib()
    net = WaveNet(Params(CFG2), seed=1234)
    net.to_gpu()
    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "timing": "device events, the two forms alternating in one process"}

    # ---- the head alone ----
    N, Cin, Q = 131072, 256, 256
    rs = np.random.RandomState(0)
    x = torch.as_tensor(rs.standard_normal((N, Cin)).astype(np.float32)).cuda()
    tgt = torch.as_tensor(rs.randint(0, Q, N).astype(np.int32)).cuda()
    lay = net.softmax_conv_layers[-1]
    with torch.no_grad():
        lay.b.copy_(torch.as_tensor(rs.standard_normal(Q).astype(np.float32) * 0.3))
    rows = torch.empty((N,), device="cuda")
    loss = torch.empty((_lib.XENT_LOSS_WORDS,), device="cuda")
    logits = torch.empty((N, Q), device="cuda")
    lab = tgt.to(torch.int64).unsqueeze(1)
    out = {}

    def head_fused():
        check(lib.wn_head_xent(ptr(x), ptr(lay.W), ptr(lay.b), ptr(tgt), ptr(loss), ptr(rows), N, Cin, Q, _lib.WN_ACT_RELU, 0,
                               net._exec(call_flags=_lib.WN_EXEC_HEAD_ROW_NLL), _lib.stream_ptr()), "wn_head_xent")

    def head_fallback():
        check(lib.wn_pointwise_fwd(ptr(x), ptr(lay.W), ptr(lay.b), ptr(logits), N, Cin, Q, _lib.WN_ACT_RELU, net._exec(),
                                   _lib.stream_ptr()), "wn_pointwise_fwd")
        out["rows"] = torch.logsumexp(logits, dim=1) - logits.gather(1, lab).squeeze(1)

    head_fused()
    head_fallback()
    torch.cuda.synchronize()
    res["head"] = {"rows": N, "cin": Cin, "cout": Q, "max_abs_difference_of_the_forms": float((rows - out["rows"]).abs().max())}
    for name, ms in alternate([("fused_rows", head_fused), ("fallback", head_fallback)], a.warmup, a.reps).items():
        res["head"][name] = stats(ms)

    # ---- WaveNet.score ----
    wave = data.synthetic_waveform(1, a.samples, 16000)[0]
    tokens = torch.as_tensor(data.mulaw_encode(wave, 256).astype(np.int32)).cuda()
    got = {}

    def scorer(fused):
        def run():
            net.fuse_head_loss = fused
            got[fused] = net.score(tokens)
        return run

    scorer(True)()
    scorer(False)()
    torch.cuda.synchronize()
    res["score"] = {"samples": a.samples, "chunk_width": 16384, "batch_size": 8,
                    "max_abs_difference_of_the_forms": float((got[True] - got[False]).abs().max()),
                    "nats_per_sample": float(got[True].double().mean())}
    for name, ms in alternate([("fused_rows", scorer(True)), ("fallback", scorer(False))], a.warmup, a.reps).items():
        res["score"][name] = stats(ms)
        res["score"][name]["samples_per_s"] = round(a.samples / (res["score"][name]["median_ms"] * 1e-3), 1)
    for key in ("head", "score"):
        res[key]["fused_over_fallback_median"] = round(res[key]["fused_rows"]["median_ms"] / res[key]["fallback"]["median_ms"], 4)
    res["fused_is_default"] = bool(res["head"]["fused_over_fallback_median"] < 1.0 and res["score"]["fused_over_fallback_median"] < 1.0)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
