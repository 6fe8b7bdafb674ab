"""What local conditioning (WaveNet(..., local_channels, local_hop)) costs a replayed training step, next to the
unconditioned and the globally conditioned step of the same box and tree.

  python tools/time_local_condition_step.py [--reps 20] [--warmup 65] [--commit ID] [--out profiles/local_condition.json]
  python tools/time_local_condition_step.py --isa-only [--isa-before BEFORE.txt --isa-after AFTER.txt]     # no GPU

One process: BASELINE config 2's step on the batch bench.py times (``bench.make_batch``), captured three times from one seed
-- unconditioned, globally conditioned (``--classes`` speakers, ``--channels`` embedding channels), locally conditioned
(``--feats`` feature channels at ``--hop`` samples per column) -- each as a TrainStepGraph with ``keep_graph=True`` so that
its kernel nodes can be counted.  Each figure is the median (and the minimum) of ``--reps`` replays timed with device
events after ``--warmup`` untimed ones.

``column_sum``: the stack backward of the two conditioned models op by op under ``wavenet_amd._lib.profile()`` (device events
around the per-layer backward launches, ``wn_layer_bwd``).  The globally conditioned model runs k_colsum_per_clip, the locally
conditioned one k_colsum_per_frame, and that ONE launch per layer is all that differs between their per-layer backwards -- so
the difference of the two, divided by the number of layers, is what the per-frame form saves per layer.  (The library
exports no entry point that runs a column sum alone, and gains none for a measurement.)

``forward_alone``: the inference-form stack forward (nothing saved, every layer its own launch) of the same two models,
fp16x2: k_layer_fwd_h2_t1<0, kCondClip> against k_layer_fwd_h2_t1<0, kCondFrame>.

``decode``: ``generate_batch`` with 64 utterances x 2,000 samples of the 2 x 8-layer 64/64/128 model of
profiles/batched_decode_any_shape.json, without and with a frame table (``--feats`` channels at ``--hop``; every utterance
is given the same features, so that both calls run one prefill), timed with device events: the whole call, the prefill
alone (a call that emits one sample), and their difference -- the decode launch.

``isa``: VGPRs, scratch and occupancy of every fused forward instantiation from the compiler's resource-usage remarks
(``hipcc -Rpass-analysis=kernel-resource-usage`` over csrc/mfma_layer.hip, saved to the two text files), before and after.
Timing needs a GPU; there is no fallback."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DECODE_MODEL = dict(quantization_steps=256, causal_conv_channels=[64], residual_conv_channels=[64] * 8, residual_num_blocks=2,
                    softmax_conv_channels=[128, 256])
REMARK_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c"]


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def demangle(name):
    """k_layer_fwd_*<template arguments> from the mangled name (ints as they stand, bools as true / false)."""
    k = re.match(r"_ZN2wn\d+(k_layer_fwd_\w+?)I((?:L[ib]\d+E)+)E", name)
    if not k:
        return None
    args = ", ".join(("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", k.group(2)))
    return "%s<%s>" % (k.group(1), args)


def remark_table(text):
    """{kernel: {"vgprs", "agprs", "sgprs", "scratch_bytes", "occupancy_waves_per_simd", "lds_bytes"}} from the remarks."""
    keys = {"SGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"remark: (?:[^ ]*: )?\s*(Function Name|[A-Za-z ]+(?: \[[^\]]+\])?): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = demangle(m.group(2))
            cur = out.setdefault(name, {}) if name else None
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return dict(sorted(out.items()))


def remarks_now():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "wavenet_amd", "csrc", "mfma_layer.hip")
    r = subprocess.run([hipcc] + REMARK_FLAGS + ["-I" + os.path.join(ROOT, "include"), src, "-o", os.devnull],
                       capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("hipcc failed:\n" + r.stderr[-2000:])
    return r.stderr + r.stdout


def isa_section(before_path, after_path):
    after = remark_table(open(after_path).read() if after_path else remarks_now())
    sec = {"source": "wavenet_amd/csrc/mfma_layer.hip, hipcc " + " ".join(REMARK_FLAGS[:-1]), "after": after}
    if before_path:
        before = remark_table(open(before_path).read())
        sec["before"] = before
        # the parent's k_layer_fwd_h2_t1<SAVE, false / true> are this tree's <SAVE, 0 / 1> (kCondNone / kCondClip)
        same = {}
        for name, row in before.items():
            m = re.match(r"^(k_layer_fwd_h2_t1<\d+), (true|false)>$", name)
            twin = "%s, %d>" % (m.group(1), 1 if m.group(2) == "true" else 0) if m else name
            # ... and its exact-fp32 k_layer_fwd_mfma32*<SAVE, HAS_BIAS> are <SAVE, HAS_BIAS, false> (FRAME off)
            twin = re.sub(r"^(k_layer_fwd_mfma32(?:_t1)?<\d+, (?:true|false))>$", r"\1, false>", twin)
            same[name + " -> " + twin] = twin in after and all(row[k] == after[twin][k] for k in ("vgprs", "scratch_bytes", "lds_bytes"))
        sec["registers_scratch_and_lds_unchanged"] = same
    sec["exact_fp32_per_frame_instantiations"] = {k: v for k, v in after.items() if k.endswith(", true, true>")}
    frame = {k: v for k, v in after.items() if re.match(r"k_layer_fwd_h2_t1<\d+, 2>", k)}
    sec["per_frame_mode"] = {"instantiations": frame, "scratch_free": all(v["scratch_bytes"] == 0 for v in frame.values()),
                             "vgprs": sorted({v["vgprs"] for v in frame.values()}),
                             "occupancy_waves_per_simd": sorted({v["occupancy_waves_per_simd"] for v in frame.values()}),
                             "frame_index": "one 32-bit integer division per lane ((tc + phase) / hop), kept: no reciprocal multiply"}
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=65)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--feats", type=int, default=80)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--isa-only", action="store_true", help="write the register table and stop (needs hipcc, no GPU)")
    ap.add_argument("--isa-before", default=None, metavar="BEFORE.txt", help="the parent's resource-usage remarks")
    ap.add_argument("--isa-after", default=None, metavar="AFTER.txt", help="this tree's remarks (default: compile now)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_condition.json"))
    a = ap.parse_args()
    res = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            res = json.load(f)                                 # the two halves are written by two runs: keep the other one
    if a.isa_only:
        res["isa"] = isa_section(a.isa_before, a.isa_after)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_local_condition_step.py needs a GPU (or --isa-only)")
        if a.reps < 20:
            raise SystemExit("--reps must be at least 20")
        res.update(measure(a, torch))
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


def measure(a, torch):
    import numpy as np
    import bench
    from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, _lib
    from wavenet_amd.graph import default_loss
    from wavenet_amd.wavenet import frames_needed

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "workload": "BASELINE config 2, the batch of bench.make_batch, one replay of TrainStepGraph per step",
           "timing": "device events around one replay; the three models one after another in one process",
           "condition_classes": a.classes, "condition_channels": a.channels, "local_channels": a.feats, "local_hop": a.hop}
    rs = np.random.RandomState(0)
    ops = {}
    modes = (("unconditioned", {}), ("globally_conditioned", dict(condition_classes=a.classes, condition_channels=a.channels)),
             ("locally_conditioned", dict(local_channels=a.feats, local_hop=a.hop)))
    for name, kw in modes:
        net = FasterWaveNet(Params(bench.CFG2), seed=1234, **kw)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        B, T = int(x.shape[0]), int(x.shape[1])
        call = {}
        if "condition_classes" in kw:
            call["condition"] = torch.as_tensor(np.arange(B) % a.classes).to(x.device)
        if "local_channels" in kw:
            call["local"] = torch.as_tensor(rs.standard_normal((B, a.feats, frames_needed(T, a.hop))).astype(np.float32)).to(x.device)
        graph = TrainStepGraph(net, x, tgt, keep_graph=True, **call)
        for _ in range(a.warmup):
            graph.step()
        torch.cuda.synchronize()
        res[name] = stats([event_ms(graph.step) for _ in range(a.reps)])
        res[name]["kernel_nodes"] = graph.node_counts()["kernel"]
        res[name]["arena_floats"] = int(net._arena.numel())
        res[name]["step_plan"] = bool(graph._use_plan)
        res[name]["loss"] = float(graph.loss)
        res[name]["batch"] = [B, T]
        del graph
        if call:
            # the conditioned stack op by op: its per-layer backward launches (the only launch that differs between the two
            # conditioned models is the column sum) and its inference-form layer launches
            t_off = T - int(tgt.shape[1])
            for _ in range(3):
                net.zero_grads()
                default_loss(net, x, tgt, **call).backward()
            layers, whole = [], []
            for _ in range(a.reps):
                net.zero_grads()
                loss = default_loss(net, x, tgt, **call)
                with _lib.profile() as prof:
                    whole.append(event_ms(loss.backward))
                layers.append(prof.result()["wn_layer_bwd"][1])
            ops[name] = {"layer_backward_launches": stats(layers), "whole_backward": stats(whole)}
            with torch.no_grad():
                c = net.forward_causal_block(x)
                for _ in range(3):
                    net.forward_residual_block(c, t_off=t_off, **call)
                fl = []
                for _ in range(a.reps):
                    with _lib.profile() as prof:
                        net.forward_residual_block(c, t_off=t_off, **call)
                        torch.cuda.synchronize()
                    fl.append(prof.result()["wn_layer_fwd"][1])
                ops[name]["forward_layer_launches"] = stats(fl)
            ops["layers"] = len(net._flat_layers)
            ops["frames_per_clip"] = frames_needed(T, a.hop)
        del net
    base = res["unconditioned"]["median_ms"]
    for name in ("globally_conditioned", "locally_conditioned"):
        res[name]["over_unconditioned"] = round(res[name]["median_ms"] / base, 4)
        res[name]["extra_kernel_nodes"] = res[name]["kernel_nodes"] - res["unconditioned"]["kernel_nodes"]
    res["bench_workload_kernel_nodes"] = res["unconditioned"]["kernel_nodes"]
    g, l = ops["globally_conditioned"], ops["locally_conditioned"]
    d = g["layer_backward_launches"]["median_ms"] - l["layer_backward_launches"]["median_ms"]
    res["column_sum"] = {
        "what": ("the per-layer backward launches of the stack (wn_layer_bwd), op by op, fp16x2: per layer k_layer_bwd_p1, the "
                 "fixed-order tile sum, k_layer_bwd_p2 and ONE column-sum launch -- k_colsum_per_clip (B x 2 cd / 64 workgroups) for "
                 "the globally conditioned model, k_colsum_per_frame (B x frames x 2 cd / 64) for the locally conditioned one; "
                 "nothing else differs, so the difference divided by the layers is what the per-frame form saves per layer"),
        "per_clip_rows": {k: g[k] for k in ("layer_backward_launches", "whole_backward")},
        "per_frame_rows": {k: l[k] for k in ("layer_backward_launches", "whole_backward")},
        "layers": ops["layers"], "frames_per_clip": ops["frames_per_clip"], "saved_per_layer_ms": round(d / ops["layers"], 5)}
    res["forward_alone"] = {
        "what": ("inference form (nothing saved), every layer its own launch, fp16x2: k_layer_fwd_h2_t1<0, kCondClip> (globally "
                 "conditioned) against k_layer_fwd_h2_t1<0, kCondFrame> (locally conditioned)"),
        "per_clip_rows": g["forward_layer_launches"], "per_frame_rows": l["forward_layer_launches"]}

    # ---- decode: 64 utterances x 2,000 samples, without and with a frame table
    dec = {"model": DECODE_MODEL, "utterances": a.utterances, "samples": a.samples, "reps": 5,
           "timing": ("device events around generate_batch, after one untimed call: the whole call (one prefill over the window, then "
                      "the decode launch), and a call that emits ONE sample per utterance (the prefill alone, no decode launch); "
                      "decode_ms is the difference of the medians and samples/s counts the decoded samples over it")}
    u = rs.random_sample((a.utterances, a.samples))
    for label, kw in (("without_table", {}), ("with_table", dict(local_channels=a.feats, local_hop=a.hop))):
        net = FasterWaveNet(Params(DECODE_MODEL), seed=1234, **kw)
        net.to_gpu()
        call = {}
        if kw:
            n = frames_needed(net.input_width + a.samples, a.hop)
            call["local"] = rs.standard_normal((a.feats, n)).astype(np.float32)      # one array for all: ONE prefill, as without
        last = [None]

        def run(n_samples):
            last[0] = net.generate_batch(n_samples, u[:, :n_samples], **call)
        run(a.samples)
        whole = [event_ms(lambda: run(a.samples)) for _ in range(5)]
        checksum = int(last[0].sum().item())
        run(1)
        pre = [event_ms(lambda: run(1)) for _ in range(5)]
        ms = statistics.median(whole) - statistics.median(pre)
        dec[label] = {"whole_call": stats(whole), "prefill_only": stats(pre), "decode_ms": round(ms, 3),
                      "decoded_samples_per_s": round(a.utterances * (a.samples - 1) / (ms * 1e-3), 1), "token_checksum": checksum}
        del net
    dec["with_over_without"] = round(dec["with_table"]["decoded_samples_per_s"] / dec["without_table"]["decoded_samples_per_s"], 4)
    res["decode"] = dec
    return res


if __name__ == "__main__":
    main()
