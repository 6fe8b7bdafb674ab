"""What linear interpolation between feature frames (``local_interp="linear"``) costs next to repeat mode, measured in the
same run on the same box: the sibling of tools/time_local_condition_step.py, whose method it uses (one process, device
events, medians after warm-up).

  python tools/time_local_interp.py [--reps 20] [--warmup 65] [--commit ID] [--out profiles/local_interp.json]
  python tools/time_local_interp.py --isa-only [--isa-before DIR]                                             # no GPU

``step``: BASELINE config 2's step on the batch bench.py times, captured three times from one seed -- unconditioned,
locally conditioned in repeat mode, locally conditioned in linear mode -- each a TrainStepGraph with ``keep_graph=True`` so
that its kernel nodes can be counted; the median (and minimum) of ``--reps`` replays after ``--warmup`` untimed ones.

``forward_alone``: the inference-form stack forward (nothing saved, every layer its own launch; 40 layers at config 2) of
the two conditioned models, fp16x2: k_layer_fwd_h2_t1<0, kCondFrame> against k_layer_fwd_h2_t1<0, kCondLinear>, as the sum
of the ``wn_layer_fwd`` launches under ``wavenet_amd._lib.profile()``.

``column_sum``: the per-layer backward launches (``wn_layer_bwd``) of the two models op by op.  The ONE launch per layer that
differs is the column sum -- k_colsum_per_frame against k_colsum_per_frame_lerp -- so the difference divided by the layers is
what the weighted form costs per layer.

``decode``: ``generate_batch`` with 64 utterances x 2,000 samples of the 2 x 8-layer 64/64/128 model with a frame table, in
both modes: the whole call, the prefill alone (a call that emits one sample), and their difference -- the decode launch.

``isa``: VGPRs, SGPRs, scratch, occupancy and LDS of every kernel of the four translation units the feature touches, from
the compiler's resource-usage remarks; with ``--isa-before DIR`` (the parent's remarks as DIR/<unit>.txt) also whether every
instantiation the parent had is register-, scratch- and LDS-identical.  Timing needs a GPU; there is no fallback."""
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

from time_local_condition_step import DECODE_MODEL, REMARK_FLAGS, commit_id, stats      # noqa: E402

UNITS = ("mfma_layer", "generic_kernels", "wide_layer", "decoder")


def demangle(name):
    """kernel<template arguments> of a ``wn::`` kernel from its mangled name (ints as they stand, bools as true / false)."""
    m = re.match(r"_ZN2wn(\d+)", name)
    if not m:
        return None
    n = int(m.group(1))
    rest = name[m.end():]
    base, rest = rest[:n], rest[n:]
    t = re.match(r"I((?:L[ib]\d+E)+)E", rest)
    if not t:
        return base
    args = ", ".join(("true" if v == "1" else "false") if k == "b" else v for k, v in re.findall(r"L([ib])(\d+)E", t.group(1)))
    return "%s<%s>" % (base, args)


def remark_table(text):
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"remark:\s+(Function Name|[A-Za-z ]+(?: \[[^\]]+\])?): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = demangle(m.group(2))
            cur = out.setdefault(name, {}) if name else None
        elif cur is not None and m.group(1) in keys:
            cur[keys[m.group(1)]] = int(m.group(2))
    return dict(sorted(out.items()))


def remarks_now(unit):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "wavenet_amd", "csrc", unit + ".hip")
    r = subprocess.run([hipcc] + REMARK_FLAGS + ["-Wno-inline-asm", "-I" + os.path.join(ROOT, "include"), src, "-o", os.devnull],
                       capture_output=True, text=True)
    if r.returncode:
        raise SystemExit("hipcc failed:\n" + r.stderr[-2000:])
    return r.stderr + r.stdout


def parent_name(name):
    """The name this tree gives an instantiation of the parent's: the exact-fp32 kernels' FRAME became an int mode (false /
    true -> 0 / 1), and k_wide_gate, k_gate_fwd, k_decode and k_decode_batch became templates whose <false> form is the parent's kernel."""
    m = re.match(r"^(k_layer_fwd_mfma32(?:_t1)?<\d+, (?:true|false)), (true|false)>$", name)
    if m:
        return "%s, %d>" % (m.group(1), 1 if m.group(2) == "true" else 0)
    if name in ("k_wide_gate", "k_gate_fwd", "k_decode", "k_decode_batch"):
        return name + "<false>"
    return name


def isa_section(before_dir):
    sec = {"source": "wavenet_amd/csrc/{%s}.hip, hipcc %s" % (", ".join(UNITS), " ".join(REMARK_FLAGS[:-1])), "after": {}}
    same, new = {}, {}
    for unit in UNITS:
        after = remark_table(remarks_now(unit))
        sec["after"][unit] = after
        if before_dir:
            before = remark_table(open(os.path.join(before_dir, unit + ".txt")).read())
            sec.setdefault("before", {})[unit] = before
            twins = {parent_name(k): k for k in before}
            for twin, k in twins.items():
                same["%s: %s -> %s" % (unit, k, twin)] = twin in after and all(
                    before[k][f] == after[twin][f] for f in ("vgprs", "agprs", "scratch_bytes", "lds_bytes", "occupancy_waves_per_simd"))
            new.update({"%s: %s" % (unit, k): v for k, v in after.items() if k not in twins})
    if before_dir:
        sec["existing_instantiations_unchanged"] = same
        sec["all_existing_unchanged"] = all(same.values())
        sec["new_instantiations"] = new
        sec["new_instantiations_scratch_free"] = all(v["scratch_bytes"] == 0 for v in new.values())
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=65)
    ap.add_argument("--feats", type=int, default=80)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--isa-only", action="store_true", help="write the register table and stop (needs hipcc, no GPU)")
    ap.add_argument("--isa-before", default=None, metavar="DIR", help="the parent's resource-usage remarks, DIR/<unit>.txt")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_interp.json"))
    a = ap.parse_args()
    res = {}
    if os.path.isfile(a.out):
        with open(a.out) as f:
            res = json.load(f)                                 # the two halves are written by two runs: keep the other one
    if a.isa_only:
        res["isa"] = isa_section(a.isa_before)
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("time_local_interp.py needs a GPU (or --isa-only)")
        if a.reps < 20:
            raise SystemExit("--reps must be at least 20")
        res.update(measure(a, torch))
    text = json.dumps(res, indent=1)
    print(text if not a.isa_only else json.dumps({k: res["isa"].get(k) for k in ("all_existing_unchanged", "new_instantiations",
                                                                                 "new_instantiations_scratch_free")}, indent=1))
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
           "local_channels": a.feats, "local_hop": a.hop}
    rs = np.random.RandomState(0)
    ops, step = {}, {}
    modes = (("unconditioned", None), ("repeat", "repeat"), ("linear", "linear"))
    for name, interp in modes:
        kw = {} if interp is None else dict(local_channels=a.feats, local_hop=a.hop, local_interp=interp)
        net = FasterWaveNet(Params(bench.CFG2), seed=1234, **kw)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        B, T = int(x.shape[0]), int(x.shape[1])
        call = {}
        if interp is not None:
            # both modes get the columns linear mode needs (repeat mode ignores the surplus one): the same features
            feats = np.random.RandomState(1).standard_normal((B, a.feats, frames_needed(T, a.hop, 0, "linear"))).astype(np.float32)
            call["local"] = torch.as_tensor(feats).to(x.device)
        graph = TrainStepGraph(net, x, tgt, keep_graph=True, **call)
        for _ in range(a.warmup):
            graph.step()
        torch.cuda.synchronize()
        step[name] = stats([event_ms(graph.step) for _ in range(a.reps)])
        step[name].update(kernel_nodes=graph.node_counts()["kernel"], step_plan=bool(graph._use_plan), loss=float(graph.loss),
                          batch=[B, T])
        del graph
        if call:
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
            ops["rows_per_clip"] = {"repeat": frames_needed(T, a.hop), "linear": frames_needed(T, a.hop, 0, "linear")}
        del net
    for name in ("repeat", "linear"):
        step[name]["over_unconditioned"] = round(step[name]["median_ms"] / step["unconditioned"]["median_ms"], 4)
    step["linear_over_repeat"] = round(step["linear"]["median_ms"] / step["repeat"]["median_ms"], 4)
    res["step"] = step
    r, l = ops["repeat"], ops["linear"]
    res["forward_alone"] = {
        "what": ("inference form (nothing saved), every layer its own launch, fp16x2: the %d k_layer_fwd_h2_t1<0, kCondFrame> launches "
                 "(repeat) against the %d k_layer_fwd_h2_t1<0, kCondLinear> launches (linear)" % (ops["layers"], ops["layers"])),
        "repeat": r["forward_layer_launches"], "linear": l["forward_layer_launches"],
        "linear_over_repeat": round(l["forward_layer_launches"]["median_ms"] / r["forward_layer_launches"]["median_ms"], 4)}
    d = l["layer_backward_launches"]["median_ms"] - r["layer_backward_launches"]["median_ms"]
    res["column_sum"] = {
        "what": ("the per-layer backward launches of the stack (wn_layer_bwd), op by op, fp16x2; the one launch per layer that "
                 "differs is the column sum: k_colsum_per_frame (B x frames x 2 cd / 64 workgroups) against k_colsum_per_frame_lerp "
                 "(B x (frames + 1) x 2 cd / 64, two weighted segments each), so the difference divided by the layers is what the "
                 "weighted form costs per layer"),
        "repeat": {k: r[k] for k in ("layer_backward_launches", "whole_backward")},
        "linear": {k: l[k] for k in ("layer_backward_launches", "whole_backward")},
        "layers": ops["layers"], "rows_per_clip": ops["rows_per_clip"], "extra_per_layer_ms": round(d / ops["layers"], 5)}

    dec = {"model": DECODE_MODEL, "utterances": a.utterances, "samples": a.samples, "reps": 5,
           "timing": ("device events around generate_batch, after one untimed call: the whole call, and a call that emits ONE sample "
                      "per utterance (the prefill alone); decode_ms is the difference of the medians")}
    u = rs.random_sample((a.utterances, a.samples))
    for interp in ("repeat", "linear"):
        net = FasterWaveNet(Params(DECODE_MODEL), seed=1234, local_channels=a.feats, local_hop=a.hop, local_interp=interp)
        net.to_gpu()
        n = frames_needed(net.input_width + a.samples, a.hop, 0, "linear")
        call = {"local": np.random.RandomState(2).standard_normal((a.feats, n)).astype(np.float32)}
        last = [None]

        def run(n_samples):
            last[0] = net.generate_batch(n_samples, u[:, :n_samples], **call)
        run(a.samples)
        whole = [event_ms(lambda: run(a.samples)) for _ in range(5)]
        checksum = int(last[0].sum().item())
        run(1)
        pre = [event_ms(lambda: run(1)) for _ in range(5)]
        ms = statistics.median(whole) - statistics.median(pre)
        dec[interp] = {"whole_call": stats(whole), "prefill_only": stats(pre), "decode_ms": round(ms, 3),
                       "decoded_samples_per_s": round(a.utterances * (a.samples - 1) / (ms * 1e-3), 1), "token_checksum": checksum}
        del net
    dec["linear_over_repeat"] = round(dec["linear"]["decoded_samples_per_s"] / dec["repeat"]["decoded_samples_per_s"], 4)
    res["decode"] = dec
    return res


if __name__ == "__main__":
    main()
