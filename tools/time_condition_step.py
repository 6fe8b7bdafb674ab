"""What global conditioning (WaveNet(..., condition_classes, condition_channels)) costs a replayed training step.

  python tools/time_condition_step.py [--reps 20] [--warmup 65] [--commit ID] [--out profiles/global_condition.json]
  python tools/time_condition_step.py --isa-only [--isa-before PARENT.s]        # no GPU: the register counts alone

One process, one box: BASELINE config 2's step on the batch bench.py times (``bench.make_batch``), captured twice from one
seed -- unconditioned, then conditioned on ``--classes`` speakers through ``--channels`` embedding channels -- each as a
TrainStepGraph with ``keep_graph=True`` so that its kernel nodes can be counted.  Each figure is the median (and the minimum)
of ``--reps`` replays timed with device events after ``--warmup`` untimed ones.  What to expect from the code: the
unconditioned step runs its layers in grouped forward launches and ONE multi-layer backward launch; the conditioned step
runs every layer as its own forward launch (the COND form of k_layer_fwd_h2_t1) and takes the per-layer backward (three
launches per layer plus the per-clip column sum), so it is slower by an amount this file reports and does not guess.
Bringing conditioning into the chained backward is the follow-up that number justifies or not.

The conditioned stack forward is also timed by itself, op by op under ``wavenet_amd._lib.profile()`` (device events around
the layer launches, ``wn_layer_fwd``): the fp16x2 COND kernels against the exact-fp32 biased kernels the same call takes
under bf16x3 arithmetic.

``isa``: registers and scratch bytes of the fused forward kernels from the gfx950 disassembly of csrc/mfma_layer.hip (what
tools/isa_waits.py reads) -- the unconditioned instantiations must be what they were in the parent (``--isa-before`` parses a
parent build's assembly into the same table).  The off figure means something only next to the on figure of the same run.
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


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except Exception:
        return "unknown"


def isa_table(lines):
    """{kernel: {"vgprs", "agpr_offset", "sgprs", "scratch_bytes", "lds_bytes"}} of the fused forward kernels, names demangled
    by hand (template arguments kept as the mangled name spells them)."""
    text = "\n".join(lines)
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        name, body = m.group(1), m.group(2)
        k = re.match(r"_ZN2wn\d+(k_layer_fwd_\w+?)I((?:L[ib]\d+E)+)E", name)
        if not k:
            continue
        args = ", ".join(("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", k.group(2)))
        get = lambda key: int(re.search(r"\.amdhsa_" + key + r"\s+(\d+)", body).group(1))
        out["%s<%s>" % (k.group(1), args)] = {"vgprs": get("next_free_vgpr"), "agpr_offset": get("accum_offset"),
                                             "sgprs": get("next_free_sgpr"), "scratch_bytes": get("private_segment_fixed_size"),
                                             "lds_bytes": get("group_segment_fixed_size")}
    return dict(sorted(out.items()))


def isa_section(before_path):
    import isa_waits
    now = isa_table(isa_waits.assembly(os.path.join(ROOT, "wavenet_amd", "csrc", "mfma_layer.hip")))
    sec = {"source": "wavenet_amd/csrc/mfma_layer.hip, hipcc -O3 --offload-arch=gfx950 -S", "kernels": now}
    if before_path:
        before = isa_table(open(before_path).read().split("\n"))
        # the parent's k_layer_fwd_h2_t1<SAVE> is this tree's k_layer_fwd_h2_t1<SAVE, false>
        same = {}
        for name, row in before.items():
            twin = re.sub(r"^(k_layer_fwd_h2_t1<\d+)>$", r"\1, false>", name)
            same[twin] = {k: row[k] for k in ("vgprs", "scratch_bytes", "lds_bytes")} == \
                {k: now[twin][k] for k in ("vgprs", "scratch_bytes", "lds_bytes")} if twin in now else False
        sec["parent_kernels"] = before
        # (the biased exact-fp32 instantiations <., true> gained the clip stride: they are listed, not required to be equal)
        sec["unconditioned_instantiations_unchanged"] = all(v for k, v in same.items() if "true" not in k)
        sec["unchanged_by_kernel"] = same
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=65)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--channels", type=int, default=16)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--isa-only", action="store_true", help="write the register table and stop (needs hipcc, no GPU)")
    ap.add_argument("--isa-before", default=None, metavar="PARENT.s", help="assembly of the parent's mfma_layer.hip to compare with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_condition.json"))
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
            raise SystemExit("time_condition_step.py needs a GPU (or --isa-only)")
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

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "workload": "BASELINE config 2, the batch of bench.make_batch, one replay of TrainStepGraph per step",
           "timing": "device events around one replay; unconditioned, then conditioned, in one process",
           "condition_classes": a.classes, "condition_channels": a.channels}
    for name, on in (("unconditioned", False), ("conditioned", True)):
        kw = dict(condition_classes=a.classes, condition_channels=a.channels) if on else {}
        net = FasterWaveNet(Params(bench.CFG2), seed=1234, **kw)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        ids = torch.as_tensor(np.arange(x.shape[0]) % a.classes).to(x.device) if on else None
        graph = TrainStepGraph(net, x, tgt, keep_graph=True, condition=ids)
        for _ in range(a.warmup):
            graph.step()
        torch.cuda.synchronize()
        res[name] = stats([event_ms(graph.step) for _ in range(a.reps)])
        res[name]["kernel_nodes"] = graph.node_counts()["kernel"]
        res[name]["arena_floats"] = int(net._arena.numel())
        res[name]["step_plan"] = bool(graph._use_plan)
        res[name]["loss"] = float(graph.loss)
        if on:
            # the conditioned stack forward by itself, op by op: the layer launches of the fp16x2 COND kernels against the
            # exact-fp32 biased kernels (bf16x3 arithmetic takes them)
            fwd = {}
            with torch.no_grad():
                c = net.forward_causal_block(x)
                for prec in ("fp16x2", "bf16x3"):
                    net.gemm_precision = prec
                    for _ in range(3):
                        net.forward_residual_block(c, t_off=x.shape[1] - tgt.shape[1], condition=ids)
                    layers, whole = [], []
                    for _ in range(a.reps):
                        with _lib.profile() as prof:
                            whole.append(event_ms(lambda: net.forward_residual_block(c, t_off=x.shape[1] - tgt.shape[1], condition=ids)))
                        layers.append(prof.result()["wn_layer_fwd"][1])
                    fwd[prec] = {"layer_launches": stats(layers), "stack_forward_with_skip_sum": stats(whole)}
                net.gemm_precision = None
            fwd["what"] = ("inference form (nothing saved), every layer its own launch: fp16x2 = k_layer_fwd_h2_t1<0, COND>, "
                           "bf16x3 = k_layer_fwd_mfma32_t1<0, HAS_BIAS> seeded with the clip's row")
            res["conditioned_forward_alone"] = fwd
        del graph, net
    d = res["conditioned"]["median_ms"] - res["unconditioned"]["median_ms"]
    res["difference_of_medians_ms"] = round(d, 4)
    res["conditioned_over_unconditioned"] = round(res["conditioned"]["median_ms"] / res["unconditioned"]["median_ms"], 4)
    res["extra_kernel_nodes"] = res["conditioned"]["kernel_nodes"] - res["unconditioned"]["kernel_nodes"]
    return res


if __name__ == "__main__":
    main()
