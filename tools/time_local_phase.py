"""What a feature phase per clip (``local_phase=`` a sequence; ``WnStackDesc.bias_phase_tab``) costs next to the one int
phase of a call, measured in the same run on the same box: the sibling of tools/time_local_interp.py, whose method it uses
(one process, device events, medians after warm-up).

  python tools/time_local_phase.py [--reps 20] [--warmup 65] [--commit ID] [--out profiles/local_phase.json]
  python tools/time_local_phase.py --isa-only [--isa-before DIR]                                             # no GPU

``step``: BASELINE config 2's step on the batch bench.py times (8 clips x 16,384, hop 256), locally conditioned, captured per
``local_interp`` mode from one seed three times -- int phase 0, a table of zeros, a table of random phases -- each a
TrainStepGraph with ``keep_graph=True`` so that its kernel nodes can be counted; the median (and minimum) of ``--reps``
replays after ``--warmup`` untimed ones.  All captures get the columns the worst phase needs, so they read the same block.
The comparison is against the int-phase step of the same run.

``forward_alone``: the inference-form stack forward (nothing saved, every layer its own launch; 40 layers at config 2) with
an int phase and with a table of random phases, as the sum of the ``wn_layer_fwd`` launches under
``wavenet_amd._lib.profile()``.

``isa``: VGPRs, SGPRs, scratch, occupancy and LDS of every kernel of the three translation units the feature touches, from
the compiler's resource-usage remarks; with ``--isa-before DIR`` (the parent's remarks as DIR/<unit>.txt) also whether every
instantiation the parent had is register-, scratch- and LDS-identical (``touched_instantiations`` lists the kernels that read
the phase, the parent's figures next to this tree's; ``new_instantiations`` the table forms of k_layer_fwd_h2_t1).  Timing needs a GPU; there is no fallback."""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_local_condition_step import REMARK_FLAGS, commit_id, stats      # noqa: E402
from time_local_interp import remark_table, remarks_now                    # noqa: E402

UNITS = ("mfma_layer", "generic_kernels", "wide_layer")
# the kernels that read the phase (every instantiation of each is listed in the file)
TOUCHED = ("k_layer_fwd_h2_t1", "k_layer_fwd_mfma32", "k_layer_fwd_mfma32_t1", "k_gate_fwd", "k_wide_gate", "k_colsum_per_frame",
           "k_colsum_per_frame_lerp")
FIELDS = ("vgprs", "agprs", "scratch_bytes", "lds_bytes", "occupancy_waves_per_simd")


def parent_name(name):
    """The name this tree gives an instantiation of the parent's: k_layer_fwd_h2_t1 gained a third template argument, "has a
    table", whose <false> form is the parent's kernel."""
    m = re.match(r"^(k_layer_fwd_h2_t1<\d+, \d+)>$", name)
    return m.group(1) + ", false>" if m else name


def isa_section(before_dir):
    sec = {"source": "wavenet_amd/csrc/{%s}.hip, hipcc %s" % (", ".join(UNITS), " ".join(REMARK_FLAGS[:-1])), "after": {}}
    same, touched, new = {}, {}, {}
    for unit in UNITS:
        after = remark_table(remarks_now(unit))
        sec["after"][unit] = after
        if before_dir:
            before = remark_table(open(os.path.join(before_dir, unit + ".txt")).read())
            sec.setdefault("before", {})[unit] = before
            twins = {parent_name(k): k for k in before}
            for twin, k in twins.items():
                same["%s: %s -> %s" % (unit, k, twin)] = twin in after and all(before[k][f] == after[twin][f] for f in FIELDS)
                if k.split("<")[0] in TOUCHED:
                    touched["%s: %s -> %s" % (unit, k, twin)] = {"parent": before[k], "now": after.get(twin)}
            new.update({"%s: %s" % (unit, k): v for k, v in after.items() if k not in twins})
    if before_dir:
        sec["existing_instantiations_unchanged"] = same
        sec["all_existing_unchanged"] = all(same.values())
        sec["touched_instantiations"] = touched
        sec["new_instantiations"] = new
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=65)
    ap.add_argument("--feats", type=int, default=80)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--isa-only", action="store_true", help="write the register table and stop (needs hipcc, no GPU)")
    ap.add_argument("--isa-before", default=None, metavar="DIR", help="the parent's resource-usage remarks, DIR/<unit>.txt")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_phase.json"))
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
            raise SystemExit("time_local_phase.py needs a GPU (or --isa-only)")
        if a.reps < 20:
            raise SystemExit("--reps must be at least 20")
        res.update(measure(a, torch))
    text = json.dumps(res, indent=1)
    print(text if not a.isa_only else json.dumps({"all_existing_unchanged": res["isa"].get("all_existing_unchanged"),
                                                  "changed": [k for k, v in res["isa"].get("existing_instantiations_unchanged",
                                                                                           {}).items() if not v]}, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


def measure(a, torch):
    import numpy as np
    import bench
    from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, _lib
    from wavenet_amd.wavenet import frames_needed

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "workload": "BASELINE config 2, the batch of bench.make_batch, locally conditioned, one replay of TrainStepGraph per step",
           "timing": "device events around one replay; the captures one after another in one process",
           "local_channels": a.feats, "local_hop": a.hop}
    step, fwd = {}, {}
    for interp in ("repeat", "linear"):
        net = FasterWaveNet(Params(bench.CFG2), seed=1234, local_channels=a.feats, local_hop=a.hop, local_interp=interp)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        B, T = int(x.shape[0]), int(x.shape[1])
        n = frames_needed(T, a.hop, a.hop - 1, interp)
        feats = torch.as_tensor(np.random.RandomState(1).standard_normal((B, a.feats, n)).astype(np.float32)).to(x.device)
        random = np.random.RandomState(2).randint(0, a.hop, size=B)
        phases = (("int_phase_0", 0), ("table_of_zeros", np.zeros(B, dtype=np.int64)), ("table_random", random))
        step[interp], fwd[interp] = {}, {}
        for name, ph in phases:
            graph = TrainStepGraph(net, x, tgt, keep_graph=True, local=feats, local_phase=ph)
            for _ in range(a.warmup):
                graph.step()
            torch.cuda.synchronize()
            step[interp][name] = stats([event_ms(graph.step) for _ in range(a.reps)])
            step[interp][name].update(kernel_nodes=graph.node_counts()["kernel"], step_plan=bool(graph._use_plan),
                                      loss=float(graph.loss), batch=[B, T])
            del graph
        base = step[interp]["int_phase_0"]["median_ms"]
        for name in ("table_of_zeros", "table_random"):
            step[interp][name]["over_int_phase"] = round(step[interp][name]["median_ms"] / base, 4)
        step[interp]["phases_of_table_random"] = [int(v) for v in random]
        t_off = T - int(tgt.shape[1])
        with torch.no_grad():
            c = net.forward_causal_block(x)
            for name, ph in (phases[0], phases[2]):
                for _ in range(3):
                    net.forward_residual_block(c, t_off=t_off, local=feats, local_phase=ph)
                fl = []
                for _ in range(a.reps):
                    with _lib.profile() as prof:
                        net.forward_residual_block(c, t_off=t_off, local=feats, local_phase=ph)
                        torch.cuda.synchronize()
                    fl.append(prof.result()["wn_layer_fwd"][1])
                fwd[interp][name] = stats(fl)
        fwd[interp]["table_over_int_phase"] = round(fwd[interp]["table_random"]["median_ms"] / fwd[interp]["int_phase_0"]["median_ms"], 4)
        fwd[interp]["layers"] = len(net._flat_layers)
        del net
    res["step"] = step
    res["forward_alone"] = dict(fwd, what="inference form (nothing saved), every layer its own launch, fp16x2: the k_layer_fwd_h2_t1 "
                                          "launches of the stack with the call's int phase and with a phase per clip")
    return res


if __name__ == "__main__":
    main()
