"""What conditioning costs a replayed training step on bf16 storage (BASELINE config 5: 4 x 10 layers, 128 / 512 channels, the
batch bench.py times: 8 x 16,384 samples), and what ``set_storage("bf16")`` brings a conditioned 128-channel model.

  python tools/time_bf16_condition_step.py [--reps 20] [--warmup 10] [--parent-lib LIB.so] [--out profiles/bf16_condition.json]
  python tools/time_bf16_condition_step.py --isa-only [--parent-src DIR/w16_layer.hip]          # no GPU

Every case runs in a process of its own (the library is chosen when the package is imported: ``WAVENET_HIP_LIB``), one after
the other on one box: a TrainStepGraph captured with ``keep_graph=True`` so that its kernel nodes can be counted, ``--warmup``
untimed replays, then the median (minimum, maximum) of ``--reps`` replays timed with device events.

``unconditioned``: this tree's library, and -- with ``--parent-lib`` -- two passes of the parent commit's: this tree must lie
inside the spread of the parent's own two passes (the unconditioned instantiations are the kernels they were).
``conditioned``: global (16 speakers, 32 channels); local at hop 256 (80 feature channels) in repeat and in linear mode; local
linear with a phase per clip -- each on bf16 storage and, the same model, on fp32 storage (what a user had until now).
``row_gradients``: the one launch per backward that sums the gate-row gradients, from ``wavenet_amd._lib.profile()`` (device
events around the launch) in an op-by-op step.
``isa``: registers, scratch and spills of every k16_fwd / k16_gate_bwd instantiation from a cross-compile, parent against
this tree; both kernels take their LDS dynamically, so the code objects record none: ``lds_bytes`` evaluates kFwdLds / kGateLds
from the ``static constexpr int`` lines of the source that was compiled (w16.hpp beside it).  Timing needs a GPU; there is no fallback."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG5 = dict(quantization_steps=256, causal_conv_channels=[128], residual_conv_channels=[128] * 10, residual_num_blocks=4,
            softmax_conv_channels=[512, 256])
CASES = {
    "unconditioned": {},
    "global": dict(condition_classes=16, condition_channels=32),
    "local_repeat": dict(local_channels=80, local_hop=256),
    "local_linear": dict(local_channels=80, local_hop=256, local_interp="linear"),
    "local_linear_phase_per_clip": dict(local_channels=80, local_hop=256, local_interp="linear"),
}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def run_case(name, storage, reps, warmup):
    import numpy as np
    import torch
    from bench import make_batch
    from oracle import wavenet_ref as R
    from wavenet_amd import Params, TrainStepGraph, WaveNet, _lib
    from wavenet_amd.graph import default_loss
    from wavenet_amd.wavenet import frames_needed
    kw = CASES[name]
    net = WaveNet(Params(R.make_params(**CFG5)), seed=1, **kw)
    net.to_gpu()
    net.set_storage(storage)
    net.update_laerning_rate(1e-4)
    x, tgt = make_batch(0, 1, net.input_width)
    B, T = x.shape
    call = {}
    rs = np.random.RandomState(0)
    if kw.get("condition_classes"):
        call["condition"] = torch.as_tensor(rs.randint(0, kw["condition_classes"], B)).cuda()
    if kw.get("local_channels"):
        n = frames_needed(T, kw["local_hop"], kw["local_hop"] - 1, kw.get("local_interp", "repeat"))
        call["local"] = torch.as_tensor(rs.standard_normal((B, kw["local_channels"], n)).astype(np.float32)).cuda()
        call["local_phase"] = [int(v) for v in rs.randint(0, kw["local_hop"], B)] if name.endswith("per_clip") else 0
    graph = TrainStepGraph(net, x, tgt, keep_graph=True, **call)
    for _ in range(warmup):
        graph.step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss = graph.step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    res = dict(stats(ms), kernel_nodes=graph.node_counts()["kernel"], loss=float(loss), storage=storage,
               library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH))
    if storage == "bf16" and kw:
        with _lib.profile() as prof:
            net.backprop(default_loss(net, x, tgt, **call))
            torch.cuda.synchronize()
        rep = prof.result()                                  # {scope: (calls, total_ms, min_ms, ...)}
        for key, scope in (("row_gradients_ms", "wn16_row_grads"), ("layer_bwd_ms", "wn16_layer_bwd"),
                           ("conv_wgrad_ms", "wn16_conv_wgrad"), ("layer_fwd_ms", "wn16_layer_fwd")):
            res[key] = round(rep[scope][1], 4) if scope in rep else None
    print("RESULT " + json.dumps(res))


def child(name, storage, a, lib=None):
    env = dict(os.environ)
    if lib:
        env["WAVENET_HIP_LIB"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--storage", storage, "--reps", str(a.reps),
                        "--warmup", str(a.warmup)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    if r.returncode != 0:
        raise SystemExit("case %s (%s) failed with %d:\n%s" % (name, storage, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("RESULT ")][-1][7:])


def short_name(mangled):
    """k16_fwd<MODE> / k16_gate_bwd<HAS_DO, HAS_DZ, MODE> from the mangled name (MODE 0 none, 1 per clip, 2 per frame, 3 linear;
    a parent kernel has no MODE)."""
    base = "k16_fwd" if "k16_fwd" in mangled else "k16_gate_bwd"
    m = re.search(base + r"I((?:L[bi]\d+E)+)E", mangled)
    return base + ("<%s>" % ", ".join(re.findall(r"L[bi](\d+)E", m.group(1))) if m else "")


def resources(src):
    """{kernel: {vgprs, agprs, scratch_bytes, spills}} of every k16_fwd / k16_gate_bwd in a cross-compile of ``src``."""
    out = os.path.join(tempfile.mkdtemp(), "k.s")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-inline-asm",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "wavenet_amd", "csrc"), "-S", "--cuda-device-only",
                    "-o", out, src], check=True, capture_output=True)
    text = open(out).read()
    res = {}
    for m in re.finditer(r"- \.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+)"
                         r".*?\.vgpr_spill_count:\s+(\d+)", text, re.S):
        name = m.group(2)
        if "k16_fwd" in name or "k16_gate_bwd" in name:
            res[short_name(name)] = dict(vgprs=int(m.group(4)), agprs=int(m.group(1)),
                                                                  scratch_bytes=int(m.group(3)), spills=int(m.group(5)))
    return res


def lds_bytes(src):
    """{"k16_fwd": kFwdLds, "k16_gate_bwd": kGateLds} evaluated from the constants of ``src`` and the w16.hpp beside it."""
    env = {}
    for path in (os.path.join(os.path.dirname(src), "w16.hpp"), src):
        for name, expr in re.findall(r"static constexpr int (\w+) = ([^;]+);", open(path).read()):
            try:
                env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
            except Exception:
                pass
    return {"k16_fwd": env["kFwdLds"], "k16_gate_bwd": env["kGateLds"]}


def isa(parent_src):
    src = os.path.join(ROOT, "wavenet_amd", "csrc", "w16_layer.hip")
    sec = {"this_tree": resources(src), "lds_bytes": {"this_tree": lds_bytes(src)}}
    if parent_src:
        sec["parent"] = resources(parent_src)
        sec["lds_bytes"]["parent"] = lds_bytes(parent_src)
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--case")
    ap.add_argument("--storage", default="bf16")
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-src")
    ap.add_argument("--isa-only", action="store_true")
    ap.add_argument("--no-fp32", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_condition.json"))
    a = ap.parse_args()
    if a.case:
        return run_case(a.case, a.storage, a.reps, a.warmup)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.isa_only:
        doc["isa"] = isa(a.parent_src)
    else:
        un = {"this_tree": child("unconditioned", "bf16", a)}
        if a.parent_lib:
            un["parent_pass_1"] = child("unconditioned", "bf16", a, a.parent_lib)
            un["this_tree_again"] = child("unconditioned", "bf16", a)
            un["parent_pass_2"] = child("unconditioned", "bf16", a, a.parent_lib)
        doc["shape"] = "config 5, 8 x 16384"
        doc["unconditioned"] = un
        doc["conditioned"] = {}
        for name in CASES:
            if name == "unconditioned":
                continue
            ent = {"bf16": child(name, "bf16", a)}
            if not a.no_fp32:
                ent["fp32"] = child(name, "fp32", a)
                ent["fp32_over_bf16"] = round(ent["fp32"]["median_ms"] / ent["bf16"]["median_ms"], 3)
            ent["bf16_over_unconditioned"] = round(ent["bf16"]["median_ms"] / un["this_tree"]["median_ms"], 3)
            doc["conditioned"][name] = ent
            print(name, json.dumps(ent), flush=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
