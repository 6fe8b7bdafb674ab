"""What a learned upsampling layer ahead of the local projection (``local_upsample`` = U) costs, measured in one process on one
box with U = 1 -- no layer -- as the baseline of the same run: the sibling of tools/time_local_interp.py, whose method it uses
(device events, medians after warm-up).

  python tools/time_local_upsample.py [--reps 20] [--warmup 30] [--factors 1,4,16] [--out profiles/local_upsample.json]

Model: BASELINE config 2, 80 feature channels at hop 256, ``local_interp="linear"``; U = 4 and 16 run the projection, the layer
kernels and the column sums at hop 64 and 16.

``step``: the step on the batch bench.py times, a TrainStepGraph (``keep_graph=True``: its kernel nodes are counted) per U, all
captured first and then replayed in turn -- round r times U = 1, 4, 16 one after another -- so that drift of the box lands on
all of them; median (and minimum, maximum) of ``--reps`` replays after ``--warmup`` untimed ones each.

``column_sum``: the per-layer backward launches (``wn_layer_bwd``) of an op-by-op backward under ``wavenet_amd._lib.profile()``.
The one launch per layer whose work changes with U is the weighted column sum (k_colsum_per_frame_lerp: about U times the
workgroups on U times shorter segments), so the difference to U = 1 divided by the layers is what it costs per layer.

``upsample_and_projection``: device events around the nodes ahead of the stack alone -- layer, cut, projection (forward), and
their backward from a random block gradient -- with the block's size in MB.

``decode``: ``generate_batch`` with 28 utterances on config 4's shape (the specialised decoder) with a table at hop H' = 256 / U:
the whole call, the prefill alone (a call that emits one sample each), and samples per second of the difference.

Timing needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_local_condition_step import commit_id, stats      # noqa: E402

CFG4 = dict(quantization_steps=256, causal_conv_channels=[32], residual_conv_channels=[32] * 10, residual_num_blocks=4,
            softmax_conv_channels=[256, 256])
BATCH = 28                       # wn_decoder_batch_max() on the nine-workgroup form: one launch


def measure(a, torch):
    import numpy as np
    import bench
    from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, _lib
    from wavenet_amd.graph import default_loss
    from wavenet_amd.wavenet import coarse_frames_needed, frames_needed

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    factors = [int(v) for v in a.factors.split(",")]
    if factors[0] != 1:
        raise SystemExit("--factors starts with 1, the baseline of the run")
    res = {"commit": a.commit or commit_id(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup,
           "workload": "BASELINE config 2, the batch of bench.make_batch, local_interp = linear",
           "timing": "device events; every U in one process, the replayed steps timed in turn (round r: every U once)",
           "local_channels": a.feats, "local_hop": a.hop, "factors": factors}

    def model(cfg, U):
        kw = dict(local_channels=a.feats, local_hop=a.hop, local_interp="linear")
        if U > 1:
            kw["local_upsample"] = U
        net = FasterWaveNet(Params(cfg), seed=1234, **kw)
        net.to_gpu()
        net.update_laerning_rate(0.001)
        return net

    # ---- the replayed step, every U captured, then timed in turn -------------------------------------------------------------
    nets, graphs, calls, step = {}, {}, {}, {}
    for U in factors:
        net = nets[U] = model(bench.CFG2, U)
        x, tgt = bench.make_batch(0, 1, net.input_width)
        B, T = int(x.shape[0]), int(x.shape[1])
        n = coarse_frames_needed(T, a.hop, U, 0, "linear")
        feats = np.random.RandomState(1).standard_normal((B, a.feats, frames_needed(T, a.hop, 0, "linear") + 1)).astype(np.float32)
        calls[U] = dict(x=x, tgt=tgt, local=torch.as_tensor(feats[:, :, :n]).to(x.device))
        graphs[U] = TrainStepGraph(net, x, tgt, keep_graph=True, local=calls[U]["local"])
        for _ in range(a.warmup):
            graphs[U].step()
        torch.cuda.synchronize()
    times = {U: [] for U in factors}
    for _ in range(a.reps):
        for U in factors:
            times[U].append(event_ms(graphs[U].step))
    for U in factors:
        net, g = nets[U], graphs[U]
        T = int(calls[U]["x"].shape[1])
        fine = a.hop // U
        rows = frames_needed(T, fine, 0, "linear")
        step[str(U)] = dict(stats(times[U]), kernel_nodes=g.node_counts()["kernel"], step_plan=bool(g._use_plan), loss=float(g.loss),
                            fine_hop=fine, coarse_columns=int(calls[U]["local"].shape[2]), rows_per_clip=rows,
                            block_mb=round(int(calls[U]["x"].shape[0]) * rows * net._cond_rows * 4 / 1e6, 2))
        step[str(U)]["over_u1"] = round(step[str(U)]["median_ms"] / step["1"]["median_ms"], 4)
    res["step"] = step
    graphs.clear()

    # ---- op by op: the per-layer backward launches, and the nodes ahead of the stack ------------------------------------------
    colsum, ahead = {}, {}
    for U in factors:
        net, c = nets[U], calls[U]
        x, tgt, kw = c["x"], c["tgt"], dict(local=c["local"])
        T = int(x.shape[1])
        for _ in range(3):
            net.zero_grads()
            default_loss(net, x, tgt, **kw).backward()
        layers, whole = [], []
        for _ in range(a.reps):
            net.zero_grads()
            loss = default_loss(net, x, tgt, **kw)
            with _lib.profile() as prof:
                whole.append(event_ms(loss.backward))
            layers.append(prof.result()["wn_layer_bwd"][1])
        colsum[str(U)] = {"layer_backward_launches": stats(layers), "whole_backward": stats(whole)}

        def forward():
            f, _, _ = net._stack_features(c["local"], 0, T)
            return net._local_block(f).contiguous()
        blk = forward()
        dblk = torch.randn_like(blk)
        fw, bw = [], []
        for i in range(a.reps + 3):
            net.zero_grads()
            hold = [None]

            def run():
                hold[0] = forward()
            t_f = event_ms(run)
            t_b = event_ms(lambda: hold[0].backward(dblk))
            if i >= 3:
                fw.append(t_f)
                bw.append(t_b)
        ahead[str(U)] = {"forward": stats(fw), "backward": stats(bw), "block_shape": list(blk.shape),
                         "block_mb": round(blk.numel() * 4 / 1e6, 2)}
        del blk, dblk
    L = len(nets[1]._flat_layers)
    for U in factors[1:]:
        d = colsum[str(U)]["layer_backward_launches"]["median_ms"] - colsum["1"]["layer_backward_launches"]["median_ms"]
        colsum[str(U)]["extra_per_layer_ms"] = round(d / L, 5)
    colsum["layers"] = L
    colsum["what"] = ("the per-layer backward launches of the stack (wn_layer_bwd), op by op, fp16x2; the launch per layer whose work "
                      "changes with U is the weighted column sum, so the difference to U = 1 divided by the layers is its extra cost")
    res["column_sum"] = colsum
    ahead["what"] = ("device events around layer + cut + projection alone (forward), and around their backward from a random block "
                     "gradient; U = 1: the projection alone")
    res["upsample_and_projection"] = ahead
    nets.clear()
    calls.clear()

    # ---- generate_batch on config 4's shape ---------------------------------------------------------------------------------
    dec = {"model": "BASELINE config 4 (4 x 10 layers of 32 channels, head 256 -> 256)", "utterances": BATCH, "samples": a.samples,
           "reps": a.decode_reps,
           "timing": ("device events around generate_batch, after one untimed call: the whole call, and a call that emits ONE sample "
                      "per utterance (the prefill alone, table build included); decode_ms is the difference of the medians")}
    u = np.random.RandomState(0).random_sample((BATCH, a.samples))
    for U in factors:
        net = model(CFG4, U)
        n = coarse_frames_needed(net.input_width + a.samples - 1, a.hop, U, 0, "linear")
        call = {"local": np.random.RandomState(2).standard_normal((a.feats, n)).astype(np.float32)}
        last = [None]

        def run(n_samples):
            last[0] = net.generate_batch(n_samples, u[:, :n_samples], **call)
        run(a.samples)
        whole = [event_ms(lambda: run(a.samples)) for _ in range(a.decode_reps)]
        checksum = int(last[0].sum().item())
        run(1)
        pre = [event_ms(lambda: run(1)) for _ in range(a.decode_reps)]
        ms = statistics.median(whole) - statistics.median(pre)
        dec[str(U)] = {"whole_call": stats(whole), "prefill_only": stats(pre), "decode_ms": round(ms, 3), "frame_hop": a.hop // U,
                       "decoded_samples_per_s": round(BATCH * (a.samples - 1) / (ms * 1e-3), 1),
                       "samples_per_s_whole_call": round(BATCH * a.samples / (statistics.median(whole) * 1e-3), 1),
                       "token_checksum": checksum}
        net.close()
        del net
    for U in factors[1:]:
        dec[str(U)]["over_u1"] = round(dec[str(U)]["decoded_samples_per_s"] / dec["1"]["decoded_samples_per_s"], 4)
    res["decode"] = dec
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--factors", default="1,4,16")
    ap.add_argument("--feats", type=int, default=80)
    ap.add_argument("--hop", type=int, default=256)
    ap.add_argument("--samples", type=int, default=4000)
    ap.add_argument("--decode-reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="recorded in the file (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_upsample.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_local_upsample.py needs a GPU")
    if a.reps < 10:
        raise SystemExit("--reps must be at least 10")
    res = measure(a, torch)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
