"""Gate-bias rows (conditioning) on the bf16-storage kernels: k16_fwd / k16_gate_bwd with rows, the row-gradient launch and the
way in through wn16_stack_fwd / wn16_stack_bwd and ``WaveNet.set_storage("bf16")``.  The six-layer model of
tests/test_gpu_bf16.py (128 channels, d = 1, 2, 4 twice) at ragged T below and above one 32-column tile; hops with several
frames inside a tile (5), a border inside a tile (48), the fine hop of U = 16 (16) and one beyond T (400); phases 0, hop - 1
and one per clip; both interpolation modes.  Bars: bit identities hold without tolerance; stored tensors against the
conditioned rounding oracle (tests/bf16_cond_ref.py) inside test_gpu_bf16.close_bf16's; row gradients against float64 sums of
the device's own [da | dg] inside (n + 4) 2^-24 sum |w v|, the bound of an fp32 sum of n terms with fp32 weights; the whole
model at test_gpu_bf16's bars (logits 2e-2, loss 1e-3, every gradient tensor 1e-2 in the 2-norm)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16_cond_ref as QC
from oracle import bf16_ref as Q
from oracle import wavenet_ref as R
from test_gpu_bf16 import SMALL, _live_bounds, _ws_views, close_bf16
from wavenet_amd import FasterWaveNet, Params, TrainStepGraph, WaveNet, WaveNetHipError, _lib
from wavenet_amd.wavenet import GateBiasRows, LocalPhases, _Stack16Fn, _to_btc, frames_needed

from gpu_util import dev, to_np

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64, 33), (2, 150, 90), (1, 333, 64)]
DIL = [1, 2, 4, 1, 2, 4]
_NETS = {}


def small_net():
    """(p, w, net): the six-layer model, built conditioned (so that it knows the layout of a row) and switched to bf16 storage;
    the stack tests hand it blocks of their own."""
    if "n" not in _NETS:
        p, w, net = build_cond(dict(condition_classes=5, condition_channels=8))
        net.set_storage("bf16")
        _NETS["n"] = (p, w, net)
    return _NETS["n"]


def run(net, idx, tw, block=None, hop=0, phase=0, interp=0, backward=True):
    """One stack call each way on a hand-made block: everything the tests look at, as numpy."""
    B, T = idx.shape
    c = net.forward_causal_block(dev(idx))
    blk = rows = None
    if block is not None:
        blk = dev(np.ascontiguousarray(block, np.float32)).requires_grad_(True)
        ph = LocalPhases(dev(np.asarray(phase, np.int32)), hop) if np.ndim(phase) else int(phase)
        rows = GateBiasRows(net, blk, hop, ph, interp)
    net._pack16_if_stale()
    out, skip = _Stack16Fn.apply(_to_btc(c), net._anchor, net, T - tw, True, blk, rows)
    x, xs, z, sk = net._last16
    r = dict(x=to_np(x.float()), xs=to_np(xs.float()), z=to_np(z.float()), skip=to_np(sk.float()))
    if not backward:
        return r
    net.zero_grads()
    (skip.float().square().sum() * 1e-3).backward()
    torch.cuda.synchronize()
    L = len(DIL)
    _, dadg, _ = _ws_views(net, L, B, T, tw)
    zero_g, live_g, _ = _live_bounds(DIL, T - tw)
    r.update(dadg=[to_np(dadg[l][:, zero_g[l]:].float()) for l in range(L)], zero_g=zero_g,
             grads=to_np(net._grad_arena).copy(), dblock=None if blk is None else to_np(blk.grad), rows=rows)
    return r


def bwd_rows_into(net, rows, B, T, tw, dskip, dblock):
    """wn16_stack_bwd through ctypes on the last forward's tensors: the row gradients accumulate into ``dblock``."""
    lib, L = _lib.lib(), len(DIL)
    x, xs, z, _ = net._last16
    desc, keep = rows.call16(B, T)
    gt = net._grad_tables()
    dbf, dbg = rows.grad_tables(dblock)
    dwf = (C.c_void_p * (2 * L))(*([gt["wf"][l] for l in range(L)] + [dbf[l] for l in range(L)]))
    dwg = (C.c_void_p * (2 * L))(*([gt["wg"][l] for l in range(L)] + [dbg[l] for l in range(L)]))
    nb = lib.wn16_stack_bwd_workspace_bytes(desc, B, T, T - tw)
    ws = torch.empty((nb,), device="cuda", dtype=torch.uint8)
    _lib.check(lib.wn16_stack_bwd(desc, _lib.ptr(net._pack16), _lib.ptr(x), _lib.ptr(xs), _lib.ptr(z), None, _lib.ptr(dskip), None,
                                  dwf, dwg, gt["wp"], gt["ws"], _lib.ptr(ws), nb, B, T, T - tw, 1, _lib.WN16_BWD_ROW_GRADS,
                                  _lib.stream_ptr()), "wn16_stack_bwd")
    torch.cuda.synchronize()
    return to_np(dblock)


def same(a, b, keys=("xs", "z", "skip", "grads")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k
    if "dadg" in a:
        for l, (u, v) in enumerate(zip(a["dadg"], b["dadg"])):
            assert u.tobytes() == v.tobytes(), ("dadg", l)


def block_for(rs, B, T, hop, worst, interp, R_=1536, scale=0.5):
    n = frames_needed(T, hop, worst, "linear" if interp else "repeat")
    return (rs.standard_normal((B, n, R_)) * scale).astype(np.float32)


# ---- 1. bit identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,tw", SHAPES)
def test_rows_of_zeros_equal_the_unconditioned_call_bit_for_bit(B, T, tw):
    _, _, net = small_net()
    idx = np.random.RandomState(T).randint(0, 256, (B, T)).astype(np.int32)
    base = run(net, idx, tw)
    same(run(net, idx, tw, np.zeros((B, 1536), np.float32)), base)
    for hop, ph, interp in ((5, 4, 0), (48, 0, 1), (400, list(range(B)), 1)):
        worst = hop - 1 if np.ndim(ph) else ph
        same(run(net, idx, tw, np.zeros((B, frames_needed(T, hop, worst, "linear" if interp else "repeat"), 1536), np.float32),
                 hop, ph, interp), base)


@pytest.mark.parametrize("hop,phase", [(5, 0), (48, 47), (16, 3)])
def test_equal_rows_inside_a_clip_equal_the_per_clip_call_and_a_table_of_one_phase_the_int(hop, phase):
    _, _, net = small_net()
    B, T, tw = 3, 64, 33
    rs = np.random.RandomState(hop)
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    row = (rs.standard_normal((B, 1536)) * 0.5).astype(np.float32)
    clip = run(net, idx, tw, row)
    for interp in (0, 1):
        n = frames_needed(T, hop, phase, "linear" if interp else "repeat")
        got = run(net, idx, tw, np.repeat(row[:, None, :], n, axis=1), hop, phase, interp)
        same(got, clip)
        blk = block_for(rs, B, T, hop, hop - 1, interp)
        a = run(net, idx, tw, blk[:, :n], hop, phase, interp)
        b = run(net, idx, tw, blk, hop, [phase] * B, interp)
        same(a, b)
        m = min(a["dblock"].shape[1], b["dblock"].shape[1])
        assert a["dblock"].tobytes() == np.ascontiguousarray(b["dblock"][:, :m]).tobytes()
        assert not b["dblock"][:, m:].any()                 # rows no position reaches


def test_distinct_phases_clip_by_clip_equal_single_clip_calls_and_two_runs_agree_in_every_bit():
    _, _, net = small_net()
    B, T, tw, hop = 2, 150, 90, 48
    rs = np.random.RandomState(7)
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    phases = [0, 47]
    for interp in (0, 1):
        blk = block_for(rs, B, T, hop, hop - 1, interp)
        both = run(net, idx, tw, blk, hop, phases, interp)
        again = run(net, idx, tw, blk, hop, phases, interp)
        same(both, again)
        assert both["dblock"].tobytes() == again["dblock"].tobytes()
        for b in range(B):
            n = frames_needed(T, hop, phases[b], "linear" if interp else "repeat")
            one = run(net, idx[b:b + 1], tw, blk[b:b + 1, :n], hop, phases[b], interp)
            for k in ("xs", "z"):
                assert both[k][:, b].tobytes() == one[k][:, 0].tobytes(), (k, b)
            assert both["skip"][b].tobytes() == one["skip"][0].tobytes()
            for l in range(len(DIL)):
                assert both["dadg"][l][b].tobytes() == one["dadg"][l][0].tobytes(), (l, b)


# ---- 2. forward against the oracle, teacher-forced per layer ---------------------------------------------------------------------
CASES = [(3, 64, 33, 0, 0, 0), (3, 64, 33, 5, [0, 4, 2], 1), (2, 150, 90, 48, 47, 0), (2, 150, 90, 48, [0, 47], 1),
         (1, 333, 64, 16, 15, 1), (1, 333, 64, 400, 0, 1), (2, 150, 90, 5, 0, 0)]


@pytest.mark.parametrize("B,T,tw,hop,phase,interp", CASES)
def test_forward_with_rows_against_the_conditioned_rounding_oracle(B, T, tw, hop, phase, interp):
    p, w, net = small_net()
    rs = np.random.RandomState(T + hop)
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    worst = hop - 1 if np.ndim(phase) else phase
    blk = block_for(rs, B, T, hop, worst, interp) if hop else (rs.standard_normal((B, 1536)) * 0.5).astype(np.float32)
    got = run(net, idx, tw, blk, hop, phase, interp, backward=False)
    rows = dict(block=blk, hop=hop, phase=phase, interp=interp, offsets=net._cond_offsets)
    y = QC.row_values(rows, B, T).astype(np.float64)
    lay = list(Q._layers(p))
    for l, (pre, d) in enumerate(lay):
        xin = (got["x"] if l == 0 else got["xs"][l - 1]).astype(np.float64)
        of, og = net._cond_offsets[l]
        zw, ow = QC.layer_fwd(xin, w[pre + "wf/W"], w[pre + "wg/W"], w[pre + "projection_block/W"], d, Q._Z(T, d, True),
                              y[:, :, of:of + 128], y[:, :, og:og + 128])
        close_bf16(got["z"][l], zw, "z of layer %d" % l, floor=0.05)
        close_bf16(got["xs"][l], ow, "output of layer %d" % l, floor=0.1)


# ---- 3. row gradients against float64 sums of the device's own [da | dg] ----------------------------------------------------------
@pytest.mark.parametrize("B,T,tw,hop,phase,interp", CASES)
def test_row_gradients_are_the_weighted_column_sums_of_the_stored_da_dg(B, T, tw, hop, phase, interp):
    p, w, net = small_net()
    rs = np.random.RandomState(T + 3 * hop)
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    worst = hop - 1 if np.ndim(phase) else phase
    blk = block_for(rs, B, T, hop, worst, interp) if hop else (rs.standard_normal((B, 1536)) * 0.5).astype(np.float32)
    got = run(net, idx, tw, blk, hop, phase, interp)
    rows = dict(block=blk, hop=hop, phase=phase, interp=interp, offsets=net._cond_offsets)
    j, alpha = QC.row_index(rows, B, T)
    dy, live = np.zeros((B, T, 1536)), np.zeros((B, T, 1536))
    for l, d in enumerate(DIL):
        lo = max(got["zero_g"][l], Q._Z(T, d, True))
        v = np.zeros((B, T, 256))
        v[:, got["zero_g"][l]:] = got["dadg"][l]
        v[:, :lo] = 0
        of, og = net._cond_offsets[l]
        dy[:, :, of:of + 128], dy[:, :, og:og + 128] = v[:, :, :128], v[:, :, 128:]
        live[:, lo:, of:of + 128] = live[:, lo:, og:og + 128] = 1.0
    want = QC.row_grads(rows, dy, B, T)
    mag = QC.row_grads(rows, np.abs(dy), B, T)              # sum |w v|: the weights are not negative
    n = QC.row_grads(dict(rows, interp=0), live, B, T)      # positions that contribute: the summed t of the row's frame ...
    if interp:
        n[:, 1:] += n[:, :-1].copy()                        # ... and of the frame before it
    bar = (n + 4) * 2.0 ** -24 * mag
    err = np.abs(got["dblock"].astype(np.float64) - want)
    assert (err <= bar).all(), (float(err.max()), float((err - bar).max()))
    assert not got["dblock"][mag == 0].any()                # rows (and columns) no live position reaches are exactly 0
    assert np.abs(got["dblock"]).max() > 0
    # += : a run into a prefilled block is float32(prefill + the zero-block run), one addition per element
    dskip = dev((rs.standard_normal((B, tw, 256)) * 1e-2).astype(np.float32)).to(torch.bfloat16)
    zero = bwd_rows_into(net, got["rows"], B, T, tw, dskip, torch.zeros(blk.shape, device="cuda"))
    pre = rs.standard_normal(blk.shape).astype(np.float32)
    filled = bwd_rows_into(net, got["rows"], B, T, tw, dskip, dev(pre))
    assert np.abs(zero).max() > 0
    assert filled.tobytes() == (pre + zero).astype(np.float32).tobytes()


# ---- 4. whole model through set_storage("bf16") ----------------------------------------------------------------------------------
FORMS = {
    "global": dict(condition_classes=5, condition_channels=8),
    "local repeat": dict(local_channels=6, local_hop=48),
    "local linear, a phase per clip": dict(local_channels=6, local_hop=48, local_interp="linear"),
    "local with U = 3": dict(local_channels=6, local_hop=48, local_upsample=3),
    "global + local": dict(condition_classes=5, condition_channels=8, local_channels=6, local_hop=5),
}


def build_cond(kw, cls=WaveNet, seed=9):
    p = R.make_params(**SMALL)
    w = R.init_weights(p, seed)
    net = cls(Params(p), seed=0, **kw)
    rs = np.random.RandomState(seed + 1)
    for ln in (net.global_condition_embed, net.global_condition_projection, net.local_condition_projection,
               net.local_condition_upsample):
        if ln is not None:
            w[ln.name + "/W"] = (rs.standard_normal(tuple(ln.W.shape)) * 0.3).astype(np.float32)
    net.load_state_dict(w)
    net.to_gpu()
    return p, w, net


@pytest.mark.parametrize("form", sorted(FORMS))
def test_conditioned_model_on_bf16_storage_against_the_oracle(form):
    kw = FORMS[form]
    p, w, net = build_cond(kw)
    net.set_storage("bf16")
    B, T, tw = 2, 150, 90
    rs = np.random.RandomState(len(form))
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    tgt = rs.randint(0, 256, (B, tw)).astype(np.int32)
    call = {}
    if kw.get("condition_classes"):
        call["condition"] = [3, 1]
    phase = 0
    if kw.get("local_channels"):
        phase = [7, 40] if "phase per clip" in form else (31 if kw.get("local_upsample") else 2)
        call["local"] = (rs.standard_normal((B, 6, T // kw["local_hop"] + 4)) * 0.7).astype(np.float32)
        call["local_phase"] = phase
    c = net.forward_causal_block(dev(idx))
    _, s = net.forward_residual_block(c, t_off=T - tw, **call)
    skip = net._last16[3]
    logits = net.forward_softmax_block(s, apply_softmax=False)
    loss = net.cross_entropy(logits, tgt)
    net.zero_grads()
    loss.backward()
    torch.cuda.synchronize()
    blk, leaves, how = QC.cond_block(kw, w, B, T, call.get("condition"), call.get("local"), phase)
    rows = dict(block=blk.detach().numpy().astype(np.float32), offsets=net._cond_offsets, **how)
    loss_ref, logits_ref, g, dblock = QC.train_step(p, w, idx, tgt, rows=rows, skip_override=to_np(skip.float()))
    blk.backward(torch.as_tensor(dblock))
    for name, leaf in leaves.items():
        g[name] = leaf.grad.numpy()
    np.testing.assert_allclose(to_np(logits)[:, :, 0, :].transpose(0, 2, 1), logits_ref, atol=2e-2)
    assert abs(float(loss.detach()) - loss_ref) < 1e-3
    seen = set()
    for ln, kind, off, n, shape in net._spans:
        k = "%s/%s" % (ln.name, kind)
        seen.add(k)
        want = np.asarray(g[k], np.float64).reshape(-1)
        got = to_np(net._grad_arena[off:off + n]).astype(np.float64)
        nw = np.linalg.norm(want)
        err = np.linalg.norm(got - want) / nw if nw > 0 else np.abs(got).max()
        assert err <= 1e-2, (form, k, err, nw)
        if "condition" in k:
            assert nw > 0, k
    assert set(leaves) <= seen


# ---- 5. the replayed step --------------------------------------------------------------------------------------------------------
def test_replayed_step_with_a_phase_refill_equals_the_eager_step_and_refuses_another_storage():
    from wavenet_amd.graph import default_loss
    kw = FORMS["local linear, a phase per clip"]
    B, T, tw = 2, 150, 90
    rs = np.random.RandomState(11)
    idx = rs.randint(0, 256, (B, T)).astype(np.int32)
    tgt = rs.randint(0, 256, (B, tw)).astype(np.int32)
    feats = (rs.standard_normal((B, 6, T // 48 + 4)) * 0.7).astype(np.float32)
    nets = []
    for _ in range(2):
        _, _, net = build_cond(kw)
        net.set_storage("bf16")
        net.update_laerning_rate(1e-3)
        nets.append(net)
    eager, graphed = nets
    x, t, f = dev(idx), dev(tgt), dev(feats)
    gr = TrainStepGraph(graphed, x, t, local=f, local_phase=[0, 0])
    lg = float(gr.step(local_phase=[5, 44]))
    le = default_loss(eager, x, t, local=f, local_phase=[5, 44])
    eager.backprop(le)
    torch.cuda.synchronize()
    assert lg == float(le.detach())
    np.testing.assert_array_equal(to_np(graphed._arena), to_np(eager._arena))
    graphed.set_storage("fp32")
    with pytest.raises(Exception, match="capture a new TrainStepGraph"):
        gr.step(local_phase=[5, 44])


# ---- 6. decoding -----------------------------------------------------------------------------------------------------------------
def test_conditioned_decoding_is_the_same_after_set_storage():
    kw = FORMS["global + local"]
    _, _, net = build_cond(kw, cls=FasterWaveNet)
    u = np.random.RandomState(2).random_sample(12)
    feats = (np.random.RandomState(3).standard_normal((6, 8)) * 0.7).astype(np.float32)
    a = to_np(net.generate(12, u, condition=2, local=feats))
    net.set_storage("bf16")
    b = to_np(net.generate(12, u, condition=2, local=feats))
    np.testing.assert_array_equal(a, b)


# ---- 7. refusals, each before any device work ------------------------------------------------------------------------------------
def test_refusals_through_ctypes():
    _, _, net = small_net()
    lib = _lib.lib()
    B, T, tw = 1, 64, 33
    L = len(DIL)
    blk = torch.zeros((B, 4, 1536), device="cuda")
    rows = GateBiasRows(net, blk, 16, 0, 0)
    net._pack16_if_stale()
    x = torch.zeros((B, T, 128), device="cuda", dtype=torch.bfloat16)
    xs = torch.full((L, B, T, 128), 7.0, device="cuda", dtype=torch.bfloat16)
    z, skip = torch.zeros_like(xs), torch.zeros((B, tw, 256), device="cuda", dtype=torch.bfloat16)
    ptr, sp = _lib.ptr, _lib.stream_ptr

    def fwd(edit):
        desc, keep = rows.call16(B, T)
        edit(keep[0], keep)
        rc = lib.wn16_stack_fwd(desc, ptr(net._pack16), ptr(x), ptr(xs), ptr(z), ptr(skip), B, T, T - tw, 1, sp())
        return rc, lib.wn_last_error().decode()

    alive = []

    def shifted(keep, by):
        t = (C.c_void_p * L)(*[keep[1][l] + by for l in range(L)])
        keep[0].bf = C.cast(t, C.POINTER(C.c_void_p))
        alive.append(t)

    def mixed(keep):
        t = (C.c_void_p * L)(*[keep[2][l] if l else None for l in range(L)])
        keep[0].bg = C.cast(t, C.POINTER(C.c_void_p))
        alive.append(t)

    cases = [
        (lambda d, k: shifted(k, 4), "16-byte aligned"),
        (lambda d, k: mixed(k), "NULL and non-NULL"),
        (lambda d, k: setattr(d, "bias_frame_stride", 1538), "multiple of 4"),
        (lambda d, k: setattr(d, "bias_phase", 16), "bias_phase"),
        (lambda d, k: (setattr(d, "bias_hop", 0), setattr(d, "bias_interp", 1)), "bias_interp"),
        (lambda d, k: (setattr(d, "bias_phase", 3), setattr(d, "bias_phase_tab", blk.data_ptr())), "bias_phase_tab"),
    ]
    for edit, word in cases:
        rc, msg = fwd(edit)
        assert rc == _lib.WN_EARG and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert float(xs.float().min()) == 7.0                  # nothing ran
    gt = net._grad_tables()
    dskip = torch.ones_like(skip)
    net.zero_grads()
    dblk = torch.full_like(blk, 3.0)                       # the gradient rows the tables point at
    marks = []

    def bwd(desc, flags, dwf, dwg):
        nb = lib.wn16_stack_bwd_workspace_bytes(desc, B, T, T - tw)
        ws = torch.full((max(nb, 1),), 0x5A, device="cuda", dtype=torch.uint8)
        marks.append(ws)
        rc = lib.wn16_stack_bwd(desc, ptr(net._pack16), ptr(x), ptr(xs), ptr(z), None, ptr(dskip), None, dwf, dwg, gt["wp"],
                                gt["ws"], ptr(ws), nb, B, T, T - tw, 1, flags, sp())
        return rc, lib.wn_last_error().decode()

    desc, keep = rows.call16(B, T)
    two = lambda t, r: (C.c_void_p * (2 * L))(*([t[l] for l in range(L)] + [r[l] for l in range(L)]))
    for d_, flags, word in ((net._stack_desc(), _lib.WN16_BWD_ROW_GRADS, "no gate-bias rows"), (desc, 0, "WN16_BWD_ROW_GRADS"),
                            (desc, 3, "unknown bits"), (net._stack_desc(), 2, "unknown bits")):
        dbf, dbg = rows.grad_tables(dblk)
        rc, msg = bwd(d_, flags, two(gt["wf"], dbf), two(gt["wg"], dbg))
        assert rc == _lib.WN_EARG and word in msg, (rc, msg, word)
    torch.cuda.synchronize()                               # nothing ran: no gradient, no gradient row, no workspace byte moved
    assert not to_np(net._grad_arena).any()
    assert float(dblk.min()) == 3.0 and float(dblk.max()) == 3.0
    for ws in marks:
        assert int(ws.min()) == 0x5A and int(ws.max()) == 0x5A
