"""The channel GEMMs of the C ABI against float64: every entry point, arithmetic mode and dispatch branch.

Each case is a table entry with a one-line reason that names the branch of launch_colgemm / launch_colgemm_b3 / launch_wgrad
(mfma_gemm.hip, mfma_gemm_b3.hip) or of the bf16-storage launchers (w16_api.hip, w16_gemm.hip) it reaches.  Every case runs
in fp32, bf16x3, bf16 and fp16x2 and once under WN_EXEC_FORCE_GENERIC, and every comparison is against the float64 reference
of tests/channel_gemm_ref.py (WN_GEMM_BF16 and wn16_*: float64 on operands rounded to bf16 where the kernels round them),
under the bars of that file: a measured multiple of the error of a float32 evaluation of the same inputs, and the hard cap
(K 2^-24 + p) |A||B|.  Output buffers are prefilled with NaN -- or with known values where the call accumulates -- between
two canaries of 64 floats that must come back untouched.  The only kernel-against-kernel assertions are the bit-equality
promises of the header: WN_EXEC_NO_PIPELINED_GEMM, and run to run where a workspace fixes the order of the sums.

The largest ratio to the yardstick per entry point, mode and family is written to channel_gemm_error.json in the directory
that the environment variable WAVENET_HIP_RECORD_DIR names (unset: no record is written; profiles/channel_gemm_error.json is
a committed copy of one).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from wavenet_amd import _lib

import channel_gemm_ref as G
from gpu_util import EX, to_np

pytestmark = pytest.mark.gpu

GENERIC = _lib.WN_EXEC_FORCE_GENERIC
NO_PIPE = _lib.WN_EXEC_NO_PIPELINED_GEMM
WN_ESHAPE = -2
# (label, WnExec.precision, WnExec.flags, the mode whose bars apply)
RUNS = [("fp32", "fp32", 0, "fp32"), ("bf16x3", "bf16x3", 0, "bf16x3"), ("bf16", "bf16", 0, "bf16"),
        ("fp16x2", "fp16x2", 0, "fp16x2"), ("generic", "fp32", GENERIC, "fp32")]

RECORD = {}          # "entry/mode/family" -> {"max": [ratio, case], "rms": [ratio, case]}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    where = os.environ.get("WAVENET_HIP_RECORD_DIR")
    if not RECORD or not where:
        return
    import test_channel_gemm_bars_cpu as cpu
    smallest = min(min(cpu._mutants(K).values()) for K in cpu.KS)
    out = {"multiple": {"max": G.MULT_MAX, "rms": G.MULT_RMS},
           "smallest_cpu_mutant_error_over_bar": round(smallest, 3),
           "smallest_cpu_mutant_ratio_to_float32_yardstick": {"max": round(min(r[0] for r in cpu.SEEN), 3), "rms": round(min(r[1] for r in cpu.SEEN), 3)},
           "largest_ratio_to_float32_yardstick": {k: {"max": [round(v["max"][0], 3), v["max"][1]], "rms": [round(v["rms"][0], 3), v["rms"][1]]}
                                                  for k, v in sorted(RECORD.items())}}
    os.makedirs(where, exist_ok=True)
    with open(os.path.join(where, "channel_gemm_error.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


# ---- guarded buffers ------------------------------------------------------------------------------------------------
CANARY_BYTES = 64 * 4


class Buf(object):
    """A device buffer between two canaries of 64 floats.  fill: NaN (None), or the array the call accumulates onto.
    dtype int16 holds raw bf16 bits (NaN = 0x7fc0)."""
    live = []

    def __init__(self, shape, fill=None, dtype=torch.float32):
        n = int(np.prod(shape))
        pad = CANARY_BYTES // (4 if dtype == torch.float32 else 2)
        self.pad, self.raw = pad, torch.empty(n + 2 * pad, dtype=dtype, device="cuda")
        self.pattern = (torch.arange(pad, device="cuda") * 3 + 1001).to(dtype)
        self.raw[:pad] = self.pattern
        self.raw[pad + n:] = self.pattern
        self.t = self.raw[pad:pad + n].view(*shape)
        if fill is None:
            self.t.fill_(float("nan") if dtype == torch.float32 else 0x7fc0)
        else:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(fill)).view(*shape))
        Buf.live.append(self)

    def intact(self):
        n = self.raw.numel() - 2 * self.pad
        return torch.equal(self.raw[:self.pad], self.pattern) and torch.equal(self.raw[self.pad + n:], self.pattern)

    def np(self):
        return to_np(self.t)


def _sync_and_check_canaries(what):
    torch.cuda.synchronize()
    bad = [i for i, b in enumerate(Buf.live) if not b.intact()]
    Buf.live = []
    assert not bad, "%s: canary overwritten around output buffer(s) %r" % (what, bad)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def P(t):
    return None if t is None else (t.t.data_ptr() if isinstance(t, Buf) else t.data_ptr())


def PA(ts):
    arr = (C.c_void_p * max(1, len(ts)))()
    for i, t in enumerate(ts):
        arr[i] = P(t)
    return arr


def ex(run):
    return EX(run[1], flags=run[2])


class Judge(object):
    """collects the verdicts of one case so that every figure is printed before anything is asserted"""

    def __init__(self, entry, case, label, mode, family):
        self.entry, self.case, self.label, self.mode, self.family, self.misses = entry, case, label, mode, family, []

    def __call__(self, name, got, ref, ref_rb, den, yard, K, out_bf16=False, rounds=True, ranged_abs=None, slack=None):
        want = ref_rb if (self.mode == "bf16" and rounds) else ref
        slack = slack if (self.mode == "bf16" and rounds) else None
        if self.family == "ranged" and self.mode == "fp16x2" and ranged_abs is not None:
            verdict = G.check_ranged_fp16x2(got, want, K, *ranged_abs)
            print("%s %s %s %s %s: absolute bar, %s" % (self.entry, self.case, self.label, self.family, name, verdict or "ok"))
        else:
            verdict = G.check(got, want, den, yard, self.mode, K, out_bf16, slack)
            r = G.ratios(got, want, den, yard, out_bf16, slack)
            print("%s %s %s %s %s: max %.3f rms %.3f x yardstick (%.3g / %.3g) %s"
                  % (self.entry, self.case, self.label, self.family, name, r[0], r[1], yard[0], yard[1], verdict or "ok"))
            if np.isfinite(r[0]) and np.isfinite(r[1]):
                rec = RECORD.setdefault("%s/%s/%s" % (self.entry, self.label, self.family), {"max": [0.0, ""], "rms": [0.0, ""]})
                if r[0] > rec["max"][0]:
                    rec["max"] = [r[0], "%s %s" % (self.case, name)]
                if r[1] > rec["rms"][0]:
                    rec["rms"] = [r[1], "%s %s" % (self.case, name)]
        if verdict:
            self.misses.append((name, verdict))

    def done(self):
        assert not self.misses, (self.entry, self.case, self.label, self.family, self.misses)


# =====================================================================================================================
# head convolutions: wn_pointwise_fwd / wn_pointwise_bwd
# =====================================================================================================================
# name: (Cin, Cout, N, act, bias, NULL output of the backward, reason)
POINTWISE = {
    "mt1": (32, 32, 1, G.ACT_NONE, True, None, "M % 64 != 0: k_colgemm<1> / b3 with mtiles 1; one row, less than a 128-row workgroup"),
    "mt1_groups": (96, 160, 127, G.ACT_RELU, False, None, "M = 160: mt 1, five row groups in grid.y; dx with M = 96: three; no bias"),
    "mt2": (64, 192, 128, G.ACT_ELU, True, None, "M % 64 == 0: mt 2; exactly one 128-row workgroup; elu on both operand paths"),
    "mt4": (128, 128, 129, G.ACT_RELU, True, None, "M % 128 == 0: mt 4 (bf16x3: mtiles 4, one group); a second workgroup of one row"),
    "mt8": (256, 256, 255, G.ACT_RELU, True, None, "M % 256 == 0: mt 8, in bf16 the one-term MT 8 kernel (mtiles >= 8); wgrad M == 256 && nprob >= 8: the wide block"),
    "wide_slices": (512, 768, 256, G.ACT_ELU, True, None, "wgrad M % 256 == 0 && nprob >= 8: one wide launch per 256 rows of A, bias sums 'all or none'; one full 256-row slab"),
    "second_c0_group": (2080, 32, 257, G.ACT_NONE, True, None, "65 column tiles of x: the second c0 group of mfma_pointwise_bwd_dw, column sums with the first only; dx with 65 row groups; a 257th row: a second wgrad slab"),
    "generic_shape": (24, 40, 129, G.ACT_RELU, True, None, "channels no multiple of 32: generic_pointwise_* in every mode"),
    "dx_null": (128, 128, 257, G.ACT_NONE, True, "dx", "dx NULL: the weight gradient alone; two wgrad slabs (257 rows)"),
    "dw_null": (64, 192, 255, G.ACT_RELU, True, "dW", "dW NULL: dbias from generic_colsum on its own"),
    "dbias_null": (256, 256, 256, G.ACT_ELU, True, "dbias", "dbias NULL: the wide block without its column sums"),
    "wide_one_row": (512, 768, 1, G.ACT_RELU, False, None, "N = 1 through the wide block: every row of the slab but one is masked; no bias"),
}

_pw_cache = {}


def _pw_frame(name):
    """inputs, references, denominators and yardstick figures of a pointwise case: made once, left unchanged"""
    if name not in _pw_cache:
        Cin, Cout, N, act, bias, null, _ = POINTWISE[name]
        rs = np.random.RandomState(100 + list(POINTWISE).index(name))
        d = dict(x=G.flat_activations(rs, N, Cin), W=G.flat_weights(rs, Cout, Cin), dout=G.flat_activations(rs, N, Cout),
                 b=(0.1 * rs.randn(Cout)).astype(np.float32) if bias else None,
                 dW0=rs.randn(Cout, Cin).astype(np.float32), db0=rs.randn(Cout).astype(np.float32))
        fr = {}
        for key, ar in (("ref", G.F64), ("rb", G.RB64), ("den", G.ABS), ("f32", G.F32)):
            fr[key] = (G.pointwise_fwd(ar, d["x"], d["W"], d["b"], act),) + G.pointwise_bwd(ar, d["x"], d["W"], d["dout"], act, d["dW0"], d["db0"])
        fr["yard"] = [G.measure(fr["f32"][i], fr["ref"][i], fr["den"][i]) for i in range(4)]
        fr["slack"] = [None] * 4
        if act == G.ACT_ELU:        # WN_GEMM_BF16 only: elu(x) lands within two float32 ulps of a bf16 midpoint (see the function)
            sl = G.elu_rounding_slack(d["x"])
            fr["slack"][0], fr["slack"][2] = sl @ np.abs(d["W"]).T.astype(np.float64), np.abs(d["dout"]).T.astype(np.float64) @ sl
        _pw_cache[name] = (d, fr)
    return _pw_cache[name]


@pytest.mark.parametrize("name", list(POINTWISE))
def test_pointwise_against_float64(name):
    Cin, Cout, N, act, bias, null, _ = POINTWISE[name]
    d, fr = _pw_frame(name)
    lib = _lib.lib()
    x, W, dout = dev(d["x"]), dev(d["W"]), dev(d["dout"])
    b = dev(d["b"]) if bias else None
    e = 4 if act == G.ACT_ELU else 0      # elu: expm1f / expf of the input and act'(x)'s product, a few more roundings per term
    Ks = (Cin + 1 + e, Cout + 2 + e, N + 1 + e, N + 1)
    for run in RUNS:
        out = Buf((N, Cout))
        _lib.check(lib.wn_pointwise_fwd(P(x), P(W), P(b), P(out), N, Cin, Cout, act, ex(run), _lib.stream_ptr()), "wn_pointwise_fwd")
        dx = None if null == "dx" else Buf((N, Cin))
        dW = None if null == "dW" else Buf((Cout, Cin), d["dW0"])
        db = None if null == "dbias" else Buf((Cout,), d["db0"])
        _lib.check(lib.wn_pointwise_bwd(P(x), P(W), P(dout), P(dx), P(dW), P(db), N, Cin, Cout, act, ex(run), _lib.stream_ptr()),
                   "wn_pointwise_bwd")
        _sync_and_check_canaries("%s %s" % (name, run[0]))
        # the split kernels run only where the MFMA path does: a generic shape multiplies in fp32 whatever the mode
        rounds = Cin % 32 == 0 and Cout % 32 == 0
        j = Judge("wn_pointwise", name, run[0], run[3], "flat")
        for i, (nm, buf) in enumerate((("out", out), ("dx", dx), ("dW", dW), ("dbias", db))):
            if buf is not None:
                j(nm, buf.np(), fr["ref"][i], fr["rb"][i], fr["den"][i], fr["yard"][i], Ks[i], rounds=rounds, slack=fr["slack"][i])
        j.done()


# =====================================================================================================================
# the skip path: wn_skip_sum_fwd / wn_skip_sum_bwd_dz / wn_skip_sum_bwd_dw
# =====================================================================================================================
# name: dict(cd = widths per layer, Cs, B, T, t_off (Tw = T - t_off), sliced = z as slices of one array, bs = None | "full" |
#            "holes", acc = accumulate, dws = "full" | "holes", dbs = None | "full", fwd_ranged, reason)
def _sk(cd, Cs, B, T, t_off, reason, sliced=True, bs="full", acc=0, dws="full", dbs="full", fwd_ranged=False):
    return dict(cd=cd, Cs=Cs, B=B, T=T, t_off=t_off, Tw=T - t_off, sliced=sliced, bs=bs, acc=acc, dws=dws, dbs=dbs,
                fwd_ranged=fwd_ranged, reason=reason)


SKIP = {
    "one_source": _sk([32], 32, 1, 32, 0, "L = 1, Cs = 32: mtiles 1, a single source; Tw = 32: exactly one tile; dz: nchunks 1"),
    "two_wide_sources": _sk([64, 64], 96, 3, 34, 1, "cd = 64: cps 2, so never the lean kernel; Cs = 96: mt 1 / mtiles 3; Tw = 33, t_off = 1; z in separate allocations",
                            sliced=False),
    "odd_chunks": _sk([32] * 3, 256, 1, 131, 100, "L = 3: nchunks odd, not lean: k_colgemm_b3<0, ., 3, 8>; Tw = 31: less than a tile; dz: k_dz_ws with idle waves; dw: nprob 3 < 8",
                      bs=None),
    "lean": _sk([32] * 8, 256, 3, 300, 43, "L = 8 equally spaced: k_colgemm_h2q; dz: k_dz_ws, nchunks == 8 && ldo == 32; dw: M == 256 && nprob >= 8: k_wgrad_h2p; Tw = 257",
                fwd_ranged=True),
    "unequal_gaps": _sk([32] * 8, 256, 3, 300, 43, "the same with unequal gaps between the sources: not lean, k_colgemm_b3<0, ., 3, 8>", sliced=False, acc=1),
    "straddle": _sk([96] * 22, 128, 1, 65, 32, "22 layers of three 32-row tiles: 66 problems, layer 21 straddles the WN_MAX_SRC cut of mfma_skip_bwd_dz / _dw (j carried); Cs = 128: mt 4",
                    bs="holes", dbs=None),
    "many_sources": _sk([32] * 66, 256, 1, 65, 32, "66 sources: the second forward launch accumulates onto the first; dw: 64 problems wide, then 2 through k_wgrad_b3",
                        dws="holes"),
    "mixed_widths": _sk([32, 64, 32, 128], 256, 3, 40, 9, "K differs between sources: WN_ESHAPE from the split launcher, the exact-fp32 k_colgemm<8>; dz / dw: a launch per run of equal widths",
                        sliced=False, bs="holes", acc=1),
    "cs512_wide": _sk([128, 128], 512, 1, 64, 32, "Cs = 512, 8 problems: one wide wgrad launch per 256 rows of dskip; forward mtiles 16; dz nchunks 16"),
    "cs512_narrow": _sk([128], 512, 3, 33, 0, "Cs = 512, 4 problems < 8: k_wgrad_b3 with mt 4 and two groups in z; t_off = 0; Tw = 33", acc=1, dws="full"),
    "last_column": _sk([32, 32], 256, 3, 40, 39, "t_off = T - 1, Tw = 1: one column per clip; L = 2 even: lean with a ragged only tile"),
    "short_clip": _sk([32] * 2, 256, 1, 31, 0, "T = 31 < 32: rows_out_per_b < 32 keeps dz off k_dz_ws: k_colgemm_b3<2, 0, 3, 8>", bs=None, dbs=None),
    "cd128_cs96": _sk([128], 96, 3, 33, 1, "cd = 128 into Cs = 96: mt 1 with three groups; dz: four tiles per layer; Tw = 32", bs="holes", acc=1),
}

_sk_cache = {}


def _holes(n):
    return [i for i in range(n) if i % 3 == 1] if n > 1 else [0]


def _sk_frame(name, family):
    """family "flat": z in [-1, 1], dskip N(0, 1).  "ranged": the rows of dskip (and of z, for the forward) over six decades."""
    key = (name, family)
    if key not in _sk_cache:
        c = SKIP[name]
        L, Cs, B, T, t_off, Tw = len(c["cd"]), c["Cs"], c["B"], c["T"], c["t_off"], c["Tw"]
        rs = np.random.RandomState(500 + list(SKIP).index(name))
        ktot = sum(c["cd"])
        d = dict(z=[G.unit_activations(rs, B, T, w) for w in c["cd"]],
                 Ws=[(rs.randn(Cs, w) / np.sqrt(ktot)).astype(np.float32) for w in c["cd"]],            # N(0, 1 / contraction)
                 Wz=[(rs.randn(Cs, w) / np.sqrt(Cs)).astype(np.float32) for w in c["cd"]],              # dz contracts over Cs
                 bs=[(0.1 * rs.randn(Cs)).astype(np.float32) for _ in range(L)],
                 skip0=rs.randn(B, Tw, Cs).astype(np.float32), dskip=rs.randn(B, Tw, Cs).astype(np.float32),
                 dW0=[rs.randn(Cs, w).astype(np.float32) for w in c["cd"]], db0=[rs.randn(Cs).astype(np.float32) for _ in range(L)])
        if c["bs"] is None:
            d["bs"] = None
        elif c["bs"] == "holes":
            for l in _holes(L):
                d["bs"][l] = None
        if c["dws"] == "holes":
            for l in _holes(L):
                d["dW0"][l] = None
        if c["dbs"] is None:
            d["db0"] = None
        if family == "ranged":
            d["dskip"] = G.ranged(rs, d["dskip"])
            d["z_fwd"] = [G.ranged(rs, z) for z in d["z"]]
        else:
            d["z_fwd"] = d["z"]
        fr = {}
        for k, ar in (("ref", G.F64), ("rb", G.RB64), ("den", G.ABS), ("f32", G.F32)):
            fwd = G.skip_fwd(ar, d["z_fwd"], d["Ws"], d["bs"], t_off, Tw, d["skip0"] if c["acc"] else None)
            dz = G.skip_dz(ar, d["Wz"], d["dskip"], T, t_off)
            dWs, dbs = G.skip_dw(ar, d["z"], d["dskip"], t_off, d["dW0"], d["db0"])
            fr[k] = dict(fwd=fwd, dz=dz, dWs=dWs, dbs=dbs)
        fr["yard"] = dict(fwd=G.measure(fr["f32"]["fwd"], fr["ref"]["fwd"], fr["den"]["fwd"]),
                          dz=[G.measure(fr["f32"]["dz"][l][:, t_off:], fr["ref"]["dz"][l][:, t_off:], fr["den"]["dz"][l][:, t_off:]) for l in range(L)],
                          dWs=[G.measure(fr["f32"]["dWs"][l], fr["ref"]["dWs"][l], fr["den"]["dWs"][l]) for l in range(L)],
                          dbs=[G.measure(fr["f32"]["dbs"][l], fr["ref"]["dbs"][l], fr["den"]["dbs"][l]) for l in range(L)])
        _sk_cache[key] = (d, fr)
    return _sk_cache[key]


def _place(arrays, sliced):
    """the arrays on the device: slices of ONE array (equally spaced; equal shapes only), or carved from one allocation with
    gaps of 64, 128, 192, 64, ... floats between them (unequal, every start 16-byte aligned)"""
    if sliced:
        whole = dev(np.stack(arrays))
        return [whole[l] for l in range(len(arrays))], whole
    gaps = [64 * (l % 3 + 1) for l in range(len(arrays))]
    whole = torch.zeros(sum(a.size for a in arrays) + sum(gaps), device="cuda")
    out, o = [], 0
    for a, g in zip(arrays, gaps):
        o += g
        v = whole[o:o + a.size].view(*a.shape)
        v.copy_(torch.as_tensor(a))
        out.append(v)
        o += a.size
    return out, whole


def _fwd_has_older_kernel(c):
    """launch_colgemm_b3's `lean`: the shapes k_colgemm_h2q takes from k_colgemm_b3<0, ., 3, 8>"""
    cd, L = c["cd"], len(c["cd"])
    return (L <= 64 and len(set(cd)) == 1 and c["Cs"] >= 256 and (L * cd[0] // 32) % 2 == 0 and
            (L == 1 or (cd[0] == 32 and c["sliced"])))


def _run_skip(name, family, run, want_fwd=True):
    c = SKIP[name]
    d, fr = _sk_frame(name, family)
    L, Cs, B, T, t_off, Tw = len(c["cd"]), c["Cs"], c["B"], c["T"], c["t_off"], c["Tw"]
    lib, cd = _lib.lib(), _lib.int_array(c["cd"])
    keep = []
    res = {}
    dskip = dev(d["dskip"])
    if want_fwd:
        z, w1 = _place(d["z_fwd"], c["sliced"])
        Ws = [dev(w) for w in d["Ws"]]
        bs = None if d["bs"] is None else [None if b is None else dev(b) for b in d["bs"]]
        skip = Buf((B, Tw, Cs), d["skip0"] if c["acc"] else None)
        keep += [z, w1, Ws, bs]
        _lib.check(lib.wn_skip_sum_fwd(L, PA(z), PA(Ws), None if bs is None else PA(bs), cd, P(skip), B, T, t_off, Tw, Cs, c["acc"],
                                       ex(run), _lib.stream_ptr()), "wn_skip_sum_fwd")
        res["fwd"] = skip
    Wz = [dev(w) for w in d["Wz"]]
    dz = [Buf((B, T, w)) for w in c["cd"]]
    _lib.check(lib.wn_skip_sum_bwd_dz(L, PA(Wz), cd, P(dskip), PA(dz), B, T, t_off, Tw, Cs, ex(run), _lib.stream_ptr()), "wn_skip_sum_bwd_dz")
    zb, w2 = _place(d["z"], c["sliced"])
    dWs = [None if w0 is None else Buf(w0.shape, w0) for w0 in d["dW0"]]
    dbs = None if d["db0"] is None else [Buf((Cs,), b0) for b0 in d["db0"]]
    keep += [Wz, zb, w2]
    _lib.check(lib.wn_skip_sum_bwd_dw(L, PA(zb), cd, P(dskip), PA(dWs), None if dbs is None else PA(dbs), B, T, t_off, Tw, Cs,
                                      ex(run), _lib.stream_ptr()), "wn_skip_sum_bwd_dw")
    _sync_and_check_canaries("%s %s %s" % (name, family, run[0]))
    res.update(dz=dz, dWs=dWs, dbs=dbs)
    return res


def _judge_skip(name, family, run, res):
    c = SKIP[name]
    d, fr = _sk_frame(name, family)
    L, Cs, B, T, t_off, Tw = len(c["cd"]), c["Cs"], c["B"], c["T"], c["t_off"], c["Tw"]
    mfma = run[2] == 0                                    # every width here is a multiple of 32
    nbias = 0 if d["bs"] is None else sum(b is not None for b in d["bs"])
    zmax = max(float(np.abs(z).max()) for z in d["z"])
    if "fwd" in res:
        j = Judge("wn_skip_sum_fwd", name, run[0], run[3], family)
        # (launch_colgemm_b3, modes 0: sources of different K are WN_ESHAPE, and launch_colgemm falls back to the exact-fp32 kernel)
        rounds = mfma and all(len(set(c["cd"][l0:l0 + 64])) == 1 for l0 in range(0, L, 64))
        j("skip", res["fwd"].np(), fr["ref"]["fwd"], fr["rb"]["fwd"], fr["den"]["fwd"], fr["yard"]["fwd"], sum(c["cd"]) + nbias + 2,
          rounds=rounds, ranged_abs=(max(float(np.abs(z).max()) for z in d["z_fwd"]), max(float(np.abs(w).max()) for w in d["Ws"])))
        j.done()
    j = Judge("wn_skip_sum_bwd_dz", name, run[0], run[3], family)
    wmax = max(float(np.abs(w).max()) for w in d["Wz"])
    for l in range(L):
        got = res["dz"][l].np()
        assert not got[:, :t_off].any(), (name, run[0], l, "dz is not exactly zero below t_off")
        j("dz[%d]" % l, got[:, t_off:], fr["ref"]["dz"][l][:, t_off:], fr["rb"]["dz"][l][:, t_off:], fr["den"]["dz"][l][:, t_off:],
          fr["yard"]["dz"][l], Cs, rounds=mfma, ranged_abs=(float(np.abs(d["dskip"]).max()), wmax))
    j.done()
    j = Judge("wn_skip_sum_bwd_dw", name, run[0], run[3], family)
    for l in range(L):
        if res["dWs"][l] is not None:
            j("dWs[%d]" % l, res["dWs"][l].np(), fr["ref"]["dWs"][l], fr["rb"]["dWs"][l], fr["den"]["dWs"][l], fr["yard"]["dWs"][l], B * Tw + 1,
              rounds=mfma, ranged_abs=(float(np.abs(d["dskip"]).max()), zmax))
        if res["dbs"] is not None:
            j("dbs[%d]" % l, res["dbs"][l].np(), fr["ref"]["dbs"][l], fr["rb"]["dbs"][l], fr["den"]["dbs"][l], fr["yard"]["dbs"][l], B * Tw + 1)
    j.done()


@pytest.mark.parametrize("name", list(SKIP))
def test_skip_path_against_float64(name):
    for run in RUNS:
        _judge_skip(name, "flat", run, _run_skip(name, "flat", run))


@pytest.mark.parametrize("name", list(SKIP))
def test_skip_path_ranged_rows_against_float64(name):
    """dskip with per-row magnitudes over six decades (its range is measured on the device), z too on the forward case"""
    fwd = SKIP[name]["fwd_ranged"]
    for run in RUNS:
        _judge_skip(name, "ranged", run, _run_skip(name, "ranged", run, want_fwd=fwd))


@pytest.mark.parametrize("name", list(SKIP))
def test_skip_path_older_kernels_bit_for_bit(name):
    """fp16x2: WN_EXEC_NO_PIPELINED_GEMM selects k_colgemm_b3 / k_wgrad_b3w instead of k_colgemm_h2q / k_dz_ws / k_wgrad_h2p --
    'same results, bit for bit' (include/wavenet_hip.h).  The forward and dz have no atomics on either side and are compared
    on every shape; dWs where the wide block runs (Cs == 256 and at least 8 problems in the launch: fixed-order partial
    sums on both sides -- k_wgrad_b3 adds its slabs with float atomics, in no fixed order)."""
    c = SKIP[name]
    new = _run_skip(name, "flat", ("fp16x2", "fp16x2", 0, "fp16x2"))
    old = _run_skip(name, "flat", ("fp16x2", "fp16x2", NO_PIPE, "fp16x2"))
    assert torch.equal(new["fwd"].t, old["fwd"].t), (name, "forward", _fwd_has_older_kernel(c))
    for l in range(len(c["cd"])):
        assert torch.equal(new["dz"][l].t, old["dz"][l].t), (name, "dz", l)
    if c["Cs"] == 256 and len(set(c["cd"])) == 1:
        live = [l for l in range(len(c["cd"])) if new["dWs"][l] is not None]
        # the launches of mfma_skip_bwd_dw: WN_MAX_SRC problems (32-column tiles of the layers that have a dWs) at a time
        nprob = len(live) * (c["cd"][0] // 32)
        if nprob >= 8 and (nprob % 64 == 0 or nprob % 64 >= 8):
            for l in live:
                assert torch.equal(new["dWs"][l].t, old["dWs"][l].t), (name, "dWs", l)


# =====================================================================================================================
# bf16 storage: wn16_cvt_*, wn16_pack_pointwise, wn16_pointwise_fwd / _bwd
# =====================================================================================================================
def _bits(a):
    """float32 values that are bf16 already -> their raw bits as an int16 numpy array (the device buffers' type)"""
    return G.bf16_bits(a).view(np.int16)


def test_wn16_cvt_is_round_to_nearest_even_bit_for_bit():
    rs = np.random.RandomState(16)
    n = 4096
    u = rs.randint(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7f800000) == 0x7f800000] &= np.uint32(0xbfffffff)          # no NaN / infinity among the random ones
    u[:512] = (u[:512] & np.uint32(0xffff0000)) | np.uint32(0x8000)      # ties, odd and even upper halves
    u[512:640] = (u[512:640] & np.uint32(0xffff0000)) | np.uint32(0x7fff)        # just below a tie
    u[640:768] = (u[640:768] & np.uint32(0xffff0000)) | np.uint32(0x8001)        # just above
    u[768:1024] &= np.uint32(0x807fffff)                                  # subnormals, both signs
    u[1024:1032] = np.array([0, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff, 0x00000001, 0x80000001], np.uint32)
    x = u.view(np.float32)
    want = G.bf16_bits(G.rb32(x)).view(np.int16)
    dst, x_dev, want_dev = Buf((n,), dtype=torch.int16), dev(x), dev(want)      # (inputs held by name: they live until the sync)
    _lib.check(_lib.lib().wn16_cvt_to_bf16(P(x_dev), P(dst), n, _lib.stream_ptr()), "wn16_cvt_to_bf16")
    back = Buf((n,))
    _lib.check(_lib.lib().wn16_cvt_to_f32(P(want_dev), P(back), n, _lib.stream_ptr()), "wn16_cvt_to_f32")
    _sync_and_check_canaries("wn16_cvt")
    got = dst.np()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(hex(int(u[i])), hex(int(got[i]) & 0xffff), hex(int(want[i]) & 0xffff)) for i in bad[:8]]
    assert np.array_equal(back.np().view(np.uint32), want.view(np.uint16).astype(np.uint32) << 16)


# name: (Cin, Cout, N, act, bias, out_f32, reason)
W16_FWD = {
    "k128_one_row": (128, 128, 1, G.ACT_NONE, True, 1, "one m-block, one source, N = 1; fp32 output with bias: k16_cgemm<false, 0, true>"),
    "k256_m384": (256, 384, 127, G.ACT_RELU, False, 0, "three m-blocks, two sources, relu on the operand, bf16 output: k16_cgemm<true, 0, false>; 127 rows"),
    "k512_m256": (512, 256, 128, G.ACT_RELU, True, 1, "the head's 512 -> 256, relu, fp32 output: k16_cgemm<true, 0, true>; exactly one 128-row block"),
    "k128_two_blocks": (128, 128, 129, G.ACT_NONE, False, 0, "a second block of one row, bf16 output without bias: k16_cgemm<false, 0, false>"),
    "k256_m384_300": (256, 384, 300, G.ACT_NONE, True, 0, "three row blocks, the last ragged (44 rows); bias into a bf16 output"),
}
# name: (Cin, Cout, N, act, dout as fp32, workspace, dx NULL, reason)
W16_BWD = {
    "sq256": (256, 256, 8, G.ACT_RELU, True, True, False, "one 256 x 256 problem, 8 rows, dout rounded from fp32 into the scratch, fixed-order sums; dx through the relu mask (ep 2)"),
    "k512": (512, 256, 120, G.ACT_NONE, False, True, False, "two problems along Cin; dout given as bf16 (no dbias); dx without a mask"),
    "m512": (256, 512, 128, G.ACT_RELU, True, False, False, "two problems along Cout, no workspace: float atomics for dW and dbias"),
    "sq256_ragged": (256, 256, 136, G.ACT_NONE, True, True, True, "dx NULL; 136 rows: a second row block of 8"),
    "k512_304": (512, 256, 304, G.ACT_RELU, True, True, False, "304 rows: three row blocks of the dx GEMM, several time chunks of k16_wgrad"),
}

_w16_cache = {}


def _w16_inputs(key, Cin, Cout, N, idx):
    if key not in _w16_cache:
        rs = np.random.RandomState(1600 + idx)
        _w16_cache[key] = dict(x=G.rb32(G.flat_activations(rs, N, Cin)), W=G.flat_weights(rs, Cout, Cin),
                               b=(0.1 * rs.randn(Cout)).astype(np.float32), dout=G.flat_activations(rs, N, Cout),
                               dW0=rs.randn(Cout, Cin).astype(np.float32), db0=rs.randn(Cout).astype(np.float32))
    return _w16_cache[key]


def _pack(W, Cout, Cin):
    """wn16_pack_pointwise, checked: Wb is bf16(W), WbT its transpose, bit for bit"""
    Wb, WbT, W_dev = Buf((Cout, Cin), dtype=torch.int16), Buf((Cin, Cout), dtype=torch.int16), dev(W)
    _lib.check(_lib.lib().wn16_pack_pointwise(P(W_dev), P(Wb), P(WbT), Cout, Cin, _lib.stream_ptr()), "wn16_pack_pointwise")
    torch.cuda.synchronize()
    want = _bits(G.rb32(W))
    assert np.array_equal(Wb.np(), want) and np.array_equal(WbT.np(), want.T)
    return Wb, WbT


@pytest.mark.parametrize("name", list(W16_FWD))
def test_wn16_pointwise_fwd_against_float64_on_bf16_operands(name):
    Cin, Cout, N, act, bias, out_f32, _ = W16_FWD[name]
    d = _w16_inputs(("fwd", name), Cin, Cout, N, list(W16_FWD).index(name))
    b = d["b"] if bias else None
    Wb, _WbT = _pack(d["W"], Cout, Cin)
    out = Buf((N, Cout)) if out_f32 else Buf((N, Cout), dtype=torch.int16)
    x_dev, b_dev = dev(_bits(d["x"])), None if b is None else dev(b)                   # held by name until the sync
    _lib.check(_lib.lib().wn16_pointwise_fwd(P(x_dev), P(Wb), P(b_dev), P(out), out_f32, N, Cin, Cout, act, _lib.stream_ptr()),
               "wn16_pointwise_fwd")
    _sync_and_check_canaries(name)
    ref, rb, den = (G.pointwise_fwd(ar, d["x"], d["W"], b, act) for ar in (G.F64, G.RB64, G.ABS))
    yard = G.measure(G.pointwise_fwd(G.F32, d["x"], d["W"], b, act), ref, den)
    got = out.np() if out_f32 else G.bf16_from_bits(out.np().view(np.uint16)).reshape(N, Cout)
    j = Judge("wn16_pointwise_fwd", name, "bf16-storage", "bf16", "flat")
    j("out", got, ref, rb, den, yard, Cin + 1, out_bf16=not out_f32)
    j.done()


@pytest.mark.parametrize("name", list(W16_BWD))
def test_wn16_pointwise_bwd_against_float64_on_bf16_operands(name):
    Cin, Cout, N, act, f32_dout, with_ws, dx_null, _ = W16_BWD[name]
    d = _w16_inputs(("bwd", name), Cin, Cout, N, 50 + list(W16_BWD).index(name))
    lib = _lib.lib()
    _Wb, WbT = _pack(d["W"], Cout, Cin)
    dout = d["dout"] if f32_dout else G.rb32(d["dout"])                   # as bf16 it IS the gradient; as fp32 the call rounds it
    x_dev, g16, g32 = dev(_bits(d["x"])), None if f32_dout else dev(_bits(dout)), dev(dout) if f32_dout else None
    nbytes = lib.wn16_pointwise_bwd_workspace_bytes(N, Cout)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda") if with_ws else None
    runs = []
    for _ in range(2 if with_ws else 1):
        dx = None if dx_null else Buf((N, Cin), dtype=torch.int16)
        dW = Buf((Cout, Cin), d["dW0"])
        db = Buf((Cout,), d["db0"]) if f32_dout else None                  # "the bias gradient is summed from the fp32 gradient"
        scratch = Buf((N, Cout), dtype=torch.int16) if f32_dout else None
        _lib.check(lib.wn16_pointwise_bwd(P(x_dev), P(WbT), P(g16), P(g32),
                                          P(scratch), P(dx), P(dW), P(db), N, Cin, Cout, act, P(ws), nbytes if with_ws else 0,
                                          _lib.stream_ptr()), "wn16_pointwise_bwd")
        _sync_and_check_canaries(name)
        runs.append((dx, dW, db, scratch))
    if with_ws:                                                            # "bit-reproducible" with the workspace
        for a, b in zip(runs[0][:3], runs[1][:3]):
            assert a is None or torch.equal(a.t, b.t), name
    dx, dW, db, scratch = runs[0]
    if scratch is not None:
        assert np.array_equal(scratch.np(), _bits(G.rb32(dout)))
    fr = {k: G.pointwise_bwd(ar, d["x"], d["W"], dout, act, d["dW0"], d["db0"]) for k, ar in
          (("ref", G.F64), ("rb", G.RB64), ("den", G.ABS), ("f32", G.F32))}
    yard = [G.measure(fr["f32"][i], fr["ref"][i], fr["den"][i]) for i in range(3)]
    j = Judge("wn16_pointwise_bwd", name, "bf16-storage", "bf16", "flat")
    if dx is not None:
        j("dx", G.bf16_from_bits(dx.np().view(np.uint16)).reshape(N, Cin), fr["ref"][0], fr["rb"][0], fr["den"][0], yard[0], Cout + 2, out_bf16=True)
    j("dW", dW.np(), fr["ref"][1], fr["rb"][1], fr["den"][1], yard[1], N + 1)
    if db is not None:
        j("dbias", db.np(), fr["ref"][2], fr["rb"][2], fr["den"][2], yard[2], N + 1)
    j.done()


def test_wn16_pointwise_refusals_leave_the_outputs_alone():
    """w16_api.hip: the forward takes channel counts that are multiples of 128, the backward of 256, both relu or none;
    anything else is WN_ESHAPE before any device work"""
    lib = _lib.lib()
    N = 16
    x, w, g = dev(np.zeros((N, 512), np.int16)), dev(np.zeros((512, 512), np.int16)), dev(np.zeros((N, 512), np.float32))
    for Cin, Cout, act in ((64, 128, G.ACT_NONE), (128, 192, G.ACT_NONE), (128, 128, G.ACT_ELU)):
        out = Buf((N, Cout))
        assert lib.wn16_pointwise_fwd(P(x), P(w), None, P(out), 1, N, Cin, Cout, act, _lib.stream_ptr()) == WN_ESHAPE, (Cin, Cout, act)
        _sync_and_check_canaries("refused forward")
        assert np.isnan(out.np()).all()
    for Cin, Cout, act in ((128, 256, G.ACT_NONE), (256, 384, G.ACT_NONE), (256, 256, G.ACT_ELU)):
        keep = np.full((Cout, Cin), 2.5, np.float32)
        dx, dW, db, scratch = Buf((N, Cin), dtype=torch.int16), Buf((Cout, Cin), keep), Buf((Cout,), keep[:, 0]), Buf((N, Cout), dtype=torch.int16)
        rc = lib.wn16_pointwise_bwd(P(x), P(w), None, P(g), P(scratch), P(dx), P(dW), P(db), N, Cin, Cout, act, None, 0, _lib.stream_ptr())
        assert rc == WN_ESHAPE, (Cin, Cout, act)
        _sync_and_check_canaries("refused backward")
        assert (dx.np() == 0x7fc0).all() and (scratch.np() == 0x7fc0).all() and (dW.np() == 2.5).all() and (db.np() == 2.5).all()
