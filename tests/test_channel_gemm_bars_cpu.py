"""The error bars of tests/channel_gemm_ref.py catch what they must -- no GPU.

For every K in {32, 96, 256, 512}: the faithful numpy emulation of each arithmetic mode passes that mode's bar on both input
families, and every mutant -- a kernel that is subtly wrong in one of the ways a split-product GEMM goes wrong -- misses it by
a factor of at least 2.  tests/test_gpu_channel_gemm_sweep.py holds the kernels to the same bars.
"""
import numpy as np
import pytest

import channel_gemm_ref as G

KS = [32, 96, 256, 512]
N_ROWS, M_OUT = 160, 96          # rows of activations, output channels: 15,360 outputs per contraction
FAMILIES = ("flat", "ranged")

_cache = {}


def _inputs(K, family):
    """the operands of every operation at contraction width K: made once, left unchanged"""
    key = (K, family)
    if key not in _cache:
        rs = np.random.RandomState(7000 + K + (1 if family == "ranged" else 0))
        d = {}
        d["x"] = G.flat_activations(rs, N_ROWS, K)
        d["W"] = G.flat_weights(rs, M_OUT, K)
        d["b"] = (0.1 * rs.randn(M_OUT)).astype(np.float32)
        # the skip path: two layers of width K / 2 into M_OUT skip channels; B = 2 clips, a window of N_ROWS / 2 columns at 3
        d["B"], d["T"], d["t_off"], d["Tw"] = 2, N_ROWS // 2 + 3, 3, N_ROWS // 2
        d["z"] = [G.unit_activations(rs, 2, d["T"], K // 2) for _ in range(2)]
        d["Ws"] = [(rs.randn(M_OUT, K // 2) / np.sqrt(K)).astype(np.float32) for _ in range(2)]      # N(0, 1 / contraction)
        d["bs"] = [(0.1 * rs.randn(M_OUT)).astype(np.float32) for _ in range(2)]
        d["skip0"] = rs.randn(2, d["Tw"], M_OUT).astype(np.float32)
        # dz: K skip channels contracted into two layers of 96 and 32 channels (96: three 32-row tiles)
        d["dskip"] = rs.randn(2, d["Tw"], K).astype(np.float32)
        d["Wz"] = [G.flat_weights(rs, 96, K).T.copy(), G.flat_weights(rs, 32, K).T.copy()]          # (Cs = K, cd)
        # dw: K rows of time contracted (B = 1); 64 skip channels, a layer of 96 channels
        d["dskip_w"] = rs.randn(1, K, 64).astype(np.float32)
        d["z_w"] = [G.unit_activations(rs, 1, K + 2, 96)]
        d["dW0"] = [rs.randn(64, 96).astype(np.float32)]
        if family == "ranged":
            d["x"] = G.ranged(rs, d["x"])
            d["z"] = [G.ranged(rs, z) for z in d["z"]]
            d["dskip"] = G.ranged(rs, d["dskip"])
            d["dskip_w"] = G.ranged(rs, d["dskip_w"])
        _cache[key] = d
    return _cache[key]


# name -> (function of (arith, inputs, **mutant knobs) giving one array, contraction length for the hard cap,
#          (max |A|, max |W|) of the fp16 split's absolute bar on the ranged family)
def _op_pointwise(ar, d, **kw):
    return G.pointwise_fwd(ar, d["x"], d["W"], d["b"], G.ACT_NONE)


def _op_skip_fwd(ar, d, accumulate=True, bias_times=1, **kw):
    return G.skip_fwd(ar, d["z"], d["Ws"], d["bs"], d["t_off"], d["Tw"], d["skip0"] if accumulate else None, bias_times)


def _op_dz(ar, d, misplace=False, **kw):
    dz = G.skip_dz(ar, d["Wz"], d["dskip"], d["T"], d["t_off"])
    if misplace:     # the first 32-row tile a launch writes of layer 0 lands where the previous launch's last tile belongs
        dz[0] = np.array(dz[0])
        dz[0][..., 0:32] = dz[0][..., 32:64]
        dz[0][..., 32:64] = 0
    return np.concatenate(dz, axis=2)


def _op_dw(ar, d, accumulate=True, **kw):
    return G.skip_dw(ar, d["z_w"], d["dskip_w"], 1, d["dW0"] if accumulate else None)[0][0]


OPS = {
    "pointwise_fwd": (_op_pointwise, lambda K: K + 1, lambda d: (np.abs(d["x"]).max(), np.abs(d["W"]).max())),
    "skip_fwd": (_op_skip_fwd, lambda K: K + 3, lambda d: (max(np.abs(z).max() for z in d["z"]), max(np.abs(w).max() for w in d["Ws"]))),
    "skip_dz": (_op_dz, lambda K: K, lambda d: (np.abs(d["dskip"]).max(), max(np.abs(w).max() for w in d["Wz"]))),
    "skip_dw": (_op_dw, lambda K: K + 1, lambda d: (np.abs(d["dskip_w"]).max(), np.abs(d["z_w"][0]).max())),
}


def _frame(op, K, family):
    """(reference F64, reference RB64, denominator, yardstick figures) of an operation: made once"""
    key = ("frame", op, K, family)
    if key not in _cache:
        f, d = OPS[op][0], _inputs(K, family)
        ref, den = f(G.F64, d), f(G.ABS, d)
        _cache[key] = (ref, f(G.RB64, d), den, G.measure(f(G.F32, d), ref, den))
    return _cache[key]


def _verdict(op, K, family, mode, got):
    ref, ref_rb, den, yard = _frame(op, K, family)
    if mode == "fp16x2" and family == "ranged":
        amax, wmax = OPS[op][2](_inputs(K, family))
        return G.check_ranged_fp16x2(got, ref, OPS[op][1](K), amax, wmax)
    return G.check(got, ref_rb if mode == "bf16" else ref, den, yard, mode, OPS[op][1](K))


SEEN = []        # (max ratio, RMS ratio) to the yardstick of every mutant evaluated: the GPU sweep's record quotes the smallest


def _excess(op, K, mode, got, family="flat"):
    """mutant error / bar: how many times over the bar it misses most (max or RMS) a result is"""
    ref, ref_rb, den, yard = _frame(op, K, family)
    r = G.ratios(got, ref_rb if mode == "bf16" else ref, den, yard)
    SEEN.append(r)
    return max(r[0] / G.MULT_MAX, r[1] / G.MULT_RMS)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", KS)
def test_faithful_emulation_of_every_mode_passes_its_bar(K, family):
    for op in OPS:
        for mode in G.MODES:
            got = OPS[op][0](G.EMULATION[mode], _inputs(K, family))
            assert _verdict(op, K, family, mode, got) is None, (op, K, family, mode, _verdict(op, K, family, mode, got))


def _mutants(K):
    """name -> excess over the bar, flat family"""
    d = _inputs(K, "flat")
    out = {}
    low = G.B3([t for t in G.B3_TERMS if t not in G.B3_LOW_TERMS])
    for op in OPS:
        out["bf16x3 without its three low terms / " + op] = _excess(op, K, "bf16x3", OPS[op][0](low, d))
        out["bf16 once where float32 is promised / " + op] = _excess(op, K, "bf16x3", OPS[op][0](G.BF16(), d))
        for mode in ("fp32", "bf16x3", "fp16x2"):
            out["a 32-wide K chunk missing / %s / %s" % (mode, op)] = _excess(op, K, mode, OPS[op][0](G.DropChunk(G.EMULATION[mode]), d))
    for op in ("skip_fwd", "skip_dz", "skip_dw"):                     # where fp16x2 runs its two-part split
        out["fp16x2 without lo*hi / " + op] = _excess(op, K, "fp16x2", OPS[op][0](G.H2(("hh", "hm")), d))
        out["fp16x2 without hi*lo / " + op] = _excess(op, K, "fp16x2", OPS[op][0](G.H2(("hh", "mh")), d))
    for mode in G.MODES:
        ar = G.EMULATION[mode]
        # every source's bias added with every source chunk (K / 32 of them, two at the least: one per source) instead of once
        out["bias once per source chunk / " + mode] = _excess("skip_fwd", K, mode, _op_skip_fwd(ar, d, bias_times=max(2, K // 32)))
        out["accumulate ignored / skip_fwd / " + mode] = _excess("skip_fwd", K, mode, _op_skip_fwd(ar, d, accumulate=False))
        out["accumulate ignored / skip_dw / " + mode] = _excess("skip_dw", K, mode, _op_dw(ar, d, accumulate=False))
        out["first tile of a layer in the previous launch's last place / " + mode] = _excess("skip_dz", K, mode, _op_dz(ar, d, misplace=True))
    return out


@pytest.mark.parametrize("K", KS)
def test_every_mutant_misses_the_bar_twice_over(K):
    m = _mutants(K)
    worst = min(m, key=m.get)
    print("K = %d: smallest mutant error / bar = %.2f (%s)" % (K, m[worst], worst))
    assert m[worst] >= 2.0, (K, worst, m[worst])


@pytest.mark.parametrize("term", G.B3_TERMS + tuple("h2:" + t for t in G.H2_TERMS))
def test_an_emulation_that_loses_any_one_product_term_fails(term):
    """Deleting any one product term from an emulation makes it miss the bar (at the narrowest contraction, where the fewest
    terms average the loss out)."""
    K = KS[0]
    d = _inputs(K, "flat")
    if term.startswith("h2:"):
        mode, ar, ops = "fp16x2", G.H2([t for t in G.H2_TERMS if t != term[3:]]), ("skip_fwd", "skip_dz", "skip_dw")
    else:
        mode, ar, ops = "bf16x3", G.B3([t for t in G.B3_TERMS if t != term]), tuple(OPS)
    for op in ops:
        assert _verdict(op, K, "flat", mode, OPS[op][0](ar, d)) is not None, (term, op)


def test_splits_are_the_headers_splits():
    """three bf16 parts carry 24 bits and two fp16 parts 22: the residuals the headers document"""
    rs = np.random.RandomState(3)
    x = (rs.randn(4096) * 10.0 ** rs.uniform(-3, 3, 4096)).astype(np.float32)
    h, m, l = G.split3(x)
    assert np.all(np.abs(x.astype(np.float64) - h - m - l) <= 2.0 ** -24 * np.abs(x))
    for part in (h, m, l):
        assert np.array_equal(G.rb32(part), part)
    s = G.h2_scale_of(np.abs(x).max())
    assert 2.0 ** 13 <= np.abs(x).max() * s < 2.0 ** 14
    big = x[np.abs(x) * s >= 1.0]                                        # both parts normal fp16 numbers
    hh, mm = G.split2h(big * np.float32(s))
    assert np.all(np.abs(big.astype(np.float64) * s - hh - mm) <= 2.0 ** -21 * np.abs(big * s))
