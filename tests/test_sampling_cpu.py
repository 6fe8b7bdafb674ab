"""CPU: the sampling controls (temperature, top-k, top-p) -- C-ABI surface, argument errors, the host module against a
literal restatement of the contract, the command-line flags.  No GPU needed.

The contract (include/wavenet_hip.h, wavenet_amd/sampling.py), per row p of float32 probabilities:
  order  j precedes i iff p[j] > p[i], or p[j] == p[i] and j < i; rank(i) = number of tokens preceding i
  top-k  pk[i] = p[i] if rank(i) < top_k else 0
  top-p  total = float64 sum of pk in index order; before(i) = float64 sum, in index order, of pk[j] over the j preceding
         i; keep i iff before(i) < top_p * total; the rank-0 token always
  draw   excluded entries 0.0f, no renormalisation; float64 running sum, divide by the last entry, first index with cdf > u
"""
import ctypes
import os
import re

import numpy as np
import pytest

from wavenet_amd import _lib, sampling
from wavenet_amd.train_audio import args as cli_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QS = (7, 64, 256, 300)
TOP_PS = (1.0, 0.9, 0.5, 1e-9)


def top_ks(Q):
    return (0, 1, 2, Q - 1, Q)


def restate_filter(p, top_k, top_p):
    """Steps 2-4 of the contract, literally: two nested loops per pass, float64 sums as adds of selected values.  (The
    float32 values are held as Python floats: every float32 is a float64, compares and sums are those of the contract.)"""
    p = [float(np.float32(v)) for v in p]
    Q = len(p)

    def precedes(j, i):
        return p[j] > p[i] or (p[j] == p[i] and j < i)

    rank = [0] * Q
    for i in range(Q):
        for j in range(Q):
            if precedes(j, i):
                rank[i] += 1
    k_on = 0 < top_k < Q
    pk = [p[i] if (not k_on or rank[i] < top_k) else 0.0 for i in range(Q)]
    if top_p >= 1.0:
        return np.asarray(pk, dtype=np.float32)
    total = 0.0
    for q in range(Q):
        total += pk[q]
    thr = top_p * total
    out = []
    for i in range(Q):
        before = 0.0
        for j in range(Q):
            before += pk[j] if precedes(j, i) else 0.0
        out.append(pk[i] if (before < thr or rank[i] == 0) else 0.0)
    return np.asarray(out, dtype=np.float32)


def restate_draw(row, u):
    """Step 5 on a filtered row: float64 running sum in index order, divide by the last entry, first index with cdf > u."""
    tot = 0.0
    for v in row:
        tot += float(v)
    c = 0.0
    for q, v in enumerate(row):
        c += float(v)
        if c / tot > u:
            return q
    return len(row)


def restate_token(p, u, top_k, top_p):
    return restate_draw(restate_filter(p, top_k, top_p), u)


def rows(Q, seed=0):
    """[(name, float32 row)]: random, with exact ties (few levels), with zeros, one-hot."""
    rs = np.random.RandomState(1000 * Q + seed)
    x = rs.standard_normal(Q) * 3.0
    rnd = np.exp(x - x.max())
    rnd = (rnd / rnd.sum()).astype(np.float32)
    lv = rs.randint(1, 5, Q).astype(np.float64)                       # four levels: many exact ties
    ties = (lv / lv.sum()).astype(np.float32)
    z = rs.random_sample(Q)
    z[rs.random_sample(Q) < 0.5] = 0.0
    z[int(rs.randint(Q))] = 0.7                                       # never all zero
    zeros = (z / z.sum()).astype(np.float32)
    hot = np.zeros(Q, np.float32)
    hot[int(rs.randint(Q))] = 1.0
    flat = np.full(Q, 1.0 / Q, np.float32)                            # one big tie
    return [("random", rnd), ("ties", ties), ("zeros", zeros), ("onehot", hot), ("flat", flat)]


def uniforms(Q, n=3):
    return list(np.random.RandomState(77 + Q).random_sample(n)) + [0.0, 1.0 - 2.0 ** -53]


def test_header_library_and_binding_carry_the_two_new_functions():
    hdr = open(os.path.join(ROOT, "include", "wavenet_hip.h")).read()
    assert re.search(r"int wn_decoder_set_sampling\(void\* handle, float temperature, int top_k, double top_p\);", hdr)
    assert re.search(r"int wn_sample_categorical_filtered\(const float\* prob, const double\* uniforms, int32_t\* out, int n, "
                     r"int Q, int top_k,\s+double top_p, void\* stream\);", hdr)
    assert "train_audio/generate.py:39" in hdr
    assert int(re.search(r"#define WN_ABI_VERSION (\d+)", hdr).group(1)) == 5 == _lib.ABI_VERSION
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("wn_decoder_set_sampling", "wn_sample_categorical_filtered"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    assert len(_lib.EXPORTS) == 69
    assert _lib.lib().wn_abi_version() == 5


def test_bad_sampling_arguments_are_refused_without_a_gpu():
    lib = _lib.lib()
    nan, inf = float("nan"), float("inf")
    fake = ctypes.c_void_p(0x1000)                       # never dereferenced: every call below is refused first
    assert lib.wn_decoder_set_sampling(None, 1.0, 0, 1.0) == _lib.WN_EARG and b"NULL" in lib.wn_last_error()
    for t in (0.0, -1.0, nan, inf, -inf):
        assert lib.wn_decoder_set_sampling(fake, t, 0, 1.0) == _lib.WN_EARG, t
        assert b"temperature" in lib.wn_last_error()
    assert lib.wn_decoder_set_sampling(fake, 1.0, -1, 1.0) == _lib.WN_EARG and b"top_k" in lib.wn_last_error()
    for tp in (0.0, -0.5, 1.0000001, 2.0, nan, inf):
        assert lib.wn_decoder_set_sampling(fake, 1.0, 0, tp) == _lib.WN_EARG, tp
        assert b"top_p" in lib.wn_last_error()
    p = 0x3000
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.wn_sample_categorical_filtered(*args, 1, 8, 2, 0.5, None) == _lib.WN_EARG
        assert b"NULL" in lib.wn_last_error()
    assert lib.wn_sample_categorical_filtered(p, p, p, 1, 8, -1, 0.5, None) == _lib.WN_EARG and b"top_k" in lib.wn_last_error()
    for tp in (0.0, -0.5, 1.0000001, nan, inf):
        assert lib.wn_sample_categorical_filtered(p, p, p, 1, 8, 2, tp, None) == _lib.WN_EARG, tp
        assert b"top_p" in lib.wn_last_error()
    # ... and the host module refuses the same values
    for bad in (dict(temperature=0.0), dict(temperature=nan), dict(temperature=inf), dict(top_k=-1), dict(top_p=0.0),
                dict(top_p=1.5), dict(top_p=nan)):
        with pytest.raises(ValueError):
            sampling.check_controls(**bad)
    sampling.check_controls(0.8, 40, 0.9)


@pytest.mark.parametrize("Q", QS)
def test_host_module_equals_the_literal_restatement(Q):
    n = 0
    for name, row in rows(Q):
        for k in top_ks(Q):
            for tp in TOP_PS:
                want_row = restate_filter(row, k, tp)
                got_row = sampling.filter_probs(row, k, tp)
                assert got_row.dtype == np.float32
                assert np.array_equal(got_row.view(np.uint32), want_row.view(np.uint32)), (name, Q, k, tp)
                first_max = int(np.argmax(row))                       # np.argmax: the first of equal maxima
                for u in uniforms(Q):
                    got = sampling.sample(row, u, k, tp)
                    assert got == restate_draw(want_row, u), (name, Q, k, tp, u)
                    if k == 1 or tp == 1e-9:
                        assert got == first_max, (name, Q, k, tp, u)
                    n += 1
    assert n == 5 * 5 * 4 * 5


def test_controls_off_is_the_plain_draw():
    for Q in QS:
        for name, row in rows(Q):
            assert np.array_equal(sampling.filter_probs(row, 0, 1.0), row)
            assert np.array_equal(sampling.filter_probs(row, Q, 1.0), row)
            for u in uniforms(Q):
                cdf = np.cumsum(row.astype(np.float64))
                cdf /= cdf[-1]
                assert sampling.sample(row, u) == int(np.searchsorted(cdf, u, side="right"))


def test_top_p_is_relative_to_the_mass_top_k_kept():
    row = np.asarray([0.4, 0.3, 0.2, 0.1], np.float32)
    # top-k 2 keeps {0.4, 0.3}: total 0.7; top-p 0.5 -> threshold 0.35: token 0 (before 0) stays, token 1 (before 0.4) goes
    assert sampling.filter_probs(row, 2, 0.5).tolist() == [np.float32(0.4), 0.0, 0.0, 0.0]
    # without top-k the threshold is 0.5 of 1.0: token 1 (before 0.4 < 0.5) stays
    assert sampling.filter_probs(row, 0, 0.5).tolist() == [np.float32(0.4), np.float32(0.3), 0.0, 0.0]
    # kept values are not renormalised
    assert sampling.filter_probs(row, 3, 1.0).tolist() == [np.float32(0.4), np.float32(0.3), np.float32(0.2), 0.0]


def test_temperature_factor_is_the_fp32_reciprocal():
    for t in (0.8, 0.7, 1.0, 1.3, 3.0):
        inv = sampling.inv_temperature(t)
        assert inv.dtype == np.float32 and inv == np.float32(1.0) / np.float32(t)
    lg = np.random.RandomState(3).standard_normal((4, 16)).astype(np.float32)
    p = sampling.apply_temperature(lg, 0.5)
    x = lg.astype(np.float64) * 2.0
    want = np.exp(x - x.max(-1, keepdims=True))
    want /= want.sum(-1, keepdims=True)
    np.testing.assert_allclose(p, want, atol=1e-6)
    assert sampling.per_utterance(0.8, 3) == [0.8] * 3 and sampling.per_utterance([1, 2], 2) == [1, 2]
    with pytest.raises(ValueError):
        sampling.per_utterance([1, 2], 3)


def test_cli_parses_the_three_flags_and_defaults_are_off():
    a = cli_args.parse([])
    assert (a.temperature, a.top_k, a.top_p) == (1.0, 0, 1.0)
    assert sampling.controls_off(a.temperature, a.top_k, a.top_p)
    a = cli_args.parse(["--fast", "--temperature", "0.8", "--top-k", "40", "--top-p", "0.9"])
    assert (a.fast, a.temperature, a.top_k, a.top_p) == (True, 0.8, 40, 0.9)
    assert not sampling.controls_off(a.temperature, a.top_k, a.top_p, 256)
