"""Float64 references, an error metric and error bars for the channel GEMMs of include/wavenet_hip.h -- numpy only, no GPU.

The five fp32-storage operations (formulas from the header):

    pointwise_fwd   out = W act(x) + b
    pointwise_bwd   dx = act'(x) * (W^T dout),  dW += dout^T act(x),  dbias += sum dout
    skip_fwd        skip[b,t,:] = sum_l (Ws_l z_l[b,t_off+t,:] + bs_l)          (+ skip when accumulate)
    skip_dz         dz_l = Ws_l^T dskip at t >= t_off, zero below
    skip_dw         dWs_l += dskip^T z_l,  dbs_l += sum dskip

Every operation is written ONCE, over an ``Arith``: the thing that says in which number format operands are held and how a
contraction ``A @ B`` is evaluated.  The same code therefore gives

    F64      the reference;
    F32      the YARDSTICK: the operation in float32 on the CPU (operands and accumulation in float32 -- the reference
             project's own arithmetic, it multiplies in float32, not code under test);
    ABS      the same contraction on absolute values, |A||B| (+ |b|, + |prefilled values| where the call accumulates): the
             denominator of the metric;
    RB64     float64 on operands rounded to bf16 once where the kernels round them: both operands of the contraction, `act`
             applied BEFORE the rounding, act'(x), biases and sums left in fp32 (k_split_w with one == 1 and the X split of
             k_colgemm_b3<.., 1, ..>, k_wgrad_b3<.., ONE>, k_wgrad_b3w<.., 1>; the bf16-storage path keeps x, W and dout as
             bf16 in memory) -- what WN_GEMM_BF16 and wn16_* are held against;
    B3, H2, BF16   numpy emulations of the operand splits of split_w.hpp / h2_ops.hpp / w16.hpp: three bf16 parts and six
             products, two fp16 parts behind a power-of-two scale and three products, one bf16 rounding.  Products of parts
             are exact in float32 and are accumulated in float32, as a matrix core does.  They exist to PROVE THE BARS
             (tests/test_channel_gemm_bars_cpu.py: the faithful form passes, every mutant fails); no GPU test compares
             against them.

Metric: |got - ref| / (|A||B| + ...) componentwise; its maximum and its RMS over the tensor (``measure``).
Bars: ``check`` -- see the comment above MULT_MAX / MULT_RMS.
"""
import numpy as np

from oracle.wavenet_ref import bf16_round

ACT_NONE, ACT_RELU, ACT_ELU = 0, 1, 2
MODES = ("fp32", "bf16x3", "bf16", "fp16x2")

# documented product error of a mode (include/wavenet_hip.h, mfma_gemm_b3.hip, split_w.hpp): the hard cap's p
PRODUCT_ERROR = {"fp32": 0.0, "bf16x3": 3 * 2.0 ** -27, "fp16x2": 2.0 ** -21, "bf16": 0.0}   # bf16: against RB64, so 0

H2_SCALE_UNIT = 16384.0     # kH2ScaleX: the fixed scale of an operand known to lie in [-1, 1] (z = tanh * sigmoid)


def rb32(a):
    """nearest bfloat16 (ties to even) of float32 values, as float32 (oracle.bf16_ref.rb without the widening)"""
    return bf16_round(np.asarray(a, dtype=np.float32))


def bf16_bits(a):
    """the raw bf16 bits (uint16) of values that are bf16 already"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf16_from_bits(u):
    return (np.ascontiguousarray(u, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_half_ulp(ref):
    """half a unit in the last place of a bf16 (8 significant bits) at |ref|: 2^(e - 8) for |ref| in [2^e, 2^(e+1)), which
    lies between 2^-9 |ref| and 2^-8 |ref| -- one bf16 rounding of a stored output"""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return np.where(a > 0, 2.0 ** (e - 8), 0.0)


# ---- arithmetics ------------------------------------------------------------------------------------------------------
class Arith(object):
    """dtype of the operands, the contraction, and whether operands are replaced by their absolute values (ABS)."""
    dtype = np.float64
    act_dtype = None            # the format act(x) is evaluated in; None: dtype
    absolute = False

    def prep(self, v):
        v = np.asarray(v).astype(self.dtype)
        return np.abs(v) if self.absolute else v

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        """A (n, k) @ B (k, m), added to acc when given.  a_unit / b_unit: the operand is known to lie in [-1, 1], b_max: the
        maximum the scale of B is taken from when it is not B's own (only the fp16 split cares)."""
        return A @ B if acc is None else acc + A @ B


class _F64(Arith):
    pass


class _F32(Arith):
    """The yardstick: float32 operands, every product rounded to float32, added term by term in k order to a float32 sum --
    the plainest float32 evaluation there is.  (One call of the BLAS on the whole contraction is float32 too, but how it
    blocks a long K, and with it its error at K in the thousands, is the BLAS build's own business: measured here, it was
    the same as this loop up to K = 256 and a quarter of it at K = 2,112.  The bars must not depend on the machine the
    test runs on.)"""
    dtype = np.float32

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        out = np.zeros((A.shape[0], B.shape[1]), np.float32) if acc is None else np.array(acc, dtype=np.float32)
        for k in range(A.shape[1]):
            out += A[:, k:k + 1] * B[k:k + 1]
        return out


class _Abs(Arith):
    absolute = True


class _RB64(Arith):
    act_dtype = np.float32      # the kernels evaluate act(x) in float32 and round THAT to bf16

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        out = rb32(A).astype(np.float64) @ rb32(B).astype(np.float64)
        return out if acc is None else acc + out


F64, F32, ABS, RB64 = _F64(), _F32(), _Abs(), _RB64()


def split3(x):
    """split_w.hpp split3: x = h + m + l, three bf16 parts (as float32)"""
    x = np.asarray(x, dtype=np.float32)
    h = rb32(x)
    r1 = x - h
    m = rb32(r1)
    return h, m, rb32(r1 - m)


B3_TERMS = ("hh", "hm", "mh", "mm", "hl", "lh")      # wh*xh + (wh*xm + wm*xh) + (wm*xm + wh*xl + wl*xh), mfma_gemm_b3.hip
B3_LOW_TERMS = ("mm", "hl", "lh")


class B3(Arith):
    """three bf16 parts per operand, the six products of magnitude >= 2^-18; float32 accumulation"""
    dtype = np.float32

    def __init__(self, terms=B3_TERMS):
        self.terms = tuple(terms)

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        pa, pb = dict(zip("hml", split3(A))), dict(zip("hml", split3(B)))
        out = np.zeros((A.shape[0], B.shape[1]), np.float32)
        for t in reversed(self.terms):                     # small terms first
            out = out + pa[t[0]] @ pb[t[1]]
        return out if acc is None else acc + out


def h2_scale_of(m):
    """split_w.hpp h2_scale_of: the power of two that brings max |x| = m just below 2^14"""
    m = float(m)
    if not (m > 0.0) or not (m < 3e38):
        return 1.0
    return float(np.ldexp(1.0, 14 - int(np.frexp(m)[1])))


def split2h(x):
    """split_w.hpp split2h: x = h + m, two fp16 parts (as float32)"""
    x = np.clip(np.asarray(x, dtype=np.float32), -65000.0, 65000.0)
    h = x.astype(np.float16).astype(np.float32)
    return h, (x - h).astype(np.float16).astype(np.float32)


H2_TERMS = ("hh", "hm", "mh")


class H2(Arith):
    """two fp16 parts per operand behind ONE power-of-two scale per operand (its measured maximum, or 2^14 for an operand
    in [-1, 1]), three products, float32 accumulation, unscaled at the end"""
    dtype = np.float32

    def __init__(self, terms=H2_TERMS):
        self.terms = tuple(terms)

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        sa = H2_SCALE_UNIT if a_unit else h2_scale_of(np.abs(A).max(initial=0.0))
        sb = H2_SCALE_UNIT if b_unit else h2_scale_of(np.abs(B).max(initial=0.0) if b_max is None else b_max)
        pa = dict(zip("hm", split2h(np.asarray(A, np.float32) * np.float32(sa))))
        pb = dict(zip("hm", split2h(np.asarray(B, np.float32) * np.float32(sb))))
        out = np.zeros((A.shape[0], B.shape[1]), np.float32)
        for t in reversed(self.terms):
            out = out + pa[t[0]] @ pb[t[1]]
        out = out * np.float32(1.0 / (sa * sb))
        return out if acc is None else acc + out


class BF16(Arith):
    """operands rounded to bf16 once, float32 accumulation"""
    dtype = np.float32

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        return rb32(A) @ rb32(B) if acc is None else acc + rb32(A) @ rb32(B)


EMULATION = {"fp32": F32, "bf16x3": B3(), "bf16": BF16(), "fp16x2": H2()}


class DropChunk(Arith):
    """mutant: one 32-wide chunk of the contraction is missing"""

    def __init__(self, inner, chunk=0):
        self.inner, self.chunk, self.dtype = inner, chunk, inner.dtype

    def mm(self, A, B, a_unit=False, b_unit=False, b_max=None, acc=None):
        A = np.array(A)
        k0 = 32 * self.chunk
        A[:, k0:k0 + 32] = 0
        return self.inner.mm(A, B, a_unit, b_unit, b_max, acc)


# ---- the operations, once, over an Arith ----------------------------------------------------------------------------
def act_apply(x, act):
    if act == ACT_RELU:
        return np.where(x > 0, x, 0).astype(x.dtype)
    if act == ACT_ELU:
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0))).astype(x.dtype)
    return x


def act_grad(x, act):
    if act == ACT_RELU:
        return (x > 0).astype(x.dtype)
    if act == ACT_ELU:
        return np.where(x > 0, 1, np.exp(np.minimum(x, 0))).astype(x.dtype)
    return np.ones_like(x)


def _a(ar, x, act):
    """act(x) in ar's format (ABS: its absolute value)"""
    return ar.prep(act_apply(np.asarray(x).astype(ar.act_dtype or ar.dtype), act))


def pointwise_fwd(ar, x, W, b, act):
    """x (N, Cin), W (Cout, Cin), b (Cout) or None -> out (N, Cout)"""
    out = ar.mm(_a(ar, x, act), ar.prep(W).T)
    return out if b is None else out + ar.prep(b).astype(out.dtype)


def pointwise_bwd(ar, x, W, dout, act, dW0=None, db0=None):
    """-> dx (N, Cin), dW (Cout, Cin), dbias (Cout); dW0 / db0: the values the call accumulates onto"""
    g = ar.prep(act_grad(np.asarray(x).astype(ar.dtype), act))
    dx = g * ar.mm(ar.prep(dout), ar.prep(W))
    dW = ar.mm(ar.prep(dout).T, _a(ar, x, act))
    db = ar.prep(dout).sum(axis=0)
    if dW0 is not None:
        dW = dW + ar.prep(dW0).astype(dW.dtype)
    if db0 is not None:
        db = db + ar.prep(db0).astype(db.dtype)
    return dx, dW, db


def skip_fwd(ar, z, Ws, bs, t_off, Tw, skip0=None, bias_times=1):
    """z[l] (B, T, cd_l), Ws[l] (Cs, cd_l), bs None or a list with None entries -> skip (B, Tw, Cs): the header's formula term
    by term into ONE running sum -- a layer's products, its bias, the next layer's products (so from the first bias on the
    sum sits at the biases' magnitude, however small z is: the yardstick owes a rounding at that magnitude per term, as any
    single-accumulator float32 evaluation does).  The fp16 split scales all the weights of the call by ONE power of two.
    bias_times: a mutant's knob."""
    B = z[0].shape[0]
    wmax = max(float(np.abs(w).max(initial=0.0)) for w in Ws)
    out = None
    for l, (zl, w) in enumerate(zip(z, Ws)):
        out = ar.mm(ar.prep(zl)[:, t_off:t_off + Tw].reshape(B * Tw, -1), ar.prep(w).T, a_unit=True, b_max=wmax, acc=out)
        if bs is not None and bs[l] is not None:
            out = out + (bias_times * ar.prep(bs[l])).astype(out.dtype)
    out = out.reshape(B, Tw, -1)
    return out if skip0 is None else out + ar.prep(skip0).astype(out.dtype)


def skip_dz(ar, Ws, dskip, T, t_off):
    """dskip (B, Tw, Cs) -> [dz_l (B, T, cd_l)]: ONE range for dskip and one for all the weights of the call"""
    B, Tw, Cs = dskip.shape
    Wc = np.concatenate([ar.prep(w) for w in Ws], axis=1)                 # (Cs, sum cd)
    full = ar.mm(ar.prep(dskip).reshape(B * Tw, Cs), Wc).reshape(B, Tw, -1)
    out, c0 = [], 0
    for w in Ws:
        dz = np.zeros((B, T, w.shape[1]), full.dtype)
        dz[:, t_off:t_off + Tw] = full[:, :, c0:c0 + w.shape[1]]
        out.append(dz)
        c0 += w.shape[1]
    return out


def skip_dw(ar, z, dskip, t_off, dW0=None, db0=None):
    """-> ([dWs_l (Cs, cd_l)], [dbs_l (Cs)]); dW0 / db0: lists of the values accumulated onto (entries may be None)"""
    B, Tw, Cs = dskip.shape
    D = ar.prep(dskip).reshape(B * Tw, Cs)
    dWs, dbs = [], []
    for l, zl in enumerate(z):
        dw = ar.mm(D.T, ar.prep(zl)[:, t_off:t_off + Tw].reshape(B * Tw, -1), b_unit=True)
        db = D.sum(axis=0)
        if dW0 is not None and dW0[l] is not None:
            dw = dw + ar.prep(dW0[l]).astype(dw.dtype)
        if db0 is not None and db0[l] is not None:
            db = db + ar.prep(db0[l]).astype(db.dtype)
        dWs.append(dw)
        dbs.append(db)
    return dWs, dbs


# ---- the two input families -------------------------------------------------------------------------------------------
def flat_activations(rs, n, k):
    return rs.randn(n, k).astype(np.float32)


def flat_weights(rs, m, k):
    """N(0, 1/K)"""
    return (rs.randn(m, k) / np.sqrt(k)).astype(np.float32)


def unit_activations(rs, *shape):
    """z = tanh * sigmoid lies in [-1, 1]"""
    return rs.uniform(-1.0, 1.0, shape).astype(np.float32)


def ranged(rs, a):
    """per-row magnitudes over six decades (tests/test_gpu_dz_weights_stationary.py): every row of the last axis scaled by
    10^-6u, u uniform in [0, 1)"""
    scale = 10.0 ** (-6.0 * rs.rand(*a.shape[:-1], 1))
    return (a * scale).astype(np.float32)


# ---- metric and bars --------------------------------------------------------------------------------------------------
def elu_rounding_slack(x):
    """WN_GEMM_BF16 rounds act(x) to bf16, and elu(x) = expm1(x) is only defined to an ulp or two of float32: where the float32
    value lies that close to the midpoint of two bf16 neighbours, the kernel's operand and RB64's may be DIFFERENT neighbours,
    both right.  Returns, per element of x, the distance between the bf16 roundings of the float32 value moved two ulps down
    and two ulps up: 0 almost everywhere (about four elements in 2^16 are that close to a midpoint), one bf16 ulp there."""
    a = act_apply(np.asarray(x, dtype=np.float32), ACT_ELU)
    lo = hi = a
    for _ in range(2):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    return np.abs(rb32(hi).astype(np.float64) - rb32(lo).astype(np.float64))


def measure(got, ref, den, out_bf16=False, slack=None):
    """(max, RMS) over the tensor of |got - ref| / den.  out_bf16: the output is stored as bf16 -- one bf16 rounding of the
    output (half a bf16 ulp at the reference value) is taken off the error first.  slack: an absolute allowance per element
    that the REFERENCE owes (elu_rounding_slack carried through the contraction), taken off as well.  Where den == 0 the
    contraction has no non-zero term: anything but the reference itself is an infinite error."""
    got, ref, den = (np.asarray(v, dtype=np.float64) for v in (got, ref, den))
    err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)          # a NaN left in an output
    if out_bf16:
        err = np.maximum(err - bf16_half_ulp(ref), 0.0)
    if slack is not None:
        err = np.maximum(err - slack, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0))
    return float(rel.max(initial=0.0)), float(np.sqrt(np.mean(rel ** 2))) if rel.size else 0.0


# The multiple of the float32 yardstick's error a kernel may show, for the maximum and the RMS of the metric separately.
# Chosen from two measurements, not in advance:
#   * the largest ratio kernel error / yardstick error the kernels show on an MI355X over every entry point, mode and case
#     of tests/test_gpu_channel_gemm_sweep.py (profiles/channel_gemm_error.json): 1.63 in the maximum (dWs of a three-row
#     window, k_wgrad_b3: its float atomics land in another order from run to run, 1.36 .. 1.63 over three runs) and 1.49
#     in RMS (the forward on rows over six decades: the kernel adds a source's bias ahead of its products, the yardstick
#     behind them);
#   * the smallest ratio mutant error / yardstick error any mutant of tests/test_channel_gemm_bars_cpu.py shows on the CPU:
#     3.27 in the maximum (K = 512, dWs) and 9.65 in RMS (K = 512, the forward), both from bf16x3 with its three low
#     product terms dropped; every other mutant is beyond 80.
# A multiple should sit above the first and below HALF the second.  In RMS it does: 1.49 < 2.5 < 4.83.  In the maximum there
# is no such number -- 1.63 against 3.27 / 2 = 1.63: at K = 512 a float32 accumulation's own worst element is a third of
# what the three dropped terms cost -- so the maximum's multiple is only held above the kernels, at 2.0, and it is the RMS
# bar that keeps every mutant at least twice over a bar (3.86 times, the nearest; the CPU test asserts 2).
# The yardstick's own figures are sample statistics of a float32 evaluation -- over a 32-element output the maximum of the
# metric is a noisy thing, and with one term per output (K = 1) it can be exactly 0 --, so they are floored at what ANY
# float32 evaluation owes: one rounding of the result, 2^-24 of it at the worst; uniform over the last place that is
# between 2^-24 / sqrt(12) = 2^-25.8 and twice that in RMS, floored here at 2^-26.  (At the shapes of the CPU test the
# yardstick's figures are 1.0e-7 .. 3.9e-7 and 1.7e-8 .. 6.3e-8: the floors do not bind there.)
MULT_MAX = 2.0
MULT_RMS = 2.5
YARD_FLOOR_MAX = 2.0 ** -24
YARD_FLOOR_RMS = 2.0 ** -26


PRODUCTS = {"fp32": 1, "bf16x3": 6, "bf16": 1, "fp16x2": 3}     # accumulator updates per term of the contraction


def hard_cap(mode, K):
    """the componentwise bound (K 2^-24 + p) on the metric, whatever the shape: the roundings of a float32 accumulation of K
    terms plus the mode's documented product error.  A split mode updates the accumulator once per product of the split, six
    or three times for the first term alone, so K counts never fewer updates than that: K + products - 1 (which is what
    decides at K = 1, a weight gradient over one row, and adds nothing to speak of at K >= 32)."""
    return (K + PRODUCTS[mode] - 1) * 2.0 ** -24 + PRODUCT_ERROR[mode]


def ratios(got, ref, den, yard, out_bf16=False, slack=None):
    """(max ratio, RMS ratio) of a result's metric to the (floored) yardstick's; yard = measure(F32 result, ref, den)"""
    mx, rms = measure(got, ref, den, out_bf16, slack)
    return mx / max(yard[0], YARD_FLOOR_MAX), rms / max(yard[1], YARD_FLOOR_RMS)


def check(got, ref, den, yard, mode, K, out_bf16=False, slack=None):
    """None when `got` is within the bars of `mode`, else a string saying which bar it misses and by how much.
    ref: F64 for fp32 / bf16x3 / fp16x2, RB64 for bf16 and the bf16-storage entry points (yard is always F32 against F64)."""
    mx, rms = measure(got, ref, den, out_bf16, slack)
    bar_max, bar_rms = MULT_MAX * max(yard[0], YARD_FLOOR_MAX), MULT_RMS * max(yard[1], YARD_FLOOR_RMS)
    cap = hard_cap(mode, K)
    if not mx <= cap:
        return "hard cap: max %.3g > (K 2^-24 + p) = %.3g (K = %d)" % (mx, cap, K)
    if not mx <= bar_max:
        return "max %.3g > %.1f x yardstick %.3g" % (mx, MULT_MAX, max(yard[0], YARD_FLOOR_MAX))
    if not rms <= bar_rms:
        return "RMS %.3g > %.1f x yardstick %.3g" % (rms, MULT_RMS, max(yard[1], YARD_FLOOR_RMS))
    return None


def check_ranged_fp16x2(got, ref, K, amax, wmax):
    """The ranged family under fp16x2: the split scales an operand by ONE power of two, so small rows lose bits by design;
    the bar is absolute, 2^-21 K max|A| max|W|."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    err = float(np.where(np.isfinite(err), err, np.inf).max(initial=0.0))
    bar = 2.0 ** -21 * K * float(amax) * float(wmax)
    return None if err <= bar else "ranged fp16x2: |err| %.3g > 2^-21 K max|A| max|W| = %.3g" % (err, bar)
