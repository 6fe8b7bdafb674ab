// Specialised persistent decode kernel for the shape of BASELINE.json config 4:
//   Q = 256, one causal layer (fw 2), Cr = Cd = 32, Cs = 256, residual fw 2, one head conv 256 -> 256,
//   no biases except the head's (the reference's defaults, wavenet.py:108,116-117,138) -- and, on WN_DECODER_GATE_ROWS handles,
//   gate biases and a frame table (global / local conditioning): "Gate rows" below, wave 1 only, the GATE instantiations.
// Same algorithm and state as k_decode in decoder.hip (FasterWaveNet._forward_one_step restated with
// rings instead of rolled windows); what changes is how ONE workgroup is used so that a step is not
// a chain of L2 round trips and wide barriers:
//   * 256 threads = one wave per SIMD;
//   * the 64 KB embedding table of the causal layer sits in LDS for the whole launch;
//   * the head's 256x256 weights live in registers for the whole launch (256 per thread: one wave
//     per SIMD owns the whole 512-entry register file);
//   * a layer's 13,312 weights are 52 per thread, fetched ONE LAYER AHEAD (the loads of layer l+1 are
//     in flight while layer l computes; the in-loop barriers wait for LDS only, never for vmcnt), as
//     is the ring column x[n-d] of the next layer;
//   * the waves are specialised.  Wave 0 alone runs the dependent chain of the 40 layers WITHOUT any barrier and
//     without an LDS round trip on the critical path: lane r owns gate row r (filter rows in lanes 0-31, gate rows in
//     32-63) with its 64 weights in registers, the x[n] it multiplies them with reaches it as 32 scalar broadcasts
//     (v_readlane -> SGPR operand of v_fmac), tanh and sigmoid are ONE exp + rcp sequence over the two half waves,
//     v_permlane32_swap brings filter and gate together, the residual projection is 32 more broadcast-FMAs per lane;
//     the x[n-d] half of the gate (known since the start of the step) comes from LDS broadcast reads off the critical
//     path.  (The previous form -- gate rows over 2 lanes, projection over 4, DPP reductions, z and x through LDS with
//     two workgroup barriers per layer -- took 1,650 cycles per layer.)
//     Wave 1 runs AHEAD of the chain: the x[n-d] half of every gate row depends only on the rings, which are known
//     when the step starts, so it computes all 40 layers' partial sums into LDS (its own copy of those weights, its
//     own layer counter) and the chain wave adds one float per row instead of 16 packed FMAs and 8 broadcast reads.
//     Waves 2-3 run the skip projection (61 % of the MACs) behind the chain from the table of z columns in LDS, two
//     rows per thread accumulated in registers over all 40 layers; they follow the chain through a layer counter in
//     LDS (LDS operations of a wave retire in order, so the counter store after the z store publishes it).
#include "wn_kernels.hpp"
#include "decoder_types.hpp"

namespace wn {

static constexpr int kFT = 256;      // waves 0-1: the dependent chain; waves 2-3: skip rows, one layer behind
static constexpr int kMaxFastLayers = 128;
static constexpr int kGateFloats = 4096, kProjFloats = 2048;
static constexpr int kLayerFloats = kGateFloats + kProjFloats + 8192;     // gate | residual projection (both half waves) | skip projection

__device__ __forceinline__ float dpp_f(float v, int ctrl_sel) {
    int r;
    switch (ctrl_sel) {
        case 101: r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xf, 0xf, true); break;  // quad xor 1
        default: r = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xf, 0xf, true); break;   // quad xor 2
    }
    return __int_as_float(r);
}
__device__ __forceinline__ float quad_allsum(float v) {
    v += dpp_f(v, 101);
    v += dpp_f(v, 102);
    return v;
}
// DPP moves: lane i <- lane i-n inside its 16-lane row (row_shr), or the previous row's last lane (row_bcast)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i(int old, int v) {
    return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ float wave_allmax(float v) {      // full-wave max, broadcast through an SGPR
    const int ninf = __float_as_int(-INFINITY);
    v = fmaxf(v, __int_as_float(dpp_i<0x111, 0xf>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x112, 0xf>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x114, 0xf>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x118, 0xf>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x142, 0xa>(ninf, __float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_i<0x143, 0xc>(ninf, __float_as_int(v))));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_allsum(float v) {
    v += __int_as_float(dpp_i<0x111, 0xf>(0, __float_as_int(v)));
    v += __int_as_float(dpp_i<0x112, 0xf>(0, __float_as_int(v)));
    v += __int_as_float(dpp_i<0x114, 0xf>(0, __float_as_int(v)));
    v += __int_as_float(dpp_i<0x118, 0xf>(0, __float_as_int(v)));
    v += __int_as_float(dpp_i<0x142, 0xa>(0, __float_as_int(v)));
    v += __int_as_float(dpp_i<0x143, 0xc>(0, __float_as_int(v)));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// inclusive prefix sum over the 64 lanes of a wave, float64 (both halves travel through the same DPP move)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_d(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = dpp_i<CTRL, ROW_MASK>(0, (int)(b & 0xffffffffll));
    const int hi = dpp_i<CTRL, ROW_MASK>(0, (int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_scan_f64(double v) {
    v += dpp_d<0x111, 0xf>(v);
    v += dpp_d<0x112, 0xf>(v);
    v += dpp_d<0x114, 0xf>(v);
    v += dpp_d<0x118, 0xf>(v);
    v += dpp_d<0x142, 0xa>(v);       // rows 1,3 += last lane of rows 0,2
    v += dpp_d<0x143, 0xc>(v);       // rows 2,3 += lane 31
    return v;
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// ---- packing: every per-lane weight group is a float4 at [plane][lane] (coalesced 16-byte loads) --
// chain wave, lane r = 0..63:  gate row r (0-31 filter channel r, 32-63 gate channel r-32), k = 4j + e over
//                              [x_old(32) | x_cur(32)]                                           (16 planes of 64 lanes)
//                              Wp row o = r % 32, k = 4j + e (both half waves hold the same rows)  (8 planes)
// skip threads t = 0..127:     rows cs = 2t (planes 0-7) and 2t+1 (planes 8-15), k = 4(j%8) + e
__global__ void k_pack_fast_layer(const float* __restrict__ Wf, const float* __restrict__ Wg,
                                  const float* __restrict__ Wp, const float* __restrict__ Ws,
                                  float* __restrict__ dst) {
    const int t = threadIdx.x;     // 0..127
    if (t < 64) {
        const int c = t & 31;
        const float* W = (t >> 5) ? Wg : Wf;
        for (int j = 0; j < 16; ++j)
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * j + e, tap = k >> 5, ch = k & 31;               // [x_old(32) | x_cur(32)]
                dst[(j * 64 + t) * 4 + e] = W[(c * 32 + ch) * 2 + tap];
            }
        for (int j = 0; j < 8; ++j)
            for (int e = 0; e < 4; ++e) dst[kGateFloats + (j * 64 + t) * 4 + e] = Wp[c * 32 + 4 * j + e];
    }
    for (int j = 0; j < 16; ++j)
        for (int e = 0; e < 4; ++e)
            dst[kGateFloats + kProjFloats + (j * 128 + t) * 4 + e] = Ws[(2 * t + (j >> 3)) * 32 + 4 * (j & 7) + e];
}
// head: row q = tid, k = 4j+e  ->  Ph[j][tid][4], j = 0..63
__global__ void k_pack_fast_head(const float* __restrict__ Wh, float* __restrict__ dst) {
    const int tid = threadIdx.x;
    for (int j = 0; j < 64; ++j)
        for (int e = 0; e < 4; ++e) dst[(j * 256 + tid) * 4 + e] = Wh[tid * 256 + 4 * j + e];
}

typedef float f4v __attribute__((ext_vector_type(4)));
struct ChainW { f4v g[8]; f4v p[8]; };            // gate rows, x[n] half | projection rows
struct OldW { float4 g[8]; };                      // gate rows, x[n-d] half (wave 1)
struct SkipW { float4 s[16]; };

// The chain wave's 16 loads of a layer: uniform layer base in an SGPR pair + one of four loop-invariant 32-bit lane
// offsets + an immediate (the immediate reaches 4 KB, the 16 planes of a layer span 16 KB).  Written as asm: from the C
// form hipcc built a 64-bit address per group in vector registers (eleven VALU / carry instructions per layer on the
// chain's critical path).  The loads are invisible to the compiler's counters: chain_run() waits for them itself
// (s_waitcnt vmcnt(0) at the top of the layer that uses them) and re-defines the registers behind that wait.
struct ChainOff { unsigned o[4]; };                // byte offsets 16 lane + 8192 + 4096 k
__device__ __forceinline__ ChainOff chain_offsets(int lane) {
    ChainOff c;
#pragma unroll
    for (int k = 0; k < 4; ++k) c.o[k] = 16u * lane + 8192u + 4096u * k;
    return c;
}
#define WN_CHAIN_LD(dst, off, imm) \
    asm volatile("global_load_dwordx4 %0, %1, %2 offset:" #imm : "=v"(dst) : "v"(off), "s"(b))
__device__ __forceinline__ void load_chain(ChainW& w, const float* __restrict__ P, int l, const ChainOff& c) {
    const float* b = P + (long long)l * kLayerFloats;
    WN_CHAIN_LD(w.g[0], c.o[0], 0); WN_CHAIN_LD(w.g[1], c.o[0], 1024); WN_CHAIN_LD(w.g[2], c.o[0], 2048); WN_CHAIN_LD(w.g[3], c.o[0], 3072);
    WN_CHAIN_LD(w.g[4], c.o[1], 0); WN_CHAIN_LD(w.g[5], c.o[1], 1024); WN_CHAIN_LD(w.g[6], c.o[1], 2048); WN_CHAIN_LD(w.g[7], c.o[1], 3072);
    WN_CHAIN_LD(w.p[0], c.o[2], 0); WN_CHAIN_LD(w.p[1], c.o[2], 1024); WN_CHAIN_LD(w.p[2], c.o[2], 2048); WN_CHAIN_LD(w.p[3], c.o[2], 3072);
    WN_CHAIN_LD(w.p[4], c.o[3], 0); WN_CHAIN_LD(w.p[5], c.o[3], 1024); WN_CHAIN_LD(w.p[6], c.o[3], 2048); WN_CHAIN_LD(w.p[7], c.o[3], 3072);
}
#undef WN_CHAIN_LD
// ... and the wait: everything this wave has in flight has landed, and no use of `w` can be scheduled above this point
__device__ __forceinline__ void chain_landed(ChainW& w) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(w.g[j]), "+v"(w.p[j]));
}
__device__ __forceinline__ void load_old(OldW& w, const float* __restrict__ P, int l, unsigned l4) {
    const float* b = P + (long long)l * kLayerFloats;
#pragma unroll
    for (int j = 0; j < 8; ++j) w.g[j] = *reinterpret_cast<const float4*>(b + j * 256 + l4);
}
__device__ __forceinline__ void load_skip(SkipW& w, const float* __restrict__ P, int l, unsigned t4) {
    const float* b = P + (long long)l * kLayerFloats + kGateFloats + kProjFloats;
#pragma unroll
    for (int j = 0; j < 16; ++j) w.s[j] = *reinterpret_cast<const float4*>(b + j * 512 + t4);
}

// LDS-only barrier: waits for this wave's LDS traffic, not for its outstanding global loads, so the
// one-layer-ahead weight prefetch stays in flight across it (__syncthreads() would drain vmcnt).
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// The LDS of the chain workgroup (the one workgroup of k_decode_fast, workgroup 0 of the nine): the carve-up is defined
// here once, as byte offsets; the launches ask for kBytes.
struct ChainLds {
    static constexpr int L = kMaxFastLayers;
    static constexpr size_t oElds = 0;                            // float [256][2][32] embedding table of the causal layer
    static constexpr size_t oXold = oElds + 256 * 2 * 32 * 4;     // float [L][32]   x_l[n-d] of every layer, fetched at step start
    static constexpr size_t oXcur = oXold + L * 32 * 4;           // float [L+1][32] x_l[n]: input of layer l (output of l-1)
    static constexpr size_t oZall = oXcur + (L + 1) * 32 * 4;     // float [L][32]   gate output of every layer of this step
    static constexpr size_t oHvec = oZall + L * 32 * 4;           // float [256]     activated skip sums (one-workgroup form)
    static constexpr size_t oLg = oHvec + 256 * 4;                // float [256]     logits / probabilities
    static constexpr size_t oRed = oLg + 256 * 4;                 // float [16]
    static constexpr size_t oCdf = oRed + 16 * 4;                 // double [256]
    static constexpr size_t oTok = oCdf + 256 * 8;                // int [4]: current token, previous token
    static constexpr size_t oRingt = oTok + 4 * 4;                // int [L] ring offset per layer
    static constexpr size_t oDmask = oRingt + L * 4;              // int [L] d - 1 (d is a power of two: fw = 2)
    static constexpr size_t oReady = oDmask + L * 4;              // int [4]: layers of this step whose z is in zall | whose aold is there
    static constexpr size_t oAold = oReady + 4 * 4;               // float [L][64] x[n-d] half of every gate row, from wave 1
    static constexpr size_t kBytes = oAold + L * 64 * 4;
    float *Elds, *xold, *xcur, *zall, *hvec, *lg, *red, *aold;
    double* cdf;
    int *s_tok, *ringt, *dmask, *ready, *ready_old;
    template <class T> static __device__ __forceinline__ T* at(float* sm, size_t off) {
        return reinterpret_cast<T*>(reinterpret_cast<char*>(sm) + off);
    }
    __device__ __forceinline__ explicit ChainLds(float* sm)
        : Elds(at<float>(sm, oElds)), xold(at<float>(sm, oXold)), xcur(at<float>(sm, oXcur)), zall(at<float>(sm, oZall)),
          hvec(at<float>(sm, oHvec)), lg(at<float>(sm, oLg)), red(at<float>(sm, oRed)), aold(at<float>(sm, oAold)),
          cdf(at<double>(sm, oCdf)), s_tok(at<int>(sm, oTok)), ringt(at<int>(sm, oRingt)), dmask(at<int>(sm, oDmask)),
          ready(at<int>(sm, oReady)), ready_old(at<int>(sm, oReady) + 1) {}
};
static_assert(ChainLds::kBytes == 152800, "the chain workgroup's LDS (launch attribute, one workgroup per CU) must not move");
static_assert(ChainLds::oCdf % 8 == 0 && ChainLds::oZall % 16 == 0, "cdf holds doubles; xold and zall are read as float4");

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float f4c(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ float bcast(float v, int k) {       // lane k's value as a scalar (SGPR) operand
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}

// The chain wave: one residual layer of one step.  xc = x_l[n] (channel lane % 32, valid in every lane); returns
// x_{l+1}[n].  Writes z to zall[l] and x_{l+1}[n] to xcur[l+1] (for the ring update), then publishes the layer.
// Hand-off protocol between the waves of the ONE workgroup of this kernel (all on one CU, all through LDS):
//   producer: data ds_writes ... counter ds_write, in that order in ITS instruction stream;
//   consumer: counter ds_read (spin) ... data ds_reads, in that order in its stream.
// What makes this sufficient is a property of the hardware, not of the HSA memory model: a CU has ONE LDS pipeline
// that executes the DS instructions of all its waves in the order they were issued, and a wave's DS instructions issue
// in program order -- so the data writes are in the array before the counter write is, and a read issued after the
// counter read that saw the new value is served after both.  The fences below are therefore wavefront-scope: they only
// stop the COMPILER from moving DS accesses across the counter access (a workgroup-scope release would add an
// s_waitcnt lgkmcnt(0) on the 40-layer critical path for an ordering the pipeline already gives).  gfx950-specific by
// construction, like everything else in this file; the 256-step golden trace of config 4
// (tests/test_gpu_baseline_configs.py) and the 16,000-step bench run would show a reordering as a token mismatch.
// The spin is bounded: a lost hand-off traps (kernel abort, reported by the next HIP call) instead of hanging the GPU.
__device__ __forceinline__ void wait_count(const int* c, int v) {               // *c >= v, then an acquire at compile level
    int spins = 0;
    while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > (1 << 24)) __builtin_trap();
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// Gate rows (WN_DECODER_GATE_ROWS handles; the GATE instantiations of the three kernels): what wave 1 adds to gate row `lane` of
// every layer besides the x[n-d] half -- the handle's static gate bias and the step's frame-table value, both known when the
// step starts.  A table row is laid out as wave 1's lanes are: flat layer l's 32 filter values at 64 l, its 32 gate values at
// 64 l + 32, so lane `lane` of layer l reads float 64 l + lane of the row -- one coalesced 256-byte read per layer --, and the
// static biases of a layer are 64 floats (bf | bg) at DecLayer.bfg of the utterance's OWN arena (never utterance 0's packed
// weights: under same_weights the utterances still differ in class and table).
// GateStep: one step's view, wave-uniform except the two offsets.
struct GateStep {
    const float* r0;          // row j of the step (NULL: no table)
    const float* r1;          // row j + 1 (NULL: repeat mode, or no table)
    float alpha;              // float(p % hop) / float(hop)
    const float* arena;
    int b_lo, b_hi;           // lane k holds DecLayer.bfg of layers k and 64 + k (< 0: the layer has no static bias)
};
struct GateB { float s, y0, y1; };                 // static bias | row j | row j + 1 of one layer, this lane's
__device__ __forceinline__ void load_gate(GateB& b, const GateStep& g, int l, int lane) {
    const int off = __builtin_amdgcn_readlane(l < 64 ? g.b_lo : g.b_hi, l & 63);      // uniform
    b.s = off >= 0 ? g.arena[off + lane] : 0.f;
    b.y0 = g.r0 ? g.r0[64 * l + lane] : 0.f;
    b.y1 = g.r1 ? g.r1[64 * l + lane] : 0.f;
}
// the step's view of utterance q's rows: `frow` = the table row of this step (walked by the step loop, gate_walk), `rem` = p % hop,
// `end` = one past the ring's last row (GateWalk.end; NULL: a flat table)
__device__ __forceinline__ GateStep gate_step(const DecUtt& q, const float* frow, const float* end, int rem, int nlayers, int lane) {
    GateStep g;
    g.r0 = frow;
    g.r1 = frow && q.fr.interp ? frow + q.fr.row : nullptr;
    if (end && g.r1 == end) g.r1 = q.fr.tab;           // ring: the row after the ring's last row is row 0 (flat: end is NULL)
    g.alpha = g.r1 ? __fdiv_rn((float)rem, (float)q.fr.hop) : 0.f;
    g.arena = q.arena;
    g.b_lo = lane < nlayers ? q.layers[lane].bfg : -1;
    g.b_hi = 64 + lane < nlayers ? q.layers[64 + lane].bfg : -1;
    return g;
}
// The table row of a launch's steps without a division per step: row and remainder of the first step once (pos0 / hop, a 64-bit
// division), then one increment per step.  Wave-uniform; every thread of the chain workgroup keeps it (scalar registers).
// A ring (DecFrames.ring, WN_DECODER_FRAME_RING): the walk starts at row j mod ring and returns to the ring's base when it
// reaches `end`, one past its last row -- one more uniform compare where the row moves on; a flat table has end == NULL, which
// no row pointer equals.
struct GateWalk { const float* frow; int rem; const float* end; };
__device__ __forceinline__ GateWalk gate_walk_open(const DecFrames& fr) {
    GateWalk w{nullptr, 0, nullptr};
    if (fr.tab) {
        const long long j = fr.pos0 / fr.hop;
        w.frow = fr.tab + (fr.ring ? j % fr.ring : j) * (long long)fr.row;
        w.rem = (int)(fr.pos0 - j * fr.hop);
        if (fr.ring) w.end = fr.tab + (long long)fr.ring * fr.row;
    }
    return w;
}
__device__ __forceinline__ void gate_walk_next(GateWalk& w, const DecFrames& fr) {
    if (w.frow && ++w.rem == fr.hop) {
        w.rem = 0;
        w.frow += fr.row;
        if (w.frow == w.end) w.frow = fr.tab;
    }
}
// (static bias or 0) + frame value: the any-shape decoder's rule (decode_steps), bias_lerp never contracted -- a table of
// zeros gives +0, the seed the unconditioned kernels start from
__device__ __forceinline__ float gate_seed_of(const GateB& b, const GateStep& g) {
    const float y = g.r1 ? bias_lerp(b.y0, b.y1, g.alpha) : b.y0;
    return __fadd_rn(b.s, y);
}
// wave 1: the x[n-d] half of gate row `lane` of layer l -> aold[l][lane]; `seed`: the row's bias (GATE), else 0
__device__ __forceinline__ void old_layer(const ChainLds& S, const OldW& w, int l, int lane, float seed) {
    const float* xo = S.xold + l * 32;                 // same address in every lane: broadcast reads
    f2 A0 = {seed, 0.f}, A1 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 x4 = *reinterpret_cast<const float4*>(xo + 4 * j);
        A0 = __builtin_elementwise_fma(f2{w.g[j].x, w.g[j].y}, f2{x4.x, x4.y}, A0);
        A1 = __builtin_elementwise_fma(f2{w.g[j].z, w.g[j].w}, f2{x4.z, x4.w}, A1);
    }
    S.aold[l * 64 + lane] = (A0.x + A0.y) + (A1.x + A1.y);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) __hip_atomic_store(S.ready_old, l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// The chain wave: one residual layer of one step.  xc = x_l[n] (channel lane % 32, valid in every lane); a_old = the
// x[n-d] half of this lane's gate row (from wave 1).  Returns x_{l+1}[n]; a_old is replaced by the next layer's.
// The next layer's a_old is requested at the TOP of this layer together with wave 1's counter (counter read first, data read
// second: the LDS pipeline serves them in that order, so a counter value >= l + 2 proves the data read saw wave 1's
// write) and looked at only at the bottom: two LDS round trips (the spin's read, then the data's) left the 40-layer
// critical path.  Wave 1 is normally many layers ahead; when it is not, the bounded spin and a second read follow.
// zx != NULL (three-workgroup form): z also goes to the skip workgroup, every lane's value in ONE 8-byte store together with
// the step's sequence number (flag-in-data: the reader spins on the entry itself, so no ordering between a data store and
// a flag store is needed and the chain never waits for a store).
typedef unsigned long long u64;
__device__ __forceinline__ void xput(u64* p, float v, unsigned seq) {
    __hip_atomic_store(p, ((u64)seq << 32) | (u64)__float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Cross-workgroup waits never trap and never hang: an entry that does not arrive within ~1-2 s is given up -- the waiting
// thread marks the launch void in the error entry (x_err: read by wn_decoder_status) and from then on waits for nothing
// (`dead`), so every workgroup still runs to the end of the launch and the HIP context survives; the tokens of such a run
// are garbage and the host is told so.  (It happens when the nine workgroups are not all resident: a device with fewer
// free CUs than workgroups, other work holding them for seconds.)
__device__ __forceinline__ float xget(const u64* p, unsigned seq, u64* err, bool& dead) {
    int spins = 0;
    u64 w = 0;
    if (dead) return 0.f;
    while ((unsigned)((w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != seq) {
        __builtin_amdgcn_s_sleep(1);
        ++spins;
        // after a while also look at the error entry: when another workgroup has given up, this entry may never come
        if (spins > (1 << 21) || ((spins & 0xfff) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            __hip_atomic_store(err, (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dead = true;
            return 0.f;
        }
    }
    return __uint_as_float((unsigned)w);
}
__device__ __forceinline__ float chain_layer(const ChainLds& S, const ChainW& w, float& a_old, int l, const bool more,
                                             int lane, float xc) {
    int c_next = 0;
    float a_next = 0.f;
    if (more) {
        c_next = __hip_atomic_load(S.ready_old, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        a_next = S.aold[(l + 1) * 64 + lane];
    }
    // gate row `lane`: 32 scalar broadcasts of x[n], all read before the first use (a v_readlane result needs wait
    // states before a VALU may consume it: batched, the FMAs need no s_nop); packed FMAs (v_pk_fma_f32: two MACs per
    // instruction, the scalar pair as an SGPR operand), two accumulator pairs
    float sx[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) sx[k] = bcast(xc, k);
    f2 A0 = {a_old, 0.f}, A1 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        A0 = __builtin_elementwise_fma(f2{sx[4 * j], sx[4 * j + 1]}, f2{w.g[j].x, w.g[j].y}, A0);
        A1 = __builtin_elementwise_fma(f2{sx[4 * j + 2], sx[4 * j + 3]}, f2{w.g[j].z, w.g[j].w}, A1);
    }
    const float acc = (A0.x + A0.y) + (A1.x + A1.y);
    // tanh (lanes 0-31) and sigmoid (lanes 32-63) as one sequence: 1 - 2/(1 + e^{2a})  |  1/(1 + e^{-g})
    const bool lo = lane < 32;
    const float r = __builtin_amdgcn_rcpf(1.0f + __expf(lo ? 2.0f * acc : -acc));
    const float act = lo ? 1.0f - 2.0f * r : r;
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(act), __float_as_uint(act), false, false);
    const float z = __uint_as_float(sw[0]) * __uint_as_float(sw[1]);          // z[lane % 32] in every lane
    S.zall[l * 32 + (lane & 31)] = z;                  // both half waves hold the same value: no exec-mask branch
    // residual projection row lane % 32
    float sz[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) sz[k] = bcast(z, k);
    f2 P0 = {0.f, 0.f}, P1 = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        P0 = __builtin_elementwise_fma(f2{sz[4 * j], sz[4 * j + 1]}, f2{w.p[j].x, w.p[j].y}, P0);
        P1 = __builtin_elementwise_fma(f2{sz[4 * j + 2], sz[4 * j + 3]}, f2{w.p[j].z, w.p[j].w}, P1);
    }
    const float xn = ((P0.x + P0.y) + (P1.x + P1.y)) + xc;
    S.xcur[(l + 1) * 32 + (lane & 31)] = xn;
    // publish: LDS operations of a wave retire in order, so the counter store only has to FOLLOW the z store in the
    // instruction stream (a compiler-level fence; no s_waitcnt on the chain's critical path)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) __hip_atomic_store(S.ready, l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (more) {
        if (__builtin_expect(__builtin_amdgcn_readfirstlane(c_next) < l + 2, 0)) {       // rare: wave 1 has not been here yet
            wait_count(S.ready_old, l + 2);
            a_next = S.aold[(l + 1) * 64 + lane];
        }
        a_old = a_next;
    }
    return xn;
}
__device__ __forceinline__ void wait_layer(const ChainLds& S, int l) { wait_count(S.ready, l); }   // z of layers < l is in zall

// skip waves: rows 2t and 2t+1 of Ws_l z_l, accumulated over the layers
__device__ __forceinline__ void skip_layer(const ChainLds& S, const SkipW& w, int l, float& s0, float& s1) {
    const float* z = S.zall + l * 32;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float4 z4 = *reinterpret_cast<const float4*>(z + 4 * j);
        s0 += dot4(w.s[j], z4);
        s1 += dot4(w.s[8 + j], z4);
    }
}

static constexpr int kUnroll = 10;      // layers per trip of the layer loop (one block of the 4 x 10 stack)

// The chain wave's walk over the layers of one step.  Layer l's weights were requested a whole layer ago (an L2 hit lands in
// a fifth of that): the wait in front of the next request costs nothing.
// WHOLE: the stack is a whole number of kUnroll-layer trips (the 4 x 10 stack is): "is there a layer l?" and "is there a
// layer l + 1?" are then compile-time facts for nine layers of ten -- each was three scalar branches on the chain's
// critical path.
template <bool WHOLE>
__device__ __forceinline__ float chain_run(const ChainLds& S, const float* __restrict__ P, int nlayers, int lane, float xc,
                                           float a_old, ChainW (&w)[2], const ChainOff& co) {   // w[0]: layer 0's weights, requested by the caller
    for (int l0 = 0; l0 < nlayers; l0 += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int l = l0 + u;
            if (WHOLE || l < nlayers) {
                const bool more = WHOLE && u + 1 < kUnroll ? true : l + 1 < nlayers;
                chain_landed(w[u & 1]);                      // requested a whole layer ago
                if (more) load_chain(w[(u + 1) & 1], P, l + 1, co);   // in flight during layer l
                xc = chain_layer(S, w[u & 1], a_old, l, more, lane, xc);
            }
        }
    }
    return xc;
}

// ---- the stages of a step that both kernels run in their chain workgroup, once each --------------------------------
// Prologue: embedding table and ring tables to LDS, the token pair; ends in a barrier.  Returns this thread's head bias.
__device__ __forceinline__ float chain_prologue(const ChainLds& S, const DecUtt& q, int nlayers, int tid) {
    for (int i = tid; i < 256 * 2 * 32 / 4; i += kFT)
        reinterpret_cast<float4*>(S.Elds)[i] = reinterpret_cast<const float4*>(q.E)[i];
    for (int i = tid; i < nlayers; i += kFT) { S.ringt[i] = q.layers[i].ring; S.dmask[i] = q.layers[i].d - 1; }
    const float hb = q.hbias ? q.hbias[tid] : 0.f;
    if (tid == 0) { S.s_tok[0] = q.first_token; S.s_tok[1] = q.tok_ring[0]; }     // fwc = 2: ring depth 1
    __syncthreads();
    return hb;
}
// every layer's x[n-d] was written at least one step ago: fetch them all, off the layer chain
__device__ __forceinline__ void fetch_xold(const ChainLds& S, const float* __restrict__ arena, int nlayers, unsigned n, int tid) {
    for (int i = tid; i < nlayers * 32; i += kFT) {
        const int l = i >> 5;
        S.xold[i] = arena[S.ringt[l] + (long long)(n & (unsigned)S.dmask[l]) * 32 + (i & 31)];
    }
}
// layer 0's input from the embedding table; nothing of this step is published yet
__device__ __forceinline__ void open_step(const ChainLds& S, int token, int tprev, int tid) {
    if (tid < 32) S.xcur[tid] = S.Elds[(tprev * 2 + 0) * 32 + tid] + S.Elds[(token * 2 + 1) * 32 + tid];
    if (tid == 0) {
        __hip_atomic_store(S.ready, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(S.ready_old, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
// Waves 0 and 1 of a step.  Each meets ONE workgroup barrier, behind its first weight request: the other waves of the
// workgroup meet theirs at the same point of the step.
__device__ __forceinline__ void chain_wave(const ChainLds& S, const float* __restrict__ P, int nlayers, int lane) {
    ChainW w[2];
    const ChainOff co = chain_offsets(lane);
    load_chain(w[0], P, 0, co);
    __syncthreads();
    const float xc0 = S.xcur[lane & 31];
    wait_count(S.ready_old, 1);
    const float a0 = S.aold[lane];
    // The partial-trip walk (a stack that is no whole number of ten-layer trips) is entered with layer 0's weights LANDED: on the
    // way into chain_run<false> hipcc copied all 64 registers of w[0] to others, between the request above and the wait at the
    // top of the walk -- a copy of registers a load still in flight had not written (stale weights for layer 0 whenever the load
    // was slow: the first launch on cold caches, then intermittently; a six-layer stack's tokens differed from run to run).
    // The wait costs nothing: the walk begins with the same one.  The whole-trip walk is entered as ever.
    if (nlayers % kUnroll == 0) {
        chain_run<true>(S, P, nlayers, lane, xc0, a0, w, co);
    } else {
        chain_landed(w[0]);
        chain_run<false>(S, P, nlayers, lane, xc0, a0, w, co);
    }
}
// GATE: every row starts from its bias (gate rows above), fetched like the weights -- one layer ahead, off the chain.  The
// hand-off to the chain wave (aold, ready_old) is the same with and without: nothing is waited for that was not before.
template <bool GATE>
__device__ __forceinline__ void old_wave(const ChainLds& S, const float* __restrict__ P, int nlayers, int lane, const DecUtt& q,
                                         const GateWalk& gw) {
    OldW wo[2];
    GateB gb[2] = {};
    GateStep g{};
    load_old(wo[0], P, 0, 4u * lane);
    if (GATE) {
        g = gate_step(q, gw.frow, gw.end, gw.rem, nlayers, lane);
        load_gate(gb[0], g, 0, lane);
    }
    __syncthreads();
    for (int l0 = 0; l0 < nlayers; l0 += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int l = l0 + u;
            if (l < nlayers) {
                __builtin_amdgcn_s_waitcnt(0x0F70);          // as in the chain wave: exact counters
                if (l + 1 < nlayers) {
                    load_old(wo[(u + 1) & 1], P, l + 1, 4u * lane);
                    if (GATE) load_gate(gb[(u + 1) & 1], g, l + 1, lane);
                }
                old_layer(S, wo[u & 1], l, lane, GATE ? gate_seed_of(gb[u & 1], g) : 0.f);
            }
        }
    }
}
// Thread `tid` holds logit `tid`: temperature, then softmax over the 256.  Returns probability `tid`.  (The three lines
// that store the row stay with the callers: with them in here, hipcc's k_decode_fast went from 346 VGPRs to 512 and 800 spills.)
__device__ __forceinline__ float softmax_row(const ChainLds& S, float v, float inv_temp, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    if (inv_temp != 1.f) v *= inv_temp;            // temperature (uniform branch: a kernel argument)
    float m = wave_allmax(v);
    if (lane == 0) S.red[wv] = m;
    lds_barrier();
    m = fmaxf(fmaxf(S.red[0], S.red[1]), fmaxf(S.red[2], S.red[3]));
    const float e = expf(v - m);
    float s = wave_allsum(e);
    if (lane == 0) S.red[4 + wv] = s;
    lds_barrier();
    s = S.red[4] + S.red[5] + S.red[6] + S.red[7];
    return e * (1.f / s);
}
// The draw from the row in S.lg with the uniform u_draw: the token to *out_token and into the token pair.
// `given` (WN_DECODER_FORCED_TOKENS launches, the FORCED instantiations; the constant -1 in every other one, where the test folds
// away and the draw is the code it was): what *out_token held when the step began, the same value in every thread.  A token of [0, 256) is emitted as it is -- no filter, no scan, no exact fallback;
// *out_token holds it already; it enters the token pair as a drawn one does -- and anything else draws.  The compare is unsigned:
// a garbage entry cannot index outside the embedding table.  The branch is uniform over the workgroup and the given path meets
// no barrier, so the callers' closing barrier stays matched; the row in S.lg is left as the softmax wrote it (store_chosen).
__device__ __forceinline__ void draw_token(const ChainLds& S, const SampleCtl& sc, double u_draw, int token,
                                           int32_t* __restrict__ out_token, int tid, int given) {
    const int lane = tid & 63, wv = tid >> 6;
    if ((unsigned)given < 256u) {
        if (tid == 0) {
            S.s_tok[1] = token;
            S.s_tok[0] = given;
        }
        return;
    }
    float* lg = S.lg;
    double* cdf = S.cdf;
    int* red = reinterpret_cast<int*>(S.red);
    // top-k / top-p (uniform branch): the row in lg is truncated in place between the barrier above and the draw,
    // which then runs on it unchanged; LDS only
    if (sc.top_k > 0 || sc.top_p < 1.0) sample_filter<true>(lg, 256, tid, kFT, sc.top_k, sc.top_p);
    // numpy: cdf = cumsum(float64(p)); cdf /= cdf[-1]; first index with cdf > u.  The running sum is a
    // 256-long dependent chain (9.5 k cycles); a parallel scan associates differently, so its cdf may differ
    // from numpy's by a few ulp (<= 256 * 2^-53).  It is therefore used only when no cdf_i / total lies within
    // 1e-12 of u -- then both orders give the same index, provably -- and the exact chain runs otherwise.
    double c = wave_scan_f64((double)lg[tid]);
    if (lane == 63) cdf[wv] = c;                   // wave totals
    lds_barrier();
    {
        const double w0 = cdf[0], w1 = cdf[1], w2 = cdf[2], w3 = cdf[3];
        c += wv > 0 ? w0 : 0.0;
        c += wv > 1 ? w1 : 0.0;
        c += wv > 2 ? w2 : 0.0;
        const double tot = ((w0 + w1) + w2) + w3;
        const double q = c / tot;
        const bool gt = q > u_draw;
        const bool near = fabs(q - u_draw) < 1e-12;
        const unsigned long long bal = __ballot(gt), nb = __ballot(near);
        if (lane == 0) {
            red[8 + wv] = bal ? wv * 64 + __ffsll((long long)bal) - 1 : 256;
            red[12 + wv] = nb ? 1 : 0;
        }
    }
    lds_barrier();
    const bool ambiguous = (red[12] | red[13] | red[14] | red[15]) != 0;     // uniform over the workgroup
    if (ambiguous) {
        if (tid == 0) {                    // numpy's float64 running sum, in index order
            double cs = 0.0;
            for (int i = 0; i < 256; ++i) { cs += (double)lg[i]; cdf[i] = cs; }
        }
        lds_barrier();
        {
            const double tot = cdf[255];
            const bool gt = cdf[tid] / tot > u_draw;
            const unsigned long long bal = __ballot(gt);
            lds_barrier();
            if (lane == 0) red[8 + wv] = bal ? wv * 64 + __ffsll((long long)bal) - 1 : 256;
        }
        lds_barrier();
    }
    if (tid == 0) {
        int idx = min(min(red[8], red[9]), min(red[10], red[11]));
        if (idx > 255) idx = 255;
        *out_token = idx;
        S.s_tok[1] = token;
        S.s_tok[0] = idx;
    }
}

// WN_DECODER_TRACE_CHOSEN (the CHOSEN instantiations of the three kernels: the host takes them when prob_stride == kProbChosen,
// and the others execute what they executed before the flag existed): step `it`'s trace is one float, the drawn token's
// entry of the row the draw consumed.  Behind the step's closing barrier the token is in s_tok[0] and the row still in lg
// (thread `tid` rewrites lg[tid] itself, next step); the filter left a kept entry as it was and the drawn token is a kept
// one, so the thread that owns it stores the float the full-row form writes at [it * Q + token].  One ordinary per-lane
// store per step; the full-row write and this one exclude each other (an instantiation has one or the other).
__device__ __forceinline__ void store_chosen(const ChainLds& S, float* __restrict__ prob_out, int it, int tid) {
    if (prob_out && tid == S.s_tok[0]) prob_out[it] = S.lg[tid];
}

// FORCED (WN_DECODER_FORCED_TOKENS handles; the host takes these instantiations for do_sample == kSampleGiven): out_tokens[it] is
// read at the top of step `it`, off the chain, and handed to draw_token.  A template parameter like CHOSEN, not a run-time test: as
// a value of do_sample it cost every existing instantiation of k_decode_fast and most of k_decode_fast3 a register (DESIGN.md,
// "Given samples in the decode loop"); so the other instantiations are, instruction for instruction, what they were.
template <bool GATE, bool CHOSEN, bool FORCED>   // GATE: wave 1 seeds the gate rows with the handle's biases and table rows (gate rows, above)
__global__ __launch_bounds__(kFT, 1) void k_decode_fast(const DecUtt q, int nlayers, int nsteps, int prob_stride,
                                                        int apply_softmax, int do_sample, int head_act) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ChainLds S(sm);
    const float* P = q.P;
    const float* Ph = P + (size_t)nlayers * kLayerFloats;
    float* hvec = S.hvec;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float hb = chain_prologue(S, q, nlayers, tid);
    const unsigned t4 = 4u * (tid & 127);
    GateWalk gw{nullptr, 0, nullptr};
    if (GATE) gw = gate_walk_open(q.fr);

    for (int it = 0; it < nsteps; ++it) {
        const unsigned n = (unsigned)(q.n0 + it);
        const int token = S.s_tok[0], tprev = S.s_tok[1];
        const double u_draw = do_sample ? q.uniforms[it] : 0.0;      // fetched here, used after the network
        const int f_tok = FORCED && do_sample ? q.out_tokens[it] : -1;           // ... and the entry a given step emits (draw_token)
        fetch_xold(S, q.arena, nlayers, n, tid);
        open_step(S, token, tprev, tid);
        if (wv == 0) {
            chain_wave(S, P, nlayers, lane);
        } else if (wv == 1) {
            old_wave<GATE>(S, P, nlayers, lane, q, gw);
        } else {
            float skip0 = 0.f, skip1 = 0.f;
            SkipW w[2];
            load_skip(w[0], P, 0, t4);
            __syncthreads();
            for (int l0 = 0; l0 < nlayers; l0 += kUnroll) {
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const int l = l0 + u;
                    if (l < nlayers && l > 0) {
                        // behind the chain: fetch layer l's rows, use layer l-1's (loaded a trip ago) once its z is there
                        __builtin_amdgcn_s_waitcnt(0x0F70);
                        load_skip(w[u & 1], P, l, t4);
                        wait_layer(S, l);
                        skip_layer(S, w[(u + 1) & 1], l - 1, skip0, skip1);
                    }
                }
            }
            wait_layer(S, nlayers);
            if ((nlayers - 1) & 1) skip_layer(S, w[1], nlayers - 1, skip0, skip1);
            else skip_layer(S, w[0], nlayers - 1, skip0, skip1);
            hvec[2 * (tid - 128)] = act_apply(skip0, head_act);
            hvec[2 * (tid - 128) + 1] = act_apply(skip1, head_act);
        }
        // ---- head on the newest column: thread q owns logit q; its 256 weights stream in from L2 -------
        float v;
        {
            const float* Phs = Ph;
            asm volatile("" : "+s"(Phs));                 // keep the loads here (no hoisting above the layer loop)
            const unsigned q4 = 4u * tid;
            float4 wa[16], wb[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) wa[j] = *reinterpret_cast<const float4*>(Phs + j * 1024 + q4);
#pragma unroll
            for (int j = 0; j < 16; ++j) wb[j] = *reinterpret_cast<const float4*>(Phs + (16 + j) * 1024 + q4);
            lds_barrier();                                // the chain has written every x_cur, the skip waves hvec
                                                          // (LDS only: the weight loads stay in flight)
            // this step's x_cur of every layer becomes the newest ring column
            for (int i = tid; i < nlayers * 32; i += kFT) {
                const int l = i >> 5;
                q.arena[S.ringt[l] + (long long)(n & (unsigned)S.dmask[l]) * 32 + (i & 31)] = S.xcur[i];
            }
            float p0 = hb, p1 = 0.f, p2 = 0.f, p3 = 0.f;
#define HEAD_ACC(W, J0)                                                                                   \
    _Pragma("unroll") for (int j = 0; j < 16; j += 4) {                                                   \
        p0 += dot4(W[j], *reinterpret_cast<const float4*>(hvec + 4 * ((J0) + j)));                        \
        p1 += dot4(W[j + 1], *reinterpret_cast<const float4*>(hvec + 4 * ((J0) + j) + 4));                \
        p2 += dot4(W[j + 2], *reinterpret_cast<const float4*>(hvec + 4 * ((J0) + j) + 8));                \
        p3 += dot4(W[j + 3], *reinterpret_cast<const float4*>(hvec + 4 * ((J0) + j) + 12));               \
    }
            HEAD_ACC(wa, 0)
#pragma unroll
            for (int j = 0; j < 16; ++j) wa[j] = *reinterpret_cast<const float4*>(Phs + (32 + j) * 1024 + q4);
            HEAD_ACC(wb, 16)
#pragma unroll
            for (int j = 0; j < 16; ++j) wb[j] = *reinterpret_cast<const float4*>(Phs + (48 + j) * 1024 + q4);
            HEAD_ACC(wa, 32)
            HEAD_ACC(wb, 48)
#undef HEAD_ACC
            v = (p0 + p1) + (p2 + p3);
        }
        if (apply_softmax) v = softmax_row(S, v, q.sc.inv_temp, tid);
        S.lg[tid] = v;
        if (!CHOSEN && q.prob_out) q.prob_out[(long long)it * prob_stride + tid] = v;
        lds_barrier();
        if (do_sample) draw_token(S, q.sc, u_draw, token, q.out_tokens + it, tid, FORCED ? __builtin_amdgcn_readfirstlane(f_tok) : -1);
        else if (tid == 0) S.s_tok[1] = token;
        __syncthreads();                           // full barrier: orders this step's ring stores before the next step's loads
        if (CHOSEN) store_chosen(S, q.prob_out, it, tid);
        if (GATE) gate_walk_next(gw, q.fr);
    }
    if (tid == 0) q.tok_ring[0] = S.s_tok[1];      // the token before the next one to be consumed
}

// ---------------------------------------------------------------------------------------------
// The same decode on NINE workgroups (nine CUs).  A step of k_decode_fast streams 2.5 MB of fp32 weights into one CU --
// 69.5 k cycles at the 36 B/clk one CU gets out of L2, which is the step time whatever the four waves do (DESIGN.md,
// round 3) -- and runs head, softmax and sampling (18 k cycles) behind the 40-layer chain.  Here
//   workgroup 0      keeps the chain (wave 0), the x[n-d] halves (wave 1), softmax and the numpy-compatible sampler; its
//                    wave 2 follows the chain through the LDS layer counter and publishes every layer's z to the others
//                    (the chain wave itself must not store: vector-memory operations retire in order, and a write-through
//                    store in its queue held back the next layer's weight loads -- 60 k cycles for the chain instead of 49);
//   workgroups 1..8  own 32 skip rows each and keep their slice of ALL layers' skip weights in REGISTERS for the whole
//                    launch (thread = (row, eighth of the 32 gate channels): one float4 per layer, 40 float4): no weight
//                    streaming, a layer costs four FMAs; they poll eight layers of z per memory round trip;
//                    and, having their 32 activated skip values, add those columns' share of EVERY logit (thread q: 32 more
//                    resident weights of head row q) -- workgroup 0 adds the eight shares: no separate head hop.
// Exchange is through `X` in device memory, flag-in-data: every float travels in an 8-byte entry with the step's
// sequence number (xput / xget above), written once and polled by its reader; entries are zeroed by a kernel before the
// launch.  Two hops follow the chain's last layer (z -> partial logits -> workgroup 0).  Skip rows and logits are summed
// in another order than k_decode_fast's (eight partial sums per row added pairwise; eight shares per logit): probabilities agree to rounding
// (~1e-7), not bit for bit; the launch itself is deterministic.  At most 40 layers (the weights must fit the registers).
// ---------------------------------------------------------------------------------------------
static constexpr int kXZ = 0;                                   // X layout (u64 entries): z [L][64] | partial logits [8][256]
static constexpr int kD10MaxL = 40;
static constexpr int kD10Skip = 8;                              // skip workgroups
__device__ __host__ __forceinline__ int x_pl(int nlayers) { return nlayers * 64; }
__device__ __host__ __forceinline__ int x_err(int nlayers) { return x_pl(nlayers) + kD10Skip * 256 + 8; }   // != 0: a wait gave up, the run is void
__device__ __host__ __forceinline__ int x_entries(int nlayers) { return x_err(nlayers) + 8; }   // the whole area, error entry inside
// X lives behind the packed weights of its handle: layers | head | X (decode_fast_pack_floats)
static u64* x_area(const float* P, int nlayers) {
    return reinterpret_cast<u64*>(const_cast<float*>(P) + (size_t)nlayers * kLayerFloats + 256 * 256);
}

// `wg`: this workgroup's role in its utterance's group of nine (0 = chain, 1..8 = skip rows): blockIdx.x for one utterance,
// blockIdx.x % 9 in the batched launch (k_decode_fast3_batch)
template <bool GATE, bool CHOSEN, bool FORCED>
__device__ __forceinline__ void decode_fast3_body(const int wg, const DecUtt& q, int nlayers, int nsteps, int prob_stride,
                                                  int apply_softmax, int do_sample, int head_act) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* P = q.P;
    const float* Ph = P + (size_t)nlayers * kLayerFloats;
    u64* X = q.X;

    if (wg >= 1 && wg <= kD10Skip) {
        // ---- 32 skip rows: thread (r = tid / 8, s = tid % 8) holds Ws_l[row][4 s .. 4 s + 3] of every layer ----
        float* zs = sm;                                               // [L][32]
        float* hs = sm + kD10MaxL * 32;                               // [32]
        const int row = 32 * (wg - 1) + (tid >> 3), sl = tid & 7;
        float4 wh[8];                                                 // head row `tid`, the 32 columns of this workgroup's skip rows
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) wh[jj] = *reinterpret_cast<const float4*>(Ph + (8 * (wg - 1) + jj) * 1024 + 4 * tid);
        float4 w[kD10MaxL];
#pragma unroll
        for (int l = 0; l < kD10MaxL; ++l)
            w[l] = l < nlayers ? *reinterpret_cast<const float4*>(P + (long long)l * kLayerFloats + kGateFloats + kProjFloats +
                                                                  ((row & 1) * 8 + sl) * 512 + 4 * (row >> 1))
                               : make_float4(0.f, 0.f, 0.f, 0.f);
        bool dead = false;                                            // a wait of this thread gave up: wait for nothing any more
        for (int it = 0; it < nsteps; ++it) {
            const unsigned seq = (unsigned)(it + 1);
            float acc = 0.f;
#pragma unroll
            for (int l0 = 0; l0 < kD10MaxL; l0 += 8) {
                if (l0 < nlayers) {
                    // a poll is a round trip to memory: the four waves fetch EIGHT layers per round trip (wave w the layers
                    // l0 + 2 w and l0 + 2 w + 1, one per half wave) into a shared table; the chain needs ~0.55 us per layer
                    const int lp = l0 + 2 * wv + (lane >> 5);
                    if (lp < nlayers) zs[lp * 32 + (lane & 31)] = xget(X + kXZ + lp * 64 + (lane & 31), seq, X + x_err(nlayers), dead);
                    lds_barrier();
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (l0 + u < nlayers) acc += dot4(w[l0 + u], *reinterpret_cast<const float4*>(zs + (l0 + u) * 32 + 4 * sl));
                }
            }
            // the row's eight partial sums, pairwise (lanes 8 r .. 8 r + 7 of a row of 16 DPP lanes: xor 1, 2, then 4)
            acc += dpp_f(acc, 101);
            acc += dpp_f(acc, 102);
            acc += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(acc), 0x101F));    // xor 4 inside groups of 32
            // this workgroup's 32 activated skip values -> LDS, then its share of EVERY logit: thread q adds the 32 products
            // of head row q with them (8 float4 of head weights per thread, resident); workgroup 0 adds the eight shares
            if (sl == 0) hs[tid >> 3] = act_apply(acc, head_act);
            lds_barrier();
            float pl = 0.f;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pl += dot4(wh[jj], *reinterpret_cast<const float4*>(hs + 4 * jj));
            xput(X + x_pl(nlayers) + (wg - 1) * 256 + tid, pl, seq);
            lds_barrier();                                            // zs / hs are rewritten by the next step
        }
        return;
    }
    // ---- workgroup 0: the chain, softmax, sampling (k_decode_fast without its skip waves and head) ----
    const ChainLds S(sm);
    const float hb = chain_prologue(S, q, nlayers, tid);
    bool dead0 = false;                                   // this thread's wait for the logit shares gave up: wait for nothing any more
    GateWalk gw{nullptr, 0, nullptr};
    if (GATE) gw = gate_walk_open(q.fr);

    for (int it = 0; it < nsteps; ++it) {
        const unsigned n = (unsigned)(q.n0 + it);
        const unsigned seq = (unsigned)(it + 1);
        const int token = S.s_tok[0], tprev = S.s_tok[1];
        const double u_draw = do_sample ? q.uniforms[it] : 0.0;
        const int f_tok = FORCED && do_sample ? q.out_tokens[it] : -1;           // the entry a given step emits (draw_token)
        if (it == 0) fetch_xold(S, q.arena, nlayers, n, tid);   // later steps: fetched during the previous step's wait (below)
        open_step(S, token, tprev, tid);
        if (wv == 0) {
            chain_wave(S, P, nlayers, lane);
        } else if (wv == 1) {
            old_wave<GATE>(S, P, nlayers, lane, q, gw);
        } else if (wv == 2) {
            __syncthreads();
            // the publisher: follows the chain through the layer counter in LDS and hands every layer's z to the other CUs
            for (int l = 0; l < nlayers; ++l) {
                wait_layer(S, l + 1);
                xput(X + kXZ + l * 64 + lane, S.zall[l * 32 + (lane & 31)], seq);
            }
        } else {
            __syncthreads();
        }
        lds_barrier();                                    // the chain has written every x_cur
        for (int i = tid; i < nlayers * 32; i += kFT) {   // this step's x_cur of every layer becomes the newest ring column
            const int l = i >> 5;
            const unsigned dm = (unsigned)S.dmask[l];
            float* ring = q.arena + S.ringt[l] + (i & 31);
            const float xn = S.xcur[i];
            ring[(long long)(n & dm) * 32] = xn;
            // ... and the NEXT step's x[n + 1 - d] is fetched now, under the wait for the logits: with d = 1 it is the value just
            // stored, otherwise a column written d - 1 steps ago (the chain and wave 1 are through with xold: barrier above)
            S.xold[i] = dm == 0u ? xn : ring[(long long)((n + 1u) & dm) * 32];
        }
        // logit `tid` = bias + the eight workgroups' shares, added in workgroup order.  The eight entries are requested
        // together (one memory round trip), re-requested together until all carry this step's number
        float v;
        {
            const u64* e = X + x_pl(nlayers) + tid;
            u64 wd[kD10Skip];
            int spins = 0;
            for (;;) {
                bool ok = true;
#pragma unroll
                for (int k = 0; k < kD10Skip; ++k) wd[k] = __hip_atomic_load(e + k * 256, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int k = 0; k < kD10Skip; ++k) ok = ok && (unsigned)(wd[k] >> 32) == seq;
                if (ok || dead0) break;
                __builtin_amdgcn_s_sleep(1);
                ++spins;
                if (spins > (1 << 21) || ((spins & 0xfff) == 0 &&
                                          __hip_atomic_load(X + x_err(nlayers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    // given up (see xget): the launch is void, say so, and wait for nothing from here on
                    __hip_atomic_store(X + x_err(nlayers), (u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    dead0 = true;
                }
            }
            v = hb;
#pragma unroll
            for (int k = 0; k < kD10Skip; ++k) v += __uint_as_float((unsigned)wd[k]);
        }
        if (apply_softmax) v = softmax_row(S, v, q.sc.inv_temp, tid);
        S.lg[tid] = v;
        if (!CHOSEN && q.prob_out) q.prob_out[(long long)it * prob_stride + tid] = v;
        lds_barrier();
        if (do_sample) draw_token(S, q.sc, u_draw, token, q.out_tokens + it, tid, FORCED ? __builtin_amdgcn_readfirstlane(f_tok) : -1);
        else if (tid == 0) S.s_tok[1] = token;
        __syncthreads();                           // full barrier: orders this step's ring stores before the next step's loads
        if (CHOSEN) store_chosen(S, q.prob_out, it, tid);
        if (GATE) gate_walk_next(gw, q.fr);
    }
    if (tid == 0) q.tok_ring[0] = S.s_tok[1];
}

template <bool GATE, bool CHOSEN, bool FORCED>
__global__ __launch_bounds__(kFT, 1) void k_decode_fast3(const DecUtt q, int nlayers, int nsteps, int prob_stride,
                                                         int apply_softmax, int do_sample, int head_act) {
    decode_fast3_body<GATE, CHOSEN, FORCED>((int)blockIdx.x, q, nlayers, nsteps, prob_stride, apply_softmax, do_sample, head_act);
}

// N independent utterances in ONE launch: nine workgroups each (the single-GPU form of "replicas only", SURVEY 8(e): batch 1
// has a strict sample-to-sample dependency, so the other 247 CUs can only run OTHER utterances).  Every utterance has its own
// decoder state (rings, token ring, exchange entries, packed weights: a handle each), its own uniforms and outputs; the groups
// share nothing and never wait for each other, so an utterance's tokens are those of its own wn_decoder_run, bit for bit.
// The launch has no step count of its own: utterance u runs a.it[u].nsteps steps.  All nine workgroups of the utterance read
// that ONE word, and decode_fast3_body has one step loop per role -- the eight skip workgroups' and the chain workgroup's, whose
// publisher wave runs inside the chain's loop --, each bounded by the same argument: no workgroup of a group runs a step its
// partners do not, so no wait is left without its entry, and a group that ends early simply ends.
struct DecBatchArgs { DecUtt it[kDecMaxBatch]; };
static_assert(sizeof(DecBatchArgs) + 4 * sizeof(int) <= 4096, "kernel arguments are passed by value: 4 KB at most");
template <bool GATE, bool CHOSEN, bool FORCED>
__global__ __launch_bounds__(kFT, 1) void k_decode_fast3_batch(const DecBatchArgs a, int nlayers, int prob_stride, int head_act) {
    const int u = blockIdx.x / (kD10Skip + 1);
    decode_fast3_body<GATE, CHOSEN, FORCED>((int)blockIdx.x - u * (kD10Skip + 1), a.it[u], nlayers, a.it[u].nsteps, prob_stride, 1, 1,
                                            head_act);
}

__global__ void k_decode_zero_x(u64* X, int n) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) X[i] = 0ull;
}
// the exchange entries are cleared by a kernel, in stream order, before every launch that uses them
static void zero_x(u64* X, int nlayers, hipStream_t s) {
    const int nx = x_entries(nlayers);
    hipLaunchKernelGGL(k_decode_zero_x, dim3(cdiv(nx, 256)), dim3(256), 0, s, X, nx);
}

// the instantiation of kernel template K for a launch: gate rows | chosen trace | given tokens
#define WN_DEC_ALL(K) K<false, false, false>, K<true, false, false>, K<false, true, false>, K<true, true, false>, \
                      K<false, false, true>, K<true, false, true>, K<false, true, true>, K<true, true, true>
#define WN_DEC_PICK2(K, g, c, F) ((c) ? ((g) ? K<true, true, F> : K<false, true, F>) : ((g) ? K<true, false, F> : K<false, false, F>))
#define WN_DEC_PICK(K, g, c, f) ((f) ? WN_DEC_PICK2(K, g, c, true) : WN_DEC_PICK2(K, g, c, false))

size_t decode_fast_lds_bytes() { return ChainLds::kBytes; }
size_t decode_fast_pack_floats(int nlayers) {            // weights, then the exchange entries of the nine-workgroup form (8 bytes each)
    return (size_t)nlayers * kLayerFloats + 256 * 256 + 2 * (size_t)x_entries(nlayers);
}

int decode_fast_pack(const WnDecoderDesc* d, float* dst, hipStream_t s) {
    const int L = d->n_blocks * d->n_layers;
    for (int l = 0; l < L; ++l)
        hipLaunchKernelGGL(k_pack_fast_layer, dim3(1), dim3(128), 0, s, d->Wf[l], d->Wg[l], d->Wp[l], d->Ws[l],
                           dst + (size_t)l * kLayerFloats);
    hipLaunchKernelGGL(k_pack_fast_head, dim3(1), dim3(256), 0, s, d->head_W[0], dst + (size_t)L * kLayerFloats);
    WN_LAUNCH_CHECK();
    return WN_OK;
}

int decode_fast_launch(DecUtt q, int nlayers, int nsteps, int prob_stride, int apply_softmax, int do_sample, int head_act,
                       bool three_wgs, bool gate_rows, hipStream_t s) {
    WN_MAX_LDS_ONCE((int)decode_fast_lds_bytes(), WN_DEC_ALL(k_decode_fast), WN_DEC_ALL(k_decode_fast3));
    const bool chosen = prob_stride == kProbChosen;          // (a sampling launch: wn_decoder_step passes Q)
    const bool forced = do_sample == kSampleGiven;           // (the kernels themselves only ask whether do_sample != 0)
    if (three_wgs && nsteps > 1 && nsteps < (1 << 30) && nlayers <= kD10MaxL) {
        // nine workgroups that wait for each other: the device the stream belongs to must be able to hold them at once (asked
        // per device, per call: cheap, and a process may drive several devices).  What the count cannot see -- other work
        // holding the CUs for seconds -- ends in a given-up wait that wn_decoder_status reports (no trap, no hang).
        int dev = 0, n_cu = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n_cu >= kD10Skip + 1) {
            q.X = x_area(q.P, nlayers);
            zero_x(q.X, nlayers, s);
            const auto k3 = WN_DEC_PICK(k_decode_fast3, gate_rows, chosen, forced);
            hipLaunchKernelGGL(k3, dim3(kD10Skip + 1), dim3(kFT), decode_fast_lds_bytes(), s, q, nlayers, nsteps,
                               prob_stride, apply_softmax, do_sample, head_act);
            WN_LAUNCH_CHECK();
            return WN_OK;
        }
    }
    const auto k1 = WN_DEC_PICK(k_decode_fast, gate_rows, chosen, forced);
    hipLaunchKernelGGL(k1, dim3(1), dim3(kFT), decode_fast_lds_bytes(), s, q, nlayers, nsteps, prob_stride,
                       apply_softmax, do_sample, head_act);
    WN_LAUNCH_CHECK();
    return WN_OK;
}

int decode_fast_batch_ok(int nlayers, int n_utt, int nsteps) {
    if (n_utt < 1 || n_utt > kDecMaxBatch || nsteps < 2 || nsteps >= (1 << 30) || nlayers > kD10MaxL) return 0;
    int dev = 0, n_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return n_utt * (kD10Skip + 1) <= n_cu ? 1 : 0;             // every workgroup resident (one per CU by LDS footprint)
}

int decode_fast_launch_batch(int n_utt, const DecUtt* utt, int nlayers, int nsteps, int prob_stride, int do_sample, int head_act,
                             bool same_weights, bool gate_rows, hipStream_t s) {
    if (!decode_fast_batch_ok(nlayers, n_utt, nsteps)) {
        wn::set_error("decode batch: %d utterances x 9 workgroups do not fit the device (or fewer than 2 steps)", n_utt);
        return WN_ESHAPE;
    }
    for (int u = 0; u < n_utt; ++u)        // every group of nine runs 2 steps at least, n at most (wn_decoder_run_batch has checked it)
        if (utt[u].nsteps < 2 || utt[u].nsteps > nsteps) {
            wn::set_error("decode batch: utterance %d's step count %d outside [2, %d]", u, utt[u].nsteps, nsteps);
            return WN_EARG;
        }
    WN_MAX_LDS_ONCE((int)decode_fast_lds_bytes(), WN_DEC_ALL(k_decode_fast3_batch));
    const bool chosen = prob_stride == kProbChosen;
    DecBatchArgs a{};
    for (int u = 0; u < n_utt; ++u) {
        DecUtt& q = a.it[u];
        q = utt[u];
        q.X = x_area(q.P, nlayers);        // the utterance's own exchange entries, whoever's weights it reads
        zero_x(q.X, nlayers, s);
        // same_weights (the caller's word that every handle was created from the same weights): every utterance reads utterance
        // 0's packed weights, embedding table and head bias -- the 28 chain workgroups then stream ONE 0.96 MB copy per step
        // through the XCDs' L2s instead of 28; the state (rings, token ring, exchange entries) stays per utterance.  An
        // utterance 0 that ends before the others leaves its packed weights in place -- a launch frees and rewrites nothing of
        // a handle's weights -- and the others keep reading them.  Gate rows are not part of P: an utterance's static gate
        // biases (its arena) and frame table (DecUtt.fr) stay its own, so utterances of one model may differ in class and table.
        if (same_weights) { q.P = utt[0].P; q.hbias = utt[0].hbias; q.E = utt[0].E; }
    }
    const auto kb = WN_DEC_PICK(k_decode_fast3_batch, gate_rows, chosen, do_sample == kSampleGiven);
    hipLaunchKernelGGL(kb, dim3(n_utt * (kD10Skip + 1)), dim3(kFT), decode_fast_lds_bytes(), s, a, nlayers,
                       prob_stride, head_act);
    WN_LAUNCH_CHECK();
    return WN_OK;
}

// 0 = the last nine-workgroup run's exchange completed; 1 = a wait gave up (its tokens are void).  Synchronises the stream.
int decode_fast_status(const float* P, int nlayers, hipStream_t s, int* gave_up) {
    u64 w = 0;
    WN_HIP(hipMemcpyAsync(&w, x_area(P, nlayers) + x_err(nlayers), sizeof(w), hipMemcpyDeviceToHost, s));
    WN_HIP(hipStreamSynchronize(s));
    *gave_up = w != 0 ? 1 : 0;
    return WN_OK;
}

}  // namespace wn
