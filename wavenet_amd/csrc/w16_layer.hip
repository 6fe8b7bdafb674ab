// Fused residual-layer kernels of the bf16-storage path (BASELINE config 5; ResidualConvLayer.__call__, wavenet.py:358-368,
// and Chainer's backward through it), Cr = Cd = 128, filter width 2.
//
//   k16_fwd       x (bf16) -> out = Wp z + x (bf16), z = tanh(Wf * x) sigmoid(Wg * x) (bf16).  One kernel per layer.
//   k16_gate_bwd  recomputes tanh / sigmoid from x (nothing but z is saved by the forward), dz = Wp^T dout + dz_skip,
//                 [da | dg] = dz (g (1 - f^2) | f g (1 - g)) (bf16).
//   k16_dx        dx[t] = dout[t] + [Wf1;Wg1]^T dab[t] + [Wf0;Wg0]^T dab[t + d] (bf16) -- the gradient the layer below
//                 receives -- and, with that layer's z, its projection weight gradient dWp += dx z^T (fp32 partials).
// All three are weight-stationary: every wave keeps its slice of the layer's weights in registers as MFMA A operands for
// the whole launch and the workgroup streams 32-column time tiles (256-byte rows) through LDS by LDS-DMA.
//
// Shape of the first two (measured on config 5, ablations in DESIGN.md): per 64 columns and SIMD the layer needs ~2,600
// cycles of matrix pipe and ~2,800 cycles of VALU issue (tanh / sigmoid: four transcendentals per gate element).  One
// 8-wave workgroup per CU with barriers between the phases kept all waves in lockstep -- everybody on the matrix pipe,
// then everybody on the VALU -- and the phases ADDED (28 us of compute per layer against 19 us of memory time).  Now a
// workgroup is 4 waves (one per SIMD, 32 gate channels each: the filter rows and the gate rows of a channel are the same
// accumulator register of two MFMA tiles) and TWO workgroups share a CU: they are not synchronised with each other, so one
// workgroup's gate arithmetic runs under the other's MFMAs and stores.
#include <stdlib.h>
#include <type_traits>

#include "w16_gemm.hpp"
#include "wn_kernels.hpp"

namespace w16 {

using wn::fast_sigmoid;
using wn::fast_tanh;

// z = tanh(a) sigmoid(g) with ONE reciprocal: (1 - e^{-2a}) / ((1 + e^{-2a}) (1 + e^{-g})) -- two exponentials, one reciprocal and
// eight plain instructions instead of two of each and fourteen (fast_tanh's small-|a| series included): the forward is bound
// by VALU issue, and the result is rounded to bf16 (8 bits) right away.  a is clamped at -30 (tanh is -1 to
// the last fp32 bit long before; e^{60} stays finite so that inf / inf cannot arise); a huge e^{-g} makes the
// denominator inf and z the 0 it should be.
__device__ __forceinline__ float gate_z(float a, float g) {
    const float e2 = __builtin_amdgcn_exp2f(fmaxf(a, -30.f) * -2.8853900817779268f);
    const float eg = __builtin_amdgcn_exp2f(g * -1.4426950408889634f);
    return (1.f - e2) * __builtin_amdgcn_rcpf((1.f + e2) * (1.f + eg));
}

// tanh(a) and sigmoid(g) with ONE reciprocal (the backward needs both): r = 1 / ((1 + e^{-2a}) (1 + e^{-g})),
// sigmoid = (1 + e^{-2a}) r, tanh = (1 - e^{-2a}) (1 + e^{-g}) r.  g is clamped at -80 so that the product stays finite
// (sigmoid(-80) = 1.8e-35: a gradient factor of 0 to bf16 either way); a as in gate_z.
__device__ __forceinline__ void gate_fg(float a, float g, float& f, float& s) {
    const float e2 = __builtin_amdgcn_exp2f(fmaxf(a, -30.f) * -2.8853900817779268f);
    const float eg = __builtin_amdgcn_exp2f(fmaxf(g, -80.f) * -1.4426950408889634f);
    const float p2 = 1.f + e2, pg = 1.f + eg;
    const float r = __builtin_amdgcn_rcpf(p2 * pg);
    s = p2 * r;
    f = (1.f - e2) * (pg * r);
}

static constexpr int kLT = 32;                          // time columns per tile
static constexpr int kLTileB = kLT * 256;               // 8 KB

// ---------------------------------------------------------------------------------------------
// gate-bias rows (conditioning; LayerRows in w16_gemm.hpp, the modes are wn::kCond*).  A lane owns one time column of a tile,
// so it reads ITS column's row values: fp32, 16 bytes at a time, straight into registers (LDS is full).  The reads are
// inline asm like every other request of these loops -- a load hipcc knows of gets an s_waitcnt vmcnt(0) at its first use,
// which drains the LDS-DMA prefetch of the next tile -- and they are issued AHEAD of issue(next): the counted waits of the
// tile loops then say what they said (the reads are gone before the tile's stores are issued), and the reads themselves are
// waited for with "as many requests as issue(next) made may stay in flight".
// ---------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
using wn::kCondNone; using wn::kCondClip; using wn::kCondFrame; using wn::kCondLinear;

template <int OFF>
__device__ __forceinline__ f32x4 row_ld16(const float* p) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(v) : "v"(p), "n"(OFF) : "memory");
    return v;
}
// behind a counted wait that covers them: the values of row_ld16 may be used from here on (the tie keeps every use behind
// the wait, which is volatile asm like it)
template <int K>
__device__ __forceinline__ void rows_tie(f32x4 (&r)[K]) {
#pragma unroll
    for (int i = 0; i < K; ++i) asm volatile("" : "+v"(r[i]));
}
template <int N, int K>
__device__ __forceinline__ void rows_wait(f32x4 (&r)[K]) {
    wait_vm<N>();
    rows_tie(r);
}
// frame and position inside it of tile column jj (< 32) of the tile at t0, phase ph: (t0 + jj + ph) / hop and % hop, with
// the division on the scalar unit alone when a frame is at least a tile long
__device__ __forceinline__ void tile_frame(int hop, int ph, int t0, int jj, int& fi, int& rem) {
    const int p0 = t0 + ph, f0 = p0 / hop, r0 = p0 - f0 * hop;
    if (hop >= kLT) {
        const bool over = r0 + jj >= hop;
        fi = f0 + (over ? 1 : 0);
        rem = r0 + jj - (over ? hop : 0);
    } else {
        const int q = (r0 + jj) / hop;
        fi = f0 + q;
        rem = r0 + jj - q * hop;
    }
}
// THE phase of clip b by wn::frame_phase's rule (the fence included), for a tile loop: b is uniform there, and the table entry
// is read by an explicit scalar load -- left to hipcc it becomes a vector load with an s_waitcnt vmcnt(0) behind it, inside
// the loop (tests/test_isa_cpu.py)
__device__ __forceinline__ int tile_phase(const wn::BiasFrames& fr, int b) {
    if (!fr.tab) return fr.phase;
    const int* p = fr.tab + b;
    int v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return wn::bias_phase_fence(v, fr.hop);
}
// what a lane needs to read its column's rows of one tile: the address of its first float of the filter row and of the gate
// row (frame J(t) of clip b; lane_off = the lane's first channel), the next frame's rows `next` floats on, and alpha
struct RowAt { const float* pf; const float* pg; float alpha; };
template <int MODE>
__device__ __forceinline__ RowAt row_at(const LayerRows& R, int b, int t0, int jj, int lane_off) {
    RowAt a;
    long long o = (long long)b * R.clip_stride + lane_off;
    a.alpha = 0.f;
    if constexpr (MODE >= kCondFrame) {
        const int ph = tile_phase(R.fr, b);
        int fi, rem;
        tile_frame(R.fr.hop, ph, t0, jj, fi, rem);
        o += (long long)fi * R.fr.stride;
        if constexpr (MODE == kCondLinear) a.alpha = wn::bias_alpha(rem, R.fr.hop);            // wn::bias_frame_alpha's value
    }
    a.pf = R.bf + o;
    a.pg = R.bg + o;
    return a;
}

// ---------------------------------------------------------------------------------------------
// forward.  256 threads; LDS: (xold, xcur) x 2 buffers + z tile + out tile = 48 KB, + the projection's operand image
// (32 KB, read at each use: keeping it in registers left none to prefetch the column operands with, and every
// ds_read_b128 -> s_waitcnt -> MFMA pair ran back to back: 16 exposed LDS latencies per tile)
// ---------------------------------------------------------------------------------------------
static constexpr int kFwdLds = 6 * kLTileB + kProjA * 2;

// MODE (wn::kCond*): the gate-bias rows.  kCondNone is the kernel without them; in the others the lane of column t0 + j starts
// its accumulators from its column's 16 filter and 16 gate values (channels 32 w + 8 q + 4 h + e = accumulator register
// 4 q + e; interpolated in fp32 first with kCondLinear), so the matrix pipe adds the convolution to them: no add, no register
// beside the accumulators while the convolution runs.  The reads of a tile are requested one tile ahead (rows_issue).
template <int MODE>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void k16_fwd(const bf16* __restrict__ x, const bf16* __restrict__ convA,
                                                   const bf16* __restrict__ projA, bf16* __restrict__ out,
                                                   bf16* __restrict__ z, int B, int T, int d, int Z, int tiles_per_b,
                                                   int ntiles, const LayerRows R) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    auto xold = [&](int buf) { return lds + buf * kLTileB; };
    auto xcur = [&](int buf) { return lds + (2 + buf) * kLTileB; };
    char* zt = lds + 4 * kLTileB;
    char* ot = lds + 5 * kLTileB;
    char* wpl = lds + 6 * kLTileB;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & 31, h = lane >> 5;
    int first, stride, last;
    tile_range(ntiles, first, stride, last);
    if (first >= last) return;

    // A operands: filter rows and gate rows of channels 32 w .. 32 w + 31 (16 k-steps: 0..7 tap 0 = x[t-d], 8..15 tap 1
    // = x[t]); this wave's slice of the projection image goes to LDS
    bf16x8 fA[16], gA[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        fA[s] = *reinterpret_cast<const bf16x8*>(convA + (((w * 2 + 0) * 16 + s) * 64 + lane) * 8);
        gA[s] = *reinterpret_cast<const bf16x8*>(convA + (((w * 2 + 1) * 16 + s) * 64 + lane) * 8);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) W16_DMA16(projA + ((w * 8 + s) * 64 + lane) * 8, wpl + (w * 8 + s) * 1024);
    // the operand loads are waited for HERE: left pending, the compiler would place its s_waitcnt vmcnt(0) at their first
    // use inside the loop, where it would also drain the LDS-DMA prefetch of every iteration
#pragma unroll
    for (int s = 0; s < 16; ++s) { asm volatile("" ::"v"(fA[s])); asm volatile("" ::"v"(gA[s])); }

    // per-lane LDS offsets, the same for every tile
    int foff[8], qoff[4];
#pragma unroll
    for (int s = 0; s < 8; ++s) foff[s] = toff(j, 2 * s + h);       // operand of k-step s: row j, chunk 2 s + h
#pragma unroll
    for (int q = 0; q < 4; ++q) qoff[q] = toff(j, 4 * w + q) + 8 * h;   // accumulator registers 4 q .. 4 q + 3 of this wave
    const int prow = lane >> 4;                                     // row piece / chunk of the whole-row copies
    int pcol[2];
    unsigned loff[2];                                               // byte offset of this lane's 16 bytes inside a tile of rows
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
        pcol[pp] = ((lane & 15) ^ key(4 * (2 * w + pp) + prow)) * 8;
        loff[pp] = (unsigned)(((4 * (2 * w + pp) + prow) * 128 + pcol[pp]) * 2);
    }
    const unsigned lds0 = lds_addr_of(lds);

    auto issue = [&](int tile, int buf) {
        const int b = tile / tiles_per_b;
        const int t0 = (tile - b * tiles_per_b) * kLT;
        const bf16* xb = x + (long long)b * T * 128;
        if (t0 + kLT <= T && t0 >= d) {                  // interior tile: no clamping; uniform base + fixed lane offsets
            const bf16* bc = xb + (long long)t0 * 128;
            const bf16* bo = bc - (long long)d * 128;
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {
                const int p = 2 * w + pp;
                dma16_s(bc, loff[pp], lds0 + (2 + buf) * kLTileB + p * 1024);
                dma16_s(bo, loff[pp], lds0 + buf * kLTileB + p * 1024);
            }
            return;
        }
        // (inline asm as the interior tiles' requests: one builtin LDS-DMA anywhere in the loop and every LDS wait hipcc emits
        // in it is lgkmcnt(0) -- fragments in flight for the next k-step are waited for with the ones being consumed)
        dma_pieces<true>(xcur(buf), lane, 2 * w, 1, 2, [&](int r) {
            const int t = t0 + r < T ? t0 + r : T - 1;
            return xb + (long long)t * 128;
        });
        dma_pieces<true>(xold(buf), lane, 2 * w, 1, 2, [&](int r) {
            int t = t0 + r < T ? t0 + r : T - 1;
            t = t - d >= 0 ? t - d : 0;
            return xb + (long long)t * 128;
        });
    };

    // the rows of a tile's columns: filter and gate row of each column's frame (ya, yb) and, with interpolation, of the next
    // (yc, yd).  A column beyond the clip reads the last one's -- its result is never stored.
    f32x4 ya[4], yb[4], yc[4], yd[4];
    float alpha = 0.f;
    const float* pg_next = nullptr;                    // (linear) the gate row of the tile whose filter pair is in flight
    auto rows_issue = [&](int tile) {                  // linear: the filter pair only, rows_issue_gate asks for the rest
        const int b = tile / tiles_per_b;
        const int t0 = (tile - b * tiles_per_b) * kLT;
        const RowAt ra = row_at<MODE>(R, b, t0, t0 + j < T ? j : T - 1 - t0, 32 * w + 4 * h);
        alpha = ra.alpha;
        ya[0] = row_ld16<0>(ra.pf); ya[1] = row_ld16<32>(ra.pf); ya[2] = row_ld16<64>(ra.pf); ya[3] = row_ld16<96>(ra.pf);
        if constexpr (MODE == kCondLinear) {
            const float* pf1 = ra.pf + R.fr.stride;
            yc[0] = row_ld16<0>(pf1); yc[1] = row_ld16<32>(pf1); yc[2] = row_ld16<64>(pf1); yc[3] = row_ld16<96>(pf1);
            pg_next = ra.pg;
        } else {
            yb[0] = row_ld16<0>(ra.pg); yb[1] = row_ld16<32>(ra.pg); yb[2] = row_ld16<64>(ra.pg); yb[3] = row_ld16<96>(ra.pg);
        }
    };
    // (linear) two rows per gate are 64 registers, which do not fit beside the weights.  The filter pair travels like a frame's
    // rows (requested behind the gate, 32 registers through the projection); BEHIND the tile's stores it is waited for and
    // folded into 16 values and the gate pair is requested: 48 registers cross the loop's head, where there is room (the
    // accumulators are not live yet) -- and the wait there is then for everything, the previous tile's stores included.
    auto rows_issue_gate = [&]() {
        rows_wait<0>(ya); rows_wait<0>(yc);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) ya[q][e] = wn::bias_lerp(ya[q][e], yc[q][e], alpha);
        const float* pg1 = pg_next + R.fr.stride;
        yb[0] = row_ld16<0>(pg_next); yb[1] = row_ld16<32>(pg_next); yb[2] = row_ld16<64>(pg_next); yb[3] = row_ld16<96>(pg_next);
        yd[0] = row_ld16<0>(pg1); yd[1] = row_ld16<32>(pg1); yd[2] = row_ld16<64>(pg1); yd[3] = row_ld16<96>(pg1);
    };

    issue(first, 0);
    if constexpr (MODE != kCondNone) rows_issue(first);
    if constexpr (MODE == kCondLinear) rows_issue_gate();
    bool full_prev = false;                            // the previous tile's 4 stores were issued unconditionally
    int it = 0;
    for (int tile = first; tile < last; tile += stride, ++it) {
        const int buf = it & 1;
        const int b = tile / tiles_per_b;
        const int t0 = (tile - b * tiles_per_b) * kLT;
        // this tile's 4 DMA pieces are older than the previous tile's 4 stores: those stay in flight
        // (and so are its row reads, requested between the previous tile's gate and its stores: this wait is theirs too)
        if (full_prev && MODE != kCondLinear) wait_vm<4>(); else wait_vm<0>();
        barrier();
        if (tile + stride < last) issue(tile + stride, buf ^ 1);
        if (t0 < d) {
            // rows whose tap-0 sample lies before the clip start read as 0 (wavenet.py:298-301 pads with zeros)
            for (int r = w; r < kLT; r += 4)
                if (t0 + r < d) *reinterpret_cast<unsigned*>(xold(buf) + r * 256 + lane * 4) = 0u;
            barrier();
        }
        // ---- both dilated convolutions for this wave's 32 channels; column operands fetched four k-steps ahead ----
        f32x16 af, ag;
        if constexpr (MODE == kCondNone) {
#pragma unroll
            for (int r = 0; r < 16; ++r) { af[r] = 0.f; ag[r] = 0.f; }
        } else {                                       // the accumulators start from the column's row values
            rows_tie(ya); rows_tie(yb);
            if constexpr (MODE == kCondLinear) {
                rows_tie(yd);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) yb[q][e] = wn::bias_lerp(yb[q][e], yd[q][e], alpha);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) { af[4 * q + e] = ya[q][e]; ag[4 * q + e] = yb[q][e]; }
        }
        {
            const char* t0p = xold(buf);
            const char* t1p = xcur(buf);
            bf16x8 bq[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) bq[s] = *reinterpret_cast<const bf16x8*>(t0p + foff[s]);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const bf16x8 bv = bq[s & 3];
                if (s + 4 < 16) bq[s & 3] = *reinterpret_cast<const bf16x8*>((s + 4 < 8 ? t0p : t1p) + foff[(s + 4) & 7]);
                af = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fA[s], bv, af, 0, 0, 0);
                ag = __builtin_amdgcn_mfma_f32_32x32x16_bf16(gA[s], bv, ag, 0, 0, 0);
            }
        }
        // ---- gate ----
        if (t0 >= Z) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float zz[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zz[e] = gate_z(af[4 * q + e], ag[4 * q + e]);
                *reinterpret_cast<bf16x4*>(zt + qoff[q]) = pack4(zz[0], zz[1], zz[2], zz[3]);
            }
        } else {                                       // the reference's zero prefix: a = g = 0 there, so z = 0
            const bool live = t0 + j >= Z;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float zz[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    zz[e] = live ? gate_z(af[4 * q + e], ag[4 * q + e]) : 0.f;
                *reinterpret_cast<bf16x4*>(zt + qoff[q]) = pack4(zz[0], zz[1], zz[2], zz[3]);
            }
        }
        if constexpr (MODE != kCondNone) {
            // the next tile's rows: the accumulators' registers are free from here on; the requests are older than this tile's
            // stores, so the wait at the loop's head covers them
            if (tile + stride < last) rows_issue(tile + stride);
        }
        barrier();
        // ---- residual projection: out rows 32 w .. of all 32 columns, + x ----
        {
            f32x16 ao;
#pragma unroll
            for (int r = 0; r < 16; ++r) ao[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 8; ++s)
                ao = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    *reinterpret_cast<const bf16x8*>(wpl + ((w * 8 + s) * 64 + lane) * 16),
                    *reinterpret_cast<const bf16x8*>(zt + foff[s]), ao, 0, 0, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bf16x4 xv = *reinterpret_cast<const bf16x4*>(xcur(buf) + qoff[q]);
                *reinterpret_cast<bf16x4*>(ot + qoff[q]) = pack4(ao[4 * q] + (float)xv[0], ao[4 * q + 1] + (float)xv[1],
                                                                 ao[4 * q + 2] + (float)xv[2], ao[4 * q + 3] + (float)xv[3]);
            }
        }
        barrier();
        // ---- whole 256-byte rows leave: 4 rows per wave instruction, two pieces of each tile per wave ----
        const bool full = t0 + kLT <= T;
        bf16* zb = z + ((long long)b * T + t0) * 128;
        bf16* ob = out + ((long long)b * T + t0) * 128;
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int p = 2 * w + pp;
            const int r = 4 * p + prow;
            const u32x4 vz = *reinterpret_cast<const u32x4*>(zt + p * 1024 + lane * 16);
            const u32x4 vo = *reinterpret_cast<const u32x4*>(ot + p * 1024 + lane * 16);
            if (full || t0 + r < T) {
                st16_wt_s(zb, loff[pp], vz);
                st16_wt_s(ob, loff[pp], vo);
            }
        }
        if constexpr (MODE == kCondLinear) {
            if (tile + stride < last) rows_issue_gate();
        }
        full_prev = full;
    }
}

// ---------------------------------------------------------------------------------------------
// gate backward.  512 threads, one workgroup per CU: wave w owns gate channels 16 w .. 16 w + 15 -- the filter rows and the
// gate rows of a channel sit in the SAME 32-row MFMA tile (rows r and r + 16 = accumulator registers r and r + 8 of one
// lane), dz comes from a tile whose rows 16..31 are zero.  LDS: (xold, xcur, dout, dzs) x 2 buffers + da, dg tiles = 80 KB.
// (A 4-wave / two-workgroup form like the forward's needs 128 + 32 operand registers per wave and spilled: 65 us against
// 47 us per layer.)
// ---------------------------------------------------------------------------------------------
static constexpr int kGateLds = 10 * kLTileB;

// Live ranges (all multiples of 32; the host computes them, w16_api.hip).  The loss reaches the stack through skip[t_off:]
// only, so layer l receives gradient at columns t >= t_off - (reach of the layers above) and nowhere else:
//   gate phase: columns below t_live carry no gradient.  Tiles wholly below t_zero (<= t_live, a multiple of 64: the deferred
//               weight-gradient launch reads [da | dg] in 64-row chunks starting there) are NOT TOUCHED -- nothing loaded,
//               nothing stored; the dead tile between t_zero and t_live, if any, stores zeros.
//   dx phase:   dx is exactly zero below t_live (= the gate bound of the layer below); such tiles are not touched unless
//               zero_dead (layer 0: the embedding backward reads every row).  [da | dg](t) and dout(t) are zero below t_gate
//               (this layer's gate bound: rows nobody wrote) -- they are not read there, their LDS tiles are zero-filled.
struct GateP {
    const bf16* x; const bf16* convA; const bf16* dzA; const bf16* dout; const bf16* dzs; int dz_t0; bf16* dadg;
    int B, T, d, Z, tiles_per_b, ntiles, t_live, t_zero;
    LayerRows R;                                         // the gate-bias rows the forward added (MODE of gate_phase)
};
struct DxP {
    const bf16* dadg; const bf16* dxA; const bf16* dout; const bf16* zprev; bf16* dx; float* dwp_part;
    int B, T, d, tiles_per_b, ntiles, t_live, t_gate, zero_dead;
};

// what every request of a wave needs: its piece of a 32-row tile is rows 4 w .. 4 w + 3, the lane's 16 bytes at a fixed offset
// from the tile's first row (off128: 256-byte rows, off256: the same piece of 512-byte [da | dg] rows)
struct WaveC { int lane, w; unsigned off128, off256, lds0; };
__device__ __forceinline__ WaveC wave_consts(const char* lds) {
    WaveC c;
    c.lane = threadIdx.x & 63;
    c.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = 4 * c.w + (c.lane >> 4);
    c.off128 = (unsigned)(r * 256 + (((c.lane & 15) ^ key(r)) << 4));
    c.off256 = c.off128 + (unsigned)(r * 256);
    c.lds0 = lds_addr_of(lds);
    return c;
}

// LDS maps, in 8 KB tiles: gate backward 10, dx 15
struct GateMap {
    static __device__ __forceinline__ int xold(int b) { return b; }
    static __device__ __forceinline__ int xcur(int b) { return 2 + b; }
    static __device__ __forceinline__ int dot(int b) { return 4 + b; }
    static __device__ __forceinline__ int dzt(int b) { return 6 + b; }
    static constexpr int dat = 8, dgt = 9;
};
struct DxMap {
    static __device__ __forceinline__ int at(int b, int which) { return 6 * b + which; }   // da dg da' dg' dout z
    static constexpr int xch = 12, dxt = 14;
};

// the requests of one gate-backward tile (this wave's piece of x[t], x[t - d], dout, dz_skip)
template <bool HAS_DO, bool HAS_DZ>
__device__ __forceinline__ void gate_issue(char* lds, const GateP& P, const WaveC& c, int tile, int buf) {
    using M = GateMap;
    const int T = P.T, d = P.d, dz_t0 = P.dz_t0, Tw = P.T - P.dz_t0, lane = c.lane, w = c.w;
    const int b = tile / P.tiles_per_b;
    const int t0 = (tile - b * P.tiles_per_b) * kLT;
    if (t0 + kLT <= P.t_live) return;                    // a dead tile
    if (t0 + kLT <= T && t0 >= d && (!HAS_DZ || t0 >= dz_t0)) {
        // interior tile (nothing to clamp): uniform base + the fixed lane offset, no 64-bit address arithmetic per
        // request -- the four requests cost a wave ~520 cycles of a ~5,900-cycle tile in the clamped form below
        const bf16* bc = P.x + ((long long)b * T + t0) * 128;
        dma16_s(bc, c.off128, c.lds0 + M::xcur(buf) * kLTileB + w * 1024);
        dma16_s(bc - (long long)d * 128, c.off128, c.lds0 + M::xold(buf) * kLTileB + w * 1024);
        if (HAS_DO) dma16_s(P.dout + ((long long)b * T + t0) * 128, c.off128, c.lds0 + M::dot(buf) * kLTileB + w * 1024);
        if (HAS_DZ) dma16_s(P.dzs + ((long long)b * Tw + (t0 - dz_t0)) * 128, c.off128, c.lds0 + M::dzt(buf) * kLTileB + w * 1024);
        return;
    }
    const bf16* xb = P.x + (long long)b * T * 128;
    dma_pieces<true>(lds + M::xcur(buf) * kLTileB, lane, w, 1, 1, [&](int r) {
        const int t = t0 + r < T ? t0 + r : T - 1;
        return xb + (long long)t * 128;
    });
    dma_pieces<true>(lds + M::xold(buf) * kLTileB, lane, w, 1, 1, [&](int r) {
        int t = t0 + r < T ? t0 + r : T - 1;
        t = t - d >= 0 ? t - d : 0;
        return xb + (long long)t * 128;
    });
    if (HAS_DO) {
        const bf16* db = P.dout + (long long)b * T * 128;
        dma_pieces<true>(lds + M::dot(buf) * kLTileB, lane, w, 1, 1, [&](int r) {
            const int t = t0 + r < T ? t0 + r : T - 1;
            return db + (long long)t * 128;
        });
    }
    if (HAS_DZ) {
        const bf16* zb = P.dzs + (long long)b * Tw * 128;       // dz_skip exists for the loss window only
        dma_pieces<true>(lds + M::dzt(buf) * kLTileB, lane, w, 1, 1, [&](int r) {
            int t = t0 + r < T ? t0 + r : T - 1;
            t = t - dz_t0 >= 0 ? t - dz_t0 : 0;
            return zb + (long long)t * 128;
        });
    }
}

// the requests of one dx tile (this wave's piece of [da | dg](t), [da | dg](t + d), dout, z of the layer below)
template <bool HAS_DO, bool HAS_Z>
__device__ __forceinline__ void dx_issue(char* lds, const DxP& P, const WaveC& c, int tile, int buf) {
    using M = DxMap;
    const int T = P.T, d = P.d, lane = c.lane, w = c.w;
    const int b = tile / P.tiles_per_b;
    const int t0 = (tile - b * P.tiles_per_b) * kLT;
    if (t0 + kLT <= P.t_live) return;                    // a dead tile
    const bool tlive = t0 + kLT > P.t_gate;            // the tile's own rows of [da | dg] and dout exist (else: zeros, dx_phase fills them in)
    if (t0 + kLT + d <= T) {                           // interior tile: uniform bases + fixed lane offsets (as in gate_issue)
        const bf16* a0 = P.dadg + ((long long)b * T + t0) * 256;
        const bf16* a1 = a0 + (long long)d * 256;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (tlive) dma16_s(a0 + 128 * half, c.off256, c.lds0 + M::at(buf, half) * kLTileB + w * 1024);
            dma16_s(a1 + 128 * half, c.off256, c.lds0 + M::at(buf, 2 + half) * kLTileB + w * 1024);
        }
        if (HAS_DO && tlive) dma16_s(P.dout + ((long long)b * T + t0) * 128, c.off128, c.lds0 + M::at(buf, 4) * kLTileB + w * 1024);
        if (HAS_Z) dma16_s(P.zprev + ((long long)b * T + t0) * 128, c.off128, c.lds0 + M::at(buf, 5) * kLTileB + w * 1024);
        return;
    }
    const bf16* ab = P.dadg + (long long)b * T * 256;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (tlive) dma_pieces<true>(lds + M::at(buf, half) * kLTileB, lane, w, 1, 1, [&](int r) {
            const int t = t0 + r < T ? t0 + r : T - 1;
            return ab + (long long)t * 256 + 128 * half;
        });
        dma_pieces<true>(lds + M::at(buf, 2 + half) * kLTileB, lane, w, 1, 1, [&](int r) {
            int t = t0 + r + d;
            t = t < T ? t : T - 1;
            return ab + (long long)t * 256 + 128 * half;
        });
    }
    if (HAS_DO && tlive) {
        const bf16* db = P.dout + (long long)b * T * 128;
        dma_pieces<true>(lds + M::at(buf, 4) * kLTileB, lane, w, 1, 1, [&](int r) {
            const int t = t0 + r < T ? t0 + r : T - 1;
            return db + (long long)t * 128;
        });
    }
    if (HAS_Z) {
        const bf16* zb = P.zprev + (long long)b * T * 128;
        dma_pieces<true>(lds + M::at(buf, 5) * kLTileB, lane, w, 1, 1, [&](int r) {
            const int t = t0 + r < T ? t0 + r : T - 1;
            return zb + (long long)t * 128;
        });
    }
}

// One layer's gate backward over this workgroup's tiles.  MODE (wn::kCond*) as in k16_fwd: the recomputed pre-activations get
// the rows the forward added -- a lane's 8 filter and 8 gate values (channels 16 w + 8 q + 4 h + e = accumulator registers
// 4 q + e and 8 + 4 q + e), read ahead of issue(next) and waited for where the elementwise phase starts.
template <bool HAS_DO, bool HAS_DZ, int MODE>
__device__ __forceinline__ void gate_phase(char* lds, const GateP& P) {
    using M = GateMap;
    const bf16* __restrict__ convA = P.convA; const bf16* __restrict__ dzA = P.dzA; bf16* __restrict__ dadg = P.dadg;
    const int dz_t0 = P.dz_t0, T = P.T, d = P.d, Z = P.Z, tiles_per_b = P.tiles_per_b, ntiles = P.ntiles, t_live = P.t_live;
    // t_live (a multiple of 32): no gradient reaches this layer's columns below it (they are further from the loss window than
    // the layers above can see).  Such tiles load and compute nothing: they store the zeros their readers expect.
    auto xold = [&](int buf) { return lds + M::xold(buf) * kLTileB; };
    auto xcur = [&](int buf) { return lds + M::xcur(buf) * kLTileB; };
    auto dot = [&](int buf) { return lds + M::dot(buf) * kLTileB; };
    auto dzt = [&](int buf) { return lds + M::dzt(buf) * kLTileB; };
    char* dat = lds + M::dat * kLTileB;
    char* dgt = lds + M::dgt * kLTileB;
    const WaveC c = wave_consts(lds);
    const int lane = c.lane, w = c.w;
    const int j = lane & 31, h = lane >> 5;
    int first, stride, last;
    tile_range(ntiles, first, stride, last);
    const int n = first < last ? (last - first + stride - 1) / stride : 0;     // this workgroup's tiles
    auto issue = [&](int tile, int buf) { gate_issue<HAS_DO, HAS_DZ>(lds, P, c, tile, buf); };
    constexpr int kStores = 2;                          // da and dg pieces per wave and tile
    constexpr int kReqs = 2 + (HAS_DO ? 1 : 0) + (HAS_DZ ? 1 : 0);   // requests per wave of one gate_issue (none for a dead tile)

    // the first tile's operands are requested BEFORE this wave's weights (register-resident A operands) so that the two
    // round trips overlap; the weights are waited for here (left pending, the compiler's s_waitcnt vmcnt(0) would sit at their
    // first use inside the loop and drain the LDS-DMA prefetch of every iteration)
    if (n > 0) issue(first, 0);
    bf16x8 cA[16], zA[8];
#pragma unroll
    for (int s = 0; s < 16; ++s) cA[s] = *reinterpret_cast<const bf16x8*>(convA + ((w * 16 + s) * 64 + lane) * 8);
    if (HAS_DO) {
#pragma unroll
        for (int s = 0; s < 8; ++s) zA[s] = *reinterpret_cast<const bf16x8*>(dzA + ((w * 8 + s) * 64 + lane) * 8);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) asm volatile("" ::"v"(cA[s]));
    if (HAS_DO) {
#pragma unroll
        for (int s = 0; s < 8; ++s) asm volatile("" ::"v"(zA[s]));
    }
    bool full_prev = false;
    int it = 0;
    for (int tile = first; tile < last; tile += stride, ++it) {
        const int buf = it & 1;
        const int b = tile / tiles_per_b;
        const int t0 = (tile - b * tiles_per_b) * kLT;
        if (full_prev) wait_vm<kStores>(); else wait_vm<0>();
        barrier();
        f32x4 ya[2], yb[2], yc[2], yd[2];                  // filter, gate rows of the column's frame; linear: and of the next
        float alpha = 0.f;
        bool next_reqs = false;                            // issue(next) makes requests (there is a next tile and it is live)
        if constexpr (MODE != kCondNone) {
            // (a dead tile reads its rows too: no branch between a request and the tie behind its wait -- a value that meets
            // another at a join is COPIED there, and a copy ahead of the wait reads a register the load has not written yet)
            {
                const RowAt ra = row_at<MODE>(P.R, b, t0, t0 + j < T ? j : T - 1 - t0, 16 * w + 4 * h);
                alpha = ra.alpha;
                ya[0] = row_ld16<0>(ra.pf); ya[1] = row_ld16<32>(ra.pf);
                yb[0] = row_ld16<0>(ra.pg); yb[1] = row_ld16<32>(ra.pg);
                if constexpr (MODE == kCondLinear) {
                    const float* pf1 = ra.pf + P.R.fr.stride;
                    const float* pg1 = ra.pg + P.R.fr.stride;
                    yc[0] = row_ld16<0>(pf1); yc[1] = row_ld16<32>(pf1);
                    yd[0] = row_ld16<0>(pg1); yd[1] = row_ld16<32>(pg1);
                }
            }
            if (tile + stride < last) {
                const int nt = tile + stride;
                next_reqs = (nt - (nt / tiles_per_b) * tiles_per_b) * kLT + kLT > t_live;
            }
        }
        if (tile + stride < last) issue(tile + stride, buf ^ 1);
        if (t0 + kLT <= t_live) {                          // dead tile (workgroup-uniform)
            if (t0 + kLT <= P.t_zero) {                    // ... that nobody reads: not touched
                full_prev = false;                         // (no stores: the next body's wait covers its requests in full)
                continue;
            }
            const int r = 4 * w + (lane >> 4);             // [da | dg] = 0, two stores per wave as below
            const int cc = (lane & 15) ^ key(r);
            bf16* o = dadg + ((long long)b * T + t0 + r) * 256 + cc * 8;
            const u32x4 zero4 = {0u, 0u, 0u, 0u};
            st16_wt(o, zero4);
            st16_wt(o + 128, zero4);
            full_prev = true;
            continue;
        }
        const bool fix_old = t0 < d;
        const bool fix_do = false;
        if (fix_old || fix_do) {
            for (int r = w; r < kLT; r += 8) {
                if (fix_old && t0 + r < d) *reinterpret_cast<unsigned*>(xold(buf) + r * 256 + lane * 4) = 0u;
                if (fix_do && t0 + r >= T) *reinterpret_cast<unsigned*>(dot(buf) + r * 256 + lane * 4) = 0u;
            }
            barrier();
        }
        const int t = t0 + j;
        // ---- recompute the gate pre-activations of this wave's 16 channels ----
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            // every column operand of the phase is requested before the first MFMA: paired one by one (read -> wait -> MFMA) the
            // sixteen LDS latencies lay end to end (1,300 cycles for 512 cycles of matrix work, in-kernel stamps)
            bf16x8 fr[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) fr[s] = frag_row(s < 8 ? xold(buf) : xcur(buf), j, s & 7, h);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cA[s], fr[s], acc, 0, 0, 0);
        }
        // ---- dz = Wp^T dout + dz_skip (registers 0..7; rows 16..31 of the A tile are zero) ----
        f32x16 dz;
#pragma unroll
        for (int r = 0; r < 16; ++r) dz[r] = 0.f;
        if (HAS_DZ) {
            if (t0 + kLT > dz_t0) {
                const bool in = t >= dz_t0;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const bf16x4 v = *reinterpret_cast<const bf16x4*>(dzt(buf) + toff(j, 2 * w + q) + 8 * h);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dz[4 * q + e] = in ? (float)v[e] : 0.f;
                }
            }
        }
        if (HAS_DO) {
            bf16x8 fr[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) fr[s] = frag_row(dot(buf), j, s, h);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 8; ++s) dz = __builtin_amdgcn_mfma_f32_32x32x16_bf16(zA[s], fr[s], dz, 0, 0, 0);
        }
        // ---- gate forward + backward, elementwise ----
        const bool live = t >= Z && t < T;
        if constexpr (MODE != kCondNone) {
            if (next_reqs) wait_vm<kReqs>(); else wait_vm<0>();      // issue(next)'s requests may stay in flight: the rows are older
            rows_tie(ya); rows_tie(yb);
            if constexpr (MODE == kCondLinear) {
                rows_tie(yc); rows_tie(yd);
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        ya[q][e] = wn::bias_lerp(ya[q][e], yc[q][e], alpha);
                        yb[q][e] = wn::bias_lerp(yb[q][e], yd[q][e], alpha);
                    }
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[4 * q + e] += ya[q][e]; acc[8 + 4 * q + e] += yb[q][e]; }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            float da[4], dg[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float f, g;
                gate_fg(live ? acc[4 * q + e] : 0.f, live ? acc[8 + 4 * q + e] : 0.f, f, g);
                const float dzv = live ? dz[4 * q + e] : 0.f;
                da[e] = dzv * g * (1.f - f * f);
                dg[e] = dzv * f * g * (1.f - g);
            }
            const int o = toff(j, 2 * w + q) + 8 * h;
            *reinterpret_cast<bf16x4*>(dat + o) = pack4(da[0], da[1], da[2], da[3]);
            *reinterpret_cast<bf16x4*>(dgt + o) = pack4(dg[0], dg[1], dg[2], dg[3]);
        }
        barrier();
        // ---- [da | dg] rows leave whole: 512-byte rows, da in the first half ----
        const bool full = t0 + kLT <= T;
        {
            const int r = 4 * w + (lane >> 4);
            const int cc = (lane & 15) ^ key(r);
            const u32x4 va = *reinterpret_cast<const u32x4*>(dat + w * 1024 + lane * 16);
            const u32x4 vg = *reinterpret_cast<const u32x4*>(dgt + w * 1024 + lane * 16);
            bf16* o = dadg + ((long long)b * T + t0 + r) * 256 + cc * 8;
            if (full || t0 + r < T) {
                st16_wt(o, va);
                st16_wt(o + 128, vg);
            }
        }
        full_prev = full;
    }
}

template <bool HAS_DO, bool HAS_DZ, int MODE>
__global__ __launch_bounds__(512, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void k16_gate_bwd(
    const bf16* __restrict__ x, const bf16* __restrict__ convA, const bf16* __restrict__ dzA,
    const bf16* __restrict__ dout, const bf16* __restrict__ dzs, int dz_t0, bf16* __restrict__ dadg, int B, int T, int d,
    int Z, int tiles_per_b, int ntiles, int t_live, int t_zero, const LayerRows R) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const GateP P{x, convA, dzA, dout, dzs, dz_t0, dadg, B, T, d, Z, tiles_per_b, ntiles, t_live, t_zero, R};
    gate_phase<HAS_DO, HAS_DZ, MODE>(lds, P);
}

// ---------------------------------------------------------------------------------------------
// dx + dWp.  512 threads, one workgroup per CU (no VALU-heavy phase here).  Wave (mt = w & 3, kh = w >> 2): output rows
// 32 mt .., contraction half kh (0: dab[t] with the tap-1 weights, 1: dab[t + d] with the tap-0 weights); the halves
// meet in an fp32 LDS patch.  LDS: (da, dg, da', dg', dout, z) x 2 buffers = 96 KB + 16 KB exchange + 8 KB dx tile
// ---------------------------------------------------------------------------------------------
static constexpr int kDxLds = 12 * kLTileB + 16384 + kLTileB;
static constexpr int kDwpPart = 128 * 128;             // floats per workgroup partial of dWp

// One layer's dx (+ the projection gradient of the layer below) over this workgroup's tiles.
template <bool HAS_DO, bool HAS_Z>
__device__ __forceinline__ void dx_phase(char* lds, const DxP& P) {
    using M = DxMap;
    const bf16* __restrict__ dxA = P.dxA; bf16* __restrict__ dx = P.dx; float* __restrict__ dwp_part = P.dwp_part;
    const int T = P.T, d = P.d, tiles_per_b = P.tiles_per_b, ntiles = P.ntiles, t_live = P.t_live;
    // t_live (a multiple of 32): dx is exactly zero below it (no gradient reaches those columns); such tiles store zeros
    auto tile_at = [&](int buf, int which) { return lds + M::at(buf, which) * kLTileB; };   // da dg da' dg' dout z
    float* xch = reinterpret_cast<float*>(lds + M::xch * kLTileB);
    char* dxt = lds + M::dxt * kLTileB;
    const WaveC c = wave_consts(lds);
    const int lane = c.lane, w = c.w;
    const int j = lane & 31, h = lane >> 5;
    const int mt = w & 3, kh = w >> 2;
    int first, stride, last;
    tile_range(ntiles, first, stride, last);
    const int n = first < last ? (last - first + stride - 1) / stride : 0;     // this workgroup's tiles

    // dWp[cr][cd] partial: wave w owns rows cr 32 (w & 3) .. + 31, columns cd 64 (w >> 2) .. + 63
    f32x16 wp[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) { wp[0][r] = 0.f; wp[1][r] = 0.f; }

    auto issue = [&](int tile, int buf) { dx_issue<HAS_DO, HAS_Z>(lds, P, c, tile, buf); };

    // the first tile's requests, then this wave's A operands (the two round trips overlap)
    if (n > 0) issue(first, 0);
    bf16x8 A[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) A[s] = *reinterpret_cast<const bf16x8*>(dxA + (((mt * 2 + kh) * 16 + s) * 64 + lane) * 8);
#pragma unroll
    for (int s = 0; s < 16; ++s) asm volatile("" ::"v"(A[s]));
    bool full_prev = false;
    int it = 0;
    for (int tile = first; tile < last; tile += stride, ++it) {
        const int buf = it & 1;
        const int b = tile / tiles_per_b;
        const int t0 = (tile - b * tiles_per_b) * kLT;
        if (full_prev) wait_vm<1>(); else wait_vm<0>();  // one dx store per wave and tile
        barrier();
        if (tile + stride < last) issue(tile + stride, buf ^ 1);
        if (t0 + kLT <= t_live) {                          // dead tile (workgroup-uniform)
            if (!P.zero_dead) {                            // ... that nobody reads: not touched
                full_prev = false;
                continue;
            }
            const int r = 4 * w + (lane >> 4);             // dx = 0, one store per wave as below
            const int cc = (lane & 15) ^ key(r);
            const u32x4 zero4 = {0u, 0u, 0u, 0u};
            st16_wt(dx + ((long long)b * T + t0 + r) * 128 + cc * 8, zero4);
            full_prev = true;
            continue;
        }
        {
            // rows that are zero by construction and were never written (or never requested): dab[t + d] beyond the clip end
            // and below this layer's gate bound; the tile's own [da | dg] and dout when it lies below the gate bound
            const bool hi_fix = t0 + kLT + d > T, lo_fix = t0 + d < P.t_gate, own_dead = t0 + kLT <= P.t_gate;
            if (hi_fix || lo_fix || own_dead) {
                for (int r = w; r < kLT; r += 8) {
                    if (t0 + r + d >= T || t0 + r + d < P.t_gate) {
                        *reinterpret_cast<unsigned*>(tile_at(buf, 2) + r * 256 + lane * 4) = 0u;
                        *reinterpret_cast<unsigned*>(tile_at(buf, 3) + r * 256 + lane * 4) = 0u;
                    }
                    if (own_dead) {
                        *reinterpret_cast<unsigned*>(tile_at(buf, 0) + r * 256 + lane * 4) = 0u;
                        *reinterpret_cast<unsigned*>(tile_at(buf, 1) + r * 256 + lane * 4) = 0u;
                        if (HAS_DO) *reinterpret_cast<unsigned*>(tile_at(buf, 4) + r * 256 + lane * 4) = 0u;
                    }
                }
                barrier();
            }
        }
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            bf16x8 fr[16];                               // all sixteen operands requested before the first MFMA (as in k16_gate_bwd)
#pragma unroll
            for (int s = 0; s < 16; ++s) fr[s] = frag_row(tile_at(buf, 2 * kh + (s >> 3)), j, s & 7, h);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[s], fr[s], acc, 0, 0, 0);
        }
        // the two contraction halves meet: wave kh keeps accumulator quarters 2 kh, 2 kh + 1 and hands the other two to its
        // partner (before, one half handed over everything and idled through the other's 1,200-cycle combine)
        auto hand_over = [&](auto KH) {                   // (constant register indices: kh is uniform but not a constant)
            constexpr int kk = decltype(KH)::value;
#pragma unroll
            for (int r = 0; r < 8; ++r) xch[(mt * 16 + 8 * (1 - kk) + r) * 64 + lane] = acc[8 * (1 - kk) + r];
        };
        auto combine = [&](auto KH) {
            constexpr int kk = decltype(KH)::value;
            const bool valid = t0 + j < T;               // rows beyond the clip must not reach dWp
#pragma unroll
            for (int qq = 0; qq < 2; ++qq) {
                constexpr int q0 = 2 * kk;
                const int q = q0 + qq;
                const int o = toff(j, 4 * mt + q) + 8 * h;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[4 * q + e] + xch[(mt * 16 + 4 * q + e) * 64 + lane];
                if (HAS_DO) {
                    const bf16x4 xv = *reinterpret_cast<const bf16x4*>(tile_at(buf, 4) + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += (float)xv[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = valid ? v[e] : 0.f;
                *reinterpret_cast<bf16x4*>(dxt + o) = pack4(v[0], v[1], v[2], v[3]);
            }
        };
        if (kh == 0) hand_over(std::integral_constant<int, 0>{}); else hand_over(std::integral_constant<int, 1>{});
        barrier();
        if (kh == 0) combine(std::integral_constant<int, 0>{}); else combine(std::integral_constant<int, 1>{});
        barrier();
        if (HAS_Z) {
            // dWp += dx z^T over this tile's 32 columns (contraction over time: transposed LDS reads)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 a = frag_tr(dxt, 16 * ks, 32 * (w & 3), lane);
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const bf16x8 bz = frag_tr(tile_at(buf, 5), 16 * ks, 64 * (w >> 2) + 32 * n, lane);
                    wp[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bz, wp[n], 0, 0, 0);
                }
            }
        }
        const bool full = t0 + kLT <= T;
        {
            const int r = 4 * w + (lane >> 4);
            const int cc = (lane & 15) ^ key(r);
            const u32x4 v = *reinterpret_cast<const u32x4*>(dxt + w * 1024 + lane * 16);
            if (full || t0 + r < T) st16_wt(dx + ((long long)b * T + t0 + r) * 128 + cc * 8, v);
        }
        full_prev = full;
    }
    if (HAS_Z) {
        // this workgroup's partial of dWp: [cr][cd] fp32, summed over workgroups by k16_reduce_parts
        float* o = dwp_part + (long long)blockIdx.x * kDwpPart;
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                o[(32 * (w & 3) + acc_row(r, h)) * 128 + 64 * (w >> 2) + 32 * n + j] = wp[n][r];
    }
}

template <bool HAS_DO, bool HAS_Z>
__global__ __launch_bounds__(512, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void k16_dx(const bf16* __restrict__ dadg, const bf16* __restrict__ dxA,
                                                  const bf16* __restrict__ dout, const bf16* __restrict__ zprev,
                                                  bf16* __restrict__ dx, float* __restrict__ dwp_part, int B, int T, int d,
                                                  int tiles_per_b, int ntiles, int t_live, int t_gate, int zero_dead) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const DxP P{dadg, dxA, dout, zprev, dx, dwp_part, B, T, d, tiles_per_b, ntiles, t_live, t_gate, zero_dead};
    dx_phase<HAS_DO, HAS_Z>(lds, P);
}

// dW[e] += sum over workgroups of part[wg][e]  (fixed order: deterministic).  blockIdx.y = layer.
struct ReduceArgs { float* dW[kMaxProb16]; };
__global__ void k16_reduce_parts(const float* __restrict__ part, long long layer_stride, int nwg, int n, ReduceArgs dW) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float* o = dW.dW[blockIdx.y];
    if (!o) return;
    const float* p = part + (long long)blockIdx.y * layer_stride + e;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 4 <= nwg; g += 4) {
        s0 += p[(long long)g * n]; s1 += p[(long long)(g + 1) * n];
        s2 += p[(long long)(g + 2) * n]; s3 += p[(long long)(g + 3) * n];
    }
    for (; g < nwg; ++g) s0 += p[(long long)g * n];
    o[e] += (s0 + s1) + (s2 + s3);
}

// ---------------------------------------------------------------------------------------------
// gate-row gradients (conditioning): the column sums of the retained [da | dg] of EVERY layer in one launch, a gather per
// output row.  Workgroup (row j, chunk c; layer; clip), 128 threads, two of the 256 columns each: the positions of the row's
// range -- [0, T) with one row per clip, frame j, or frames j - 1 and j with interpolation -- are cut into chunks of kRowChunk from
// the range's first position on, a thread adds its chunk in ascending t (fp32, fma with the weight).  One chunk per row: the
// sum is added to the gradient row at once.  More: the chunks' sums go to the workspace and k16_row_grads_reduce adds them in
// chunk order.  Rows below lo[l] (unwritten memory below the layer's zero bound, the zero prefix) are not read.
// ---------------------------------------------------------------------------------------------
struct RowGradArgs { float* dbf[kMaxProb16]; float* dbg[kMaxProb16]; int lo[kMaxProb16]; };

__device__ __forceinline__ float* row_grad_out(const LayerRows& R, const RowGradArgs& A, int l, int b, int row, int col) {
    float* o = col < 128 ? A.dbf[l] : A.dbg[l];
    return o + (long long)b * R.clip_stride + (long long)row * R.fr.stride + (col & 127);
}

template <int MODE>
__global__ __launch_bounds__(128) void k16_row_grads(const bf16* __restrict__ dadg, const LayerRows R, const RowGradArgs A,
                                                     int B, int T, int nrows, int nch, float* __restrict__ part) {
    const int l = blockIdx.y, b = blockIdx.z;
    const int row = blockIdx.x / nch, c = blockIdx.x - row * nch;
    const long long hop = R.fr.hop;
    const int ph = MODE >= kCondFrame ? wn::frame_phase(R.fr, b) : 0;
    long long a = 0, e = T, mid = 0;                    // the row's range [a, e); linear: frame j - 1 below mid, frame j from it on
    if (MODE == kCondFrame) { a = row * hop - ph; e = a + hop; }
    if (MODE == kCondLinear) { mid = row * hop - ph; a = mid - hop; e = mid + hop; }
    if (a < 0) a = 0;
    if (e > T) e = T;
    long long t = a + (long long)c * kRowChunk;
    const long long hi = t + kRowChunk < e ? t + kRowChunk : e;
    if (t < A.lo[l]) t = A.lo[l];
    const bf16x2* src = reinterpret_cast<const bf16x2*>(dadg) + ((long long)l * B + b) * T * 128 + threadIdx.x;
    auto weight = [&](long long tt) {                  // 1 - alpha_t in frame j, alpha_t in frame j - 1 (wn::bias_frame_alpha's value)
        if (MODE != kCondLinear) return 1.f;
        const float al = wn::bias_alpha((int)(tt < mid ? tt - (mid - hop) : tt - mid), R.fr.hop);
        return tt < mid ? al : __fsub_rn(1.f, al);
    };
    float s0 = 0.f, s1 = 0.f;
    for (; t + 8 <= hi; t += 8) {
        bf16x2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(t + u) * 128];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float wt = weight(t + u);
            s0 = __fmaf_rn(wt, (float)v[u][0], s0);
            s1 = __fmaf_rn(wt, (float)v[u][1], s1);
        }
    }
    for (; t < hi; ++t) {
        const bf16x2 v = src[t * 128];
        const float wt = weight(t);
        s0 = __fmaf_rn(wt, (float)v[0], s0);
        s1 = __fmaf_rn(wt, (float)v[1], s1);
    }
    const int col = 2 * threadIdx.x;
    if (nch == 1) {
        float* o = row_grad_out(R, A, l, b, row, col);
        o[0] += s0;
        o[1] += s1;
    } else {
        float* o = part + ((((long long)l * B + b) * nrows + row) * nch + c) * 256 + col;
        o[0] = s0;
        o[1] = s1;
    }
}

__global__ __launch_bounds__(128) void k16_row_grads_reduce(const float* __restrict__ part, const LayerRows R, const RowGradArgs A,
                                                            int B, int nrows, int nch) {
    const int l = blockIdx.y, b = blockIdx.z, row = blockIdx.x, col = 2 * threadIdx.x;
    const float* p = part + (((long long)l * B + b) * nrows + row) * nch * 256 + col;
    float s0 = p[0], s1 = p[1];
    for (int c = 1; c < nch; ++c) { s0 += p[(long long)c * 256]; s1 += p[(long long)c * 256 + 1]; }
    float* o = row_grad_out(R, A, l, b, row, col);
    o[0] += s0;
    o[1] += s1;
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------
static int grid_for(int ntiles, int per_cu) {
    int g = ntiles < 256 * per_cu ? ntiles : 256 * per_cu;
    if (g >= 8) g &= ~7;
    return g;
}

int fwd_layer(const bf16* x, const bf16* img, bf16* out, bf16* z, int B, int T, int d, int Z, const LayerRows& R,
              hipStream_t s) {
    const int tiles_per_b = (T + kLT - 1) / kLT;
    const int ntiles = B * tiles_per_b;
#define FWD_LAUNCH(MODE)                                                                                               \
    do {                                                                                                               \
        WN_MAX_LDS_ONCE(kFwdLds, k16_fwd<MODE>);                                                                       \
        hipLaunchKernelGGL(k16_fwd<MODE>, dim3(grid_for(ntiles, 2)), dim3(256), kFwdLds, s, x, img, img + kConvA, out, \
                           z, B, T, d, Z, tiles_per_b, ntiles, R);                                                     \
    } while (0)
    switch (R.mode) {
        case kCondNone: FWD_LAUNCH(kCondNone); break;
        case kCondClip: FWD_LAUNCH(kCondClip); break;
        case kCondFrame: FWD_LAUNCH(kCondFrame); break;
        case kCondLinear: FWD_LAUNCH(kCondLinear); break;
        default: wn::set_error("fwd_layer: unknown row mode %d", R.mode); return WN_EARG;
    }
#undef FWD_LAUNCH
    WN_LAUNCH_CHECK();
    return WN_OK;
}

int gate_bwd_layer(const bf16* x, const bf16* img, const bf16* dout, const bf16* dzs, int dz_t0, bf16* dadg, int B, int T,
                   int d, int Z, int t_live, int t_zero, const LayerRows& R, hipStream_t s) {
    const int tiles_per_b = (T + kLT - 1) / kLT;
    const int ntiles = B * tiles_per_b;
    const int grid = grid_for(ntiles, 1);
#define GB_LAUNCH_M(DO, DZ, MODE)                                                                                      \
    do {                                                                                                               \
        WN_MAX_LDS_ONCE(kGateLds, k16_gate_bwd<DO, DZ, MODE>);                                                         \
        hipLaunchKernelGGL((k16_gate_bwd<DO, DZ, MODE>), dim3(grid), dim3(512), kGateLds, s, x, img + kOffConvA8,     \
                           img + kOffDzA8, dout, dzs, dz_t0, dadg, B, T, d, Z, tiles_per_b, ntiles, t_live, t_zero, R); \
    } while (0)
#define GB_LAUNCH(DO, DZ)                                                                                              \
    switch (R.mode) {                                                                                                  \
        case kCondNone: GB_LAUNCH_M(DO, DZ, kCondNone); break;                                                         \
        case kCondClip: GB_LAUNCH_M(DO, DZ, kCondClip); break;                                                         \
        case kCondFrame: GB_LAUNCH_M(DO, DZ, kCondFrame); break;                                                       \
        case kCondLinear: GB_LAUNCH_M(DO, DZ, kCondLinear); break;                                                     \
        default: wn::set_error("gate_bwd_layer: unknown row mode %d", R.mode); return WN_EARG;                         \
    }
    if (dout && dzs) { GB_LAUNCH(true, true); }
    else if (dout) { GB_LAUNCH(true, false); }
    else if (dzs) { GB_LAUNCH(false, true); }
    else { wn::set_error("gate_bwd_layer: no incoming gradient"); return WN_EARG; }
#undef GB_LAUNCH
#undef GB_LAUNCH_M
    WN_LAUNCH_CHECK();
    return WN_OK;
}

// rows of a clip's block and chunks per row of the row-gradient launch
static void row_grad_geometry(const LayerRows& R, int T, long long& nrows, long long& nch) {
    nrows = R.mode >= kCondFrame ? R.fr.rows(T) : 1;
    long long span = R.mode == kCondFrame ? R.fr.hop : R.mode == kCondLinear ? 2ll * R.fr.hop : T;
    if (span > T) span = T;
    nch = (span + kRowChunk - 1) / kRowChunk;
}

size_t row_grad_ws_bytes(const LayerRows& R, int L, int B, int T) {
    if (R.mode == kCondNone) return 0;
    long long nrows, nch;
    row_grad_geometry(R, T, nrows, nch);
    return nch > 1 ? (size_t)L * B * nrows * nch * 256 * sizeof(float) : 0;
}

int row_grads(const bf16* dadg, const LayerRows& R, float* const* dbf, float* const* dbg, const int* lo, int L, int B, int T,
              float* part, hipStream_t s) {
    if (L > kMaxProb16) { wn::set_error("w16: more than %d layers", kMaxProb16); return WN_ESHAPE; }
    long long nrows, nch;
    row_grad_geometry(R, T, nrows, nch);
    if (nrows * nch > 2147483647ll || B > 65535) { wn::set_error("w16 row gradients: too many rows or clips for one launch"); return WN_ESHAPE; }
    RowGradArgs a{};
    for (int l = 0; l < L; ++l) { a.dbf[l] = dbf[l]; a.dbg[l] = dbg[l]; a.lo[l] = lo[l]; }
    const dim3 grid((unsigned)(nrows * nch), L, B);
    switch (R.mode) {
        case kCondClip: hipLaunchKernelGGL(k16_row_grads<kCondClip>, grid, dim3(128), 0, s, dadg, R, a, B, T, (int)nrows, (int)nch, part); break;
        case kCondFrame: hipLaunchKernelGGL(k16_row_grads<kCondFrame>, grid, dim3(128), 0, s, dadg, R, a, B, T, (int)nrows, (int)nch, part); break;
        case kCondLinear: hipLaunchKernelGGL(k16_row_grads<kCondLinear>, grid, dim3(128), 0, s, dadg, R, a, B, T, (int)nrows, (int)nch, part); break;
        default: wn::set_error("row_grads: unknown row mode %d", R.mode); return WN_EARG;
    }
    WN_LAUNCH_CHECK();
    if (nch > 1) {
        hipLaunchKernelGGL(k16_row_grads_reduce, dim3((unsigned)nrows, L, B), dim3(128), 0, s, part, R, a, B, (int)nrows, (int)nch);
        WN_LAUNCH_CHECK();
    }
    return WN_OK;
}

int dx_grid(int B, int T) { return grid_for(B * ((T + kLT - 1) / kLT), 1); }

// dx = dout + conv^T(dadg); zprev (the z of the layer BELOW, may be NULL) -> that layer's dWp partial tiles
int dx_layer(const bf16* dadg, const bf16* img, const bf16* dout, const bf16* zprev, bf16* dx, float* dwp_part, int B,
             int T, int d, int t_live, int t_gate, int zero_dead, hipStream_t s) {
    const int tiles_per_b = (T + kLT - 1) / kLT;
    const int ntiles = B * tiles_per_b;
    const int grid = dx_grid(B, T);
#define DX_LAUNCH(DO, ZZ)                                                                                              \
    do {                                                                                                               \
        WN_MAX_LDS_ONCE(kDxLds, k16_dx<DO, ZZ>);                                                                       \
        hipLaunchKernelGGL((k16_dx<DO, ZZ>), dim3(grid), dim3(512), kDxLds, s, dadg, img + kOffDxA, dout,                \
                           zprev, dx, dwp_part, B, T, d, tiles_per_b, ntiles, t_live, t_gate, zero_dead);             \
    } while (0)
    if (dout && zprev) DX_LAUNCH(true, true);
    else if (dout) DX_LAUNCH(true, false);
    else if (zprev) DX_LAUNCH(false, true);
    else DX_LAUNCH(false, false);
#undef DX_LAUNCH
    WN_LAUNCH_CHECK();
    return WN_OK;
}

int reduce_parts(const float* part, long long layer_stride, int nwg, int n, float* const* dW, int L, hipStream_t s) {
    if (L > kMaxProb16) { wn::set_error("w16: more than %d layers", kMaxProb16); return WN_ESHAPE; }
    ReduceArgs a{};
    for (int l = 0; l < L; ++l) a.dW[l] = dW[l];
    hipLaunchKernelGGL(k16_reduce_parts, dim3((n + 255) / 256, L), dim3(256), 0, s, part, layer_stride, nwg, n, a);
    WN_LAUNCH_CHECK();
    return WN_OK;
}


}  // namespace w16

