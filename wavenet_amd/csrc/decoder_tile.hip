// Batched decoding in utterance tiles: the any-shape step loop (decoder.hip, decode_steps) for U utterances per workgroup that
// share one read of the packed weights.  wn_decoder_run_batch (decoder.hip) makes every check and fills the utterances' table;
// this file holds the kernel and its launch.  It is a translation unit of its own so that k_decode and k_decode_batch compile
// to the instructions they were.
#include "wn_kernels.hpp"
#include "decoder_types.hpp"
#include "sample_filter.hpp"

namespace wn {

static constexpr int kDecThreads = 512;          // (decoder.hip's)

__device__ __forceinline__ int pmod(long long a, int D) {
    long long r = a % D;
    return (int)(r < 0 ? r + D : r);
}
// the draw of one row by one thread, as decode_steps' thread 0 makes it, here by a slot's owner thread -- numpy legacy
// choice: float64 cumsum, divide by the total, first index with cdf > u
__device__ __forceinline__ int draw_index(const float* p, int Q, double u) {
    double tot = 0.0;
    for (int q = 0; q < Q; ++q) tot += (double)p[q];
    double c = 0.0;
    int idx = Q;
    for (int q = 0; q < Q; ++q) {
        c += (double)p[q];
        if (c / tot > u) { idx = q; break; }
    }
    if (idx >= Q) idx = Q - 1;
    return idx;
}


// ---- utterance tiles ---------------------------------------------------------------------------
// wn_decoder_run_batch with same_weights = U in {2, 4, 8, 16} on any-shape handles: workgroup g decodes utterances
// [gU, gU + U) of the launch against ONE copy of the packed weights, handle 0's.  The activations lie in LDS as
// [channel][slot], so a thread that holds a weight in a register reads a channel's values of its slots from one address.
// Every output element of every utterance is formed by the fp32 operations decode_steps forms it by, in its order: bias,
// frame value, taps k ascending, channels c ascending, residual add last -- between two taps an accumulator rests in LDS
// (a store and a load of an fp32 value change no bit).  A thread takes UG = min(U, 4) slots of one output; the U / UG slot
// groups of an output go to different threads, so narrow layers still fill the workgroup.
// Shared (handle 0's arena and tables): embedding, causal weights and biases, wfg, wps, bps, the head.  Own: rings, token
// ring, static gate biases (arena_u[L.bfg]), frame table / ring, controls, counters, uniforms and outputs.
// A slot is live at step `it` iff it has an utterance and it < its nsteps.  A slot that is not live reads and writes
// nothing outside LDS, and its LDS columns hold 0.
template <int U> struct Tile {
    static constexpr int UG = U < 4 ? U : 4;      // slots per thread
    static constexpr int G = U / UG;              // slot groups of one output
};
// one slot of a tile (LDS): DecAnyUtt's own part, and the slot's state from step to step
struct TileSlot {
    float* arena; int* tok_ring; const double* uniforms; int32_t* out_tokens; float* prob_out;
    const float* ftab; const float* frow; const float* fnext;
    long long n0, pos0; double top_p;
    float inv_temp, falpha;
    int top_k, nsteps, hop, row, ring, token, ftok, rslot, rrem;
};
template <int UG>
__device__ __forceinline__ void lds_slots(const float* p, float (&x)[UG]) {
    if constexpr (UG == 4) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else if constexpr (UG == 2) {
        const float2 v = *reinterpret_cast<const float2*>(p);
        x[0] = v.x; x[1] = v.y;
    } else {
        x[0] = p[0];
    }
}
// One tap of a matrix-vector product for every slot: acc = init(o, slot), then acc += w[c][o] * x[c][slot] for c ascending,
// then fin(o, slot, acc).  w is read once per thread and c, x from LDS ([c][U]).
template <int U, class Init, class Fin>
__device__ __forceinline__ void tile_matvec(const float* __restrict__ w, int cin, int nout, const float* x, Init init, Fin fin) {
    constexpr int UG = Tile<U>::UG, G = Tile<U>::G;
    const int NT = blockDim.x;
    for (int i = threadIdx.x; i < nout * G; i += NT) {
        const int g = G == 1 ? 0 : i / nout, o = i - g * nout, j0 = g * UG;
        float acc[UG];
#pragma unroll
        for (int j = 0; j < UG; ++j) acc[j] = init(o, j0 + j);
        const float* wp = w + o;
        const float* xp = x + j0;
#pragma unroll 8
        for (int c = 0; c < cin; ++c) {
            const float wv = wp[(long long)c * nout];
            float xv[UG];
            lds_slots<UG>(xp + c * U, xv);
#pragma unroll
            for (int j = 0; j < UG; ++j) acc[j] += wv * xv[j];
        }
#pragma unroll
        for (int j = 0; j < UG; ++j) fin(o, j0 + j, acc[j]);
    }
}
// block_reduce for U rows at once: each row's operations and their order are block_reduce's (red: [waves][U])
template <int U>
__device__ __forceinline__ void block_reduce_tile(float (&v)[U], bool is_max, float* red) {
#pragma unroll
    for (int j = 0; j < U; ++j)
        for (int o = 32; o > 0; o >>= 1) {
            float w = __shfl_xor(v[j], o);
            v[j] = is_max ? fmaxf(v[j], w) : v[j] + w;
        }
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < U; ++j) red[(threadIdx.x >> 6) * U + j] = v[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < U; ++j) {
        float r = red[j];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, red[w * U + j]) : r + red[w * U + j];
        v[j] = r;
    }
}

template <int U, bool LERP, bool FORCED, bool RING>
__global__ __launch_bounds__(kDecThreads) void k_decode_tile(DecMeta M, const DecAnyUtt* __restrict__ tab, int n_utt, int prob_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ TileSlot sl[U];
    const int tid = threadIdx.x, NT = blockDim.x;
    const int u0 = (int)blockIdx.x * U;
    if (u0 >= n_utt) return;
    const int cnt = n_utt - u0 < U ? n_utt - u0 : U;          // the last tile may be short
    const int S = M.maxc * U;
    float* xcur = sm;                    // [maxc][U] current column of the residual stream / causal stack
    float* xnew = xcur + S;              // [maxc][U] (and the staged tap column of the gate)
    float* ab = xnew + S;                // [2*maxc][U] gate pre-activations; behind the head: U rows of maxc probabilities
    float* zz = ab + 2 * S;              // [maxc][U] (and the staged tap column of causal layers >= 1)
    float* skip = zz + S;                // [maxc][U]
    float* hbuf = skip + S;              // [maxc][U]
    float* red = hbuf + S;               // [16][U]
    // the shared side: handle 0's tables and arena
    const DecCausal* __restrict__ causal = tab[0].causal;
    const DecLayer* __restrict__ layers = tab[0].layers;
    const DecHead* __restrict__ heads = tab[0].heads;
    const float* __restrict__ arena0 = tab[0].arena;
    int maxn = 0;
    for (int j = 0; j < cnt; ++j) maxn = tab[u0 + j].nsteps > maxn ? tab[u0 + j].nsteps : maxn;
    if (tid < U) {
        TileSlot s{};                    // a slot without an utterance: nsteps = 0, never live
        if (tid < cnt) {
            const DecAnyUtt q = tab[u0 + tid];
            s.arena = q.arena; s.tok_ring = q.tok_ring; s.uniforms = q.uniforms; s.out_tokens = q.out_tokens; s.prob_out = q.prob_out;
            s.ftab = q.fr.tab; s.n0 = q.n0; s.pos0 = q.fr.pos0; s.top_p = q.sc.top_p; s.inv_temp = q.sc.inv_temp; s.top_k = q.sc.top_k;
            s.nsteps = q.nsteps; s.hop = q.fr.hop; s.row = q.fr.row; s.ring = q.fr.ring; s.token = q.first_token;
            if (RING && q.fr.tab) {      // slot = (pos0 / hop) mod ring and p % hop of the first step once, then one increment per step
                const long long j = q.fr.pos0 / q.fr.hop;
                s.rslot = (int)(j % q.fr.ring);
                s.rrem = (int)(q.fr.pos0 - j * q.fr.hop);
            }
        }
        sl[tid] = s;
    }
    __syncthreads();

    for (int it = 0; it < maxn; ++it) {
        const auto live = [&](int j) { return it < sl[j].nsteps; };
        // ---- per slot, by thread `slot`: the entry a FORCED step may have to emit, and the step's frame row -----------------
        if (tid < U) {
            TileSlot& s = sl[tid];
            s.ftok = -1; s.frow = nullptr; s.fnext = nullptr; s.falpha = 0.f;
            if (it < s.nsteps) {
                if (FORCED) s.ftok = s.out_tokens[it];
                if (s.ftab) {
                    s.frow = RING ? s.ftab + s.rslot * (long long)s.row : s.ftab + ((s.pos0 + it) / s.hop) * (long long)s.row;
                    if (LERP) {
                        s.fnext = RING && s.rslot + 1 == s.ring ? s.ftab : s.frow + s.row;
                        s.falpha = __fdiv_rn(RING ? (float)s.rrem : (float)(int)((s.pos0 + it) % s.hop), (float)s.hop);
                    }
                    if (RING && ++s.rrem == s.hop) {         // the walk, for the next step
                        s.rrem = 0;
                        if (++s.rslot == s.ring) s.rslot = 0;
                    }
                }
            }
        }
        __syncthreads();
        // an utterance's ring column `back` steps ago -> dst[c][slot] (0 for a slot that is not live)
        const auto stage = [&](float* dst, int ringoff, int C, int D, long long back) {
            for (int i = tid; i < C * U; i += NT) {
                const int j = i / C, c = i - j * C;
                dst[c * U + j] = live(j) ? sl[j].arena[ringoff + (long long)pmod(sl[j].n0 + it - back, D) * C + c] : 0.f;
            }
        };
        // column n of every live utterance into its ring
        const auto keep = [&](const float* src, int ringoff, int C, int D) {
            for (int i = tid; i < C * U; i += NT) {
                const int j = i / C, c = i - j * C;
                if (live(j)) sl[j].arena[ringoff + (long long)pmod(sl[j].n0 + it, D) * C + c] = src[c * U + j];
            }
        };
        // ---- causal layer 0: two (fwc) gathered rows of the packed table ---------------------
        {
            const DecCausal L = causal[0];
            const int Dc = M.fwc - 1;
            for (int i = tid; i < L.cout * U; i += NT) {
                const int j = i / L.cout, c = i - j * L.cout;
                float acc = 0.f;
                if (live(j)) {
                    const long long n = sl[j].n0 + it;
                    acc = L.b >= 0 ? arena0[L.b + c] : 0.f;
                    for (int k = 0; k < M.fwc; ++k) {
                        int m = M.fwc - 1 - k;      // age of the tap
                        int q = m == 0 ? sl[j].token : sl[j].tok_ring[pmod(n - m, Dc)];
                        acc += arena0[L.w + ((long long)q * M.fwc + k) * L.cout + c];
                    }
                }
                xcur[c * U + j] = acc;
            }
            __syncthreads();
            if (tid < U && live(tid) && Dc > 0) sl[tid].tok_ring[pmod(sl[tid].n0 + it, Dc)] = sl[tid].token;
        }
        // ---- further causal layers (d = 1) ----------------------------------------------------
        for (int i = 1; i < M.ncausal; ++i) {
            const DecCausal L = causal[i];
            const int Dc = M.fwc - 1;
            for (int k = 0; k < M.fwc; ++k) {
                const int m = M.fwc - 1 - k;
                if (m > 0) {
                    stage(zz, L.ring, L.cin, Dc, m);
                    __syncthreads();
                }
                tile_matvec<U>(arena0 + L.w + (long long)k * L.cin * L.cout, L.cin, L.cout, m > 0 ? zz : xcur,
                    [&](int o, int j) { return k > 0 ? ab[o * U + j] : live(j) && L.b >= 0 ? arena0[L.b + o] : 0.f; },
                    [&](int o, int j, float v) { ab[o * U + j] = live(j) ? v : 0.f; });
                __syncthreads();
            }
            if (Dc > 0) keep(xcur, L.ring, L.cin, Dc);
            __syncthreads();
            for (int e = tid; e < L.cout * U; e += NT) xcur[e] = ab[e];
            __syncthreads();
        }
        for (int e = tid; e < M.Cs * U; e += NT) skip[e] = 0.f;
        // ---- residual layers ------------------------------------------------------------------
        int foff = 0;                    // layer j's 2 cd values of a frame row lie at the running offset
        for (int jl = 0; jl < M.nlayers; ++jl) {
            const DecLayer L = layers[jl];
            const int D = (M.fw - 1) * L.d;
            const int n2 = 2 * L.cd;
            // gate: ab[o2] = b + frame + sum_k sum_c WfgT[k*Cr+c][o2] x[n-(fw-1-k)d][c]
            for (int k = 0; k < M.fw; ++k) {
                const int m = M.fw - 1 - k;
                if (m > 0) {
                    stage(xnew, L.ring, M.Cr, D, (long long)m * L.d);
                    __syncthreads();
                }
                tile_matvec<U>(arena0 + L.wfg + (long long)k * M.Cr * n2, M.Cr, n2, m > 0 ? xnew : xcur,
                    [&](int o, int j) {
                        if (k > 0) return ab[o * U + j];
                        if (!live(j)) return 0.f;
                        const TileSlot& s = sl[j];
                        float acc = L.bfg >= 0 ? s.arena[L.bfg + o] : 0.f;      // the utterance's own static gate bias
                        if (LERP && s.fnext) acc += bias_lerp(s.frow[foff + o], s.fnext[foff + o], s.falpha);
                        else if (s.frow) acc += s.frow[foff + o];
                        return acc;
                    },
                    [&](int o, int j, float v) { ab[o * U + j] = live(j) ? v : 0.f; });
                __syncthreads();
            }
            for (int e = tid; e < L.cd * U; e += NT) zz[e] = fast_tanh(ab[e]) * fast_sigmoid(ab[L.cd * U + e]);
            // the ring slot of column n is the one that held column n-(fw-1)d: all reads are done
            if (D > 0) keep(xcur, L.ring, M.Cr, D);
            __syncthreads();
            // projections: rows [0,Cr) residual, rows [Cr,Cr+Cs) skip
            tile_matvec<U>(arena0 + L.wps, L.cd, M.Cr + M.Cs, zz,
                [&](int o, int j) { return live(j) && L.bps >= 0 ? arena0[L.bps + o] : 0.f; },
                [&](int o, int j, float v) {
                    if (o < M.Cr) xnew[o * U + j] = live(j) ? v + xcur[o * U + j] : 0.f;
                    else if (live(j)) skip[(o - M.Cr) * U + j] += v;
                });
            __syncthreads();
            for (int e = tid; e < M.Cr * U; e += NT) xcur[e] = xnew[e];
            __syncthreads();
            foff += n2;
        }
        // ---- head on the newest column only ---------------------------------------------------
        float* hin = skip;
        float* hout = hbuf;
        for (int i = 0; i < M.nhead; ++i) {
            const DecHead H = heads[i];
            // the activation once per input element, in place (the value every one of decode_steps' reads of it forms)
            for (int e = tid; e < H.cin * U; e += NT) hin[e] = act_apply(hin[e], M.head_act);
            __syncthreads();
            tile_matvec<U>(arena0 + H.w, H.cin, H.cout, hin,
                [&](int o, int j) { return live(j) && H.b >= 0 ? arena0[H.b + o] : 0.f; },
                [&](int o, int j, float v) { hout[o * U + j] = live(j) ? v : 0.f; });
            __syncthreads();
            float* t = hin; hin = hout; hout = t;
        }
        // ---- hin holds the Q logits of every slot: softmax, each row by block_reduce's operations ---------------------------
        float* rows = ab;                // slot j's probabilities: rows[j * maxc + q]
        {
            float mx[U], sv[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float it_ = sl[j].inv_temp;          // temperature: the fp32 logits times 1/T
                if (live(j) && it_ != 1.f)
                    for (int q = tid; q < M.Q; q += NT) hin[q * U + j] *= it_;
                mx[j] = -INFINITY;
                for (int q = tid; q < M.Q; q += NT) mx[j] = fmaxf(mx[j], hin[q * U + j]);
            }
            block_reduce_tile<U>(mx, true, red);
#pragma unroll
            for (int j = 0; j < U; ++j) {
                sv[j] = 0.f;
                for (int q = tid; q < M.Q; q += NT) sv[j] += expf(hin[q * U + j] - mx[j]);
            }
            block_reduce_tile<U>(sv, false, red);
            __syncthreads();
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const float inv = 1.f / sv[j];
                for (int q = tid; q < M.Q; q += NT) rows[j * M.maxc + q] = expf(hin[q * U + j] - mx[j]) * inv;
            }
            __syncthreads();
        }
        if (prob_stride)                 // the full row; prob_stride == 0 (kProbChosen): one float per step, at the draw below
            for (int i = tid; i < M.Q * U; i += NT) {
                const int j = i / M.Q, q = i - j * M.Q;
                if (live(j) && sl[j].prob_out) sl[j].prob_out[(long long)it * prob_stride + q] = rows[j * M.maxc + q];
            }
        // top-k / top-p, one slot after another (workgroup-uniform branches): a given step takes no filter
        for (int j = 0; j < U; ++j) {
            const bool given = FORCED && (unsigned)sl[j].ftok < (unsigned)M.Q;
            if (live(j) && !given && (sl[j].top_k > 0 || sl[j].top_p < 1.0))
                sample_filter<false>(rows + j * M.maxc, M.Q, tid, NT, sl[j].top_k, sl[j].top_p);
        }
        __syncthreads();
        // the draws, side by side: slot j's owner is lane j / 8 of wave j % 8
        {
            const int j = (tid & 63) * 8 + (tid >> 6);
            if ((tid & 63) < (U + 7) / 8 && j < U && live(j)) {
                TileSlot& s = sl[j];
                const float* p = rows + j * M.maxc;
                if (FORCED && (unsigned)s.ftok < (unsigned)M.Q) {
                    // a given step: no draw; out_tokens[it] holds the token already, and it enters the next step as a drawn one
                    s.token = s.ftok;
                    if (s.prob_out && !prob_stride) s.prob_out[it] = p[s.ftok];
                } else {
                    const int idx = draw_index(p, M.Q, s.uniforms[it]);
                    s.token = idx;
                    s.out_tokens[it] = idx;
                    if (s.prob_out && !prob_stride) s.prob_out[it] = p[idx];
                }
            }
        }
        __syncthreads();
    }
}

// k_decode_tile<U, ...> of a launch, or NULL for a U that is no tile size
template <int U>
static const void* tile_kernel_of(bool lerp, bool forced, bool ring) {
    const auto kern = ring ? (forced ? (lerp ? k_decode_tile<U, true, true, true> : k_decode_tile<U, false, true, true>)
                                     : (lerp ? k_decode_tile<U, true, false, true> : k_decode_tile<U, false, false, true>))
                           : (forced ? (lerp ? k_decode_tile<U, true, true, false> : k_decode_tile<U, false, true, false>)
                                     : (lerp ? k_decode_tile<U, true, false, false> : k_decode_tile<U, false, false, false>));
    return reinterpret_cast<const void*>(kern);
}
static const void* tile_kernel(int U, bool lerp, bool forced, bool ring) {
    return U == 2 ? tile_kernel_of<2>(lerp, forced, ring) : U == 4 ? tile_kernel_of<4>(lerp, forced, ring)
         : U == 8 ? tile_kernel_of<8>(lerp, forced, ring) : U == 16 ? tile_kernel_of<16>(lerp, forced, ring) : nullptr;
}

int decode_tile_launch(int U, bool lerp, bool forced, bool ring, const DecMeta& M, const DecAnyUtt* tab, int n_utt, int prob_stride,
                       size_t lds, hipStream_t s) {
    const void* tk = tile_kernel(U, lerp, forced, ring);
    WN_CHECK_ARG(tk, "decode_tile_launch: %d is no tile size", U);
    if (lds > 48 * 1024) WN_HIP(hipFuncSetAttribute(tk, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DecMeta meta = M;
    void* args[] = {&meta, &tab, &n_utt, &prob_stride};
    WN_HIP(hipLaunchKernel(tk, dim3(cdiv(n_utt, U)), dim3(kDecThreads), args, lds, s));
    return WN_OK;
}

}  // namespace wn
