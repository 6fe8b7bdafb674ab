// Queue-cached autoregressive decoder (FasterWaveNet._forward_one_step, faster_wavenet.py:50-113,
// driven by train_audio/generate.py:24-43).
//
// What the reference keeps per layer is a full-window cache (1,C,1,W) that it rolls by one column
// every step (faster_wavenet.py:72-73, 90-96) although only columns -1 and -1-d are ever read
// (wavenet.py:286,290,354).  Here each layer keeps a ring of its last (fw-1)*d INPUT columns in HBM
// (0.52 MB in total at 4 x 10 layers of 32 channels), the head runs on the newest column only, and
// the whole sample loop -- network step, softmax, numpy-compatible categorical draw, feedback of
// the drawn token -- runs inside ONE persistent workgroup, so a 16,000-sample utterance is one
// launch.  Sample n+1 depends on sample n through all layers, so there is nothing to spread
// over other CUs without paying a cross-CU hand-off per layer (MI355X_MICROARCH price list).
//
// Weights are re-packed once per handle into transposed form (consecutive threads read consecutive
// addresses): gate  WfgT[k*Cr+c][o2]  (o2 < 2Cd: filter then gate),  projections  WpsT[cd][o]
// (o < Cr+Cs: residual rows then skip rows), head  WhT[ci][co], first causal layer W0t[q][k][c].
#include <memory>
#include <new>
#include <vector>

#include "wn_kernels.hpp"
#include "decoder_types.hpp"
#include "sample_filter.hpp"

namespace wn {

static constexpr int kDecThreads = 512;

// local conditioning: the handle's own compact copy of the table -- n rows (room for cap) of `row` floats --, hop, phase, mode
// A WN_DECODER_FRAME_RING handle copies nothing: `ring` is the caller's memory, n its capacity R and row the caller's stride (tab
// stays NULL).
struct FrameTable { float* tab; int cap, n, hop, phase, row, interp; const float* ring; };

struct Decoder {
    DecMeta meta{};
    std::vector<DecCausal> causal;
    std::vector<DecLayer> layers;
    std::vector<DecHead> heads;
    float* arena = nullptr;       // packed weights + rings
    long long arena_floats = 0;
    int* tok_ring = nullptr;      // fwc-1 previous tokens
    void* dmeta = nullptr;        // device copies of causal/layers/heads tables
    DecCausal* d_causal = nullptr;
    DecLayer* d_layers = nullptr;
    DecHead* d_heads = nullptr;
    long long step = 0;           // index of the next column to be consumed
    size_t lds_bytes = 0;
    float* fastP = nullptr;       // packed weights of the specialised kernel (decoder_fast.hip), or NULL
    int head_bias_off = -1;
    bool three_wgs = true;        // wn_decoder_run on nine workgroups (decoder_fast.hip); WN_DECODER_ONE_WORKGROUP clears it
    bool gate_bias = false;       // ... and the last create / update gave it static gate biases (else its 64 floats per layer hold 0)
    bool gate_rows = false;       // created with WN_DECODER_GATE_ROWS (the handle's form is fixed at create): a fast handle that
                                  // takes static gate biases and a frame table -- wave 1 of the chain workgroup adds them
    bool trace_chosen = false;    // created with WN_DECODER_TRACE_CHOSEN (fixed at create, on every shape): a run's prob_trace is one
                                  // float per step, the drawn token's probability, not a row of Q
    bool forced = false;          // created with WN_DECODER_FORCED_TOKENS (fixed at create, on every shape): a run reads out_tokens[i] before
                                  // it writes it, and a step whose entry is a token of [0, Q) emits that token instead of drawing
    bool frame_ring = false;      // created with WN_DECODER_FRAME_RING (fixed at create, on every shape): the frame table is a ring in the
                                  // caller's memory, read in place (FrameTable.ring)
    bool ran_multi = false;       // a nine-workgroup run has been launched (its error entry is meaningful)
    SampleCtl ctl;                // wn_decoder_set_sampling: temperature / top-k / top-p of wn_decoder_run (off at create)
    // wn_decoder_run_batch on any-shape handles, as handle 0 of the call: the per-utterance table (DecAnyUtt) in device
    // memory, its pinned host image, and the event behind the last copy of the image (the image is rewritten after it)
    void* batch_tab = nullptr;
    void* batch_img = nullptr;
    int batch_cap = 0;
    hipEvent_t batch_copied = nullptr;
    FrameTable frames{};          // local conditioning (WnDecoderDesc.frame_bias); n == 0: none
    // steps run since the last create / update call -- the call that sets the frame table AND the step limit, so one counter
    // serves both: the table row of a step and the steps left under WnDecoderDesc.step_limit (0: no limit)
    long long since_set = 0;
    int step_limit = 0;
    unsigned long long src_key = 0;   // hash of the caller's weight POINTERS at the last pack: two handles packed from the same
                                      // model carry the same key (wn_decoder_run_batch's same_weights check)
    unsigned long long tile_key = 0;  // ... the same hash without the gate-bias pointers: what a tile shares (same_weights >= 2 on
                                      // any-shape handles; the static gate biases stay an utterance's own)
};

// the shape decoder_fast.hip is written for (BASELINE.json config 4 with the reference's default biases).  Gate biases
// (bf / bg) and a frame table deselect it unless the description carries WN_DECODER_GATE_ROWS; bp / bs, a causal bias and
// WN_EXEC_FORCE_GENERIC always do
static bool fast_shape(const WnDecoderDesc* d) {
    const bool rows = (d->flags & WN_DECODER_GATE_ROWS) != 0;
    if (d->flags & WN_EXEC_FORCE_GENERIC) return false;
    if (!(d->Q == 256 && d->n_causal == 1 && d->fw_causal == 2 && d->fw == 2 && d->Cr == 32 && d->Cs == 256 &&
          d->n_head == 1 && d->head_channels[0] == 256 && d->head_channels[1] == 256 &&
          d->n_blocks * d->n_layers <= 128))
        return false;
    if (d->causal_b && d->causal_b[0]) return false;
    if (d->frame_bias && !rows) return false;      // a frame table selects the any-shape decoder, as biased layers do
    for (int l = 0; l < d->n_layers; ++l)
        if (d->cd[l] != 32) return false;
    for (int j = 0; j < d->n_blocks * d->n_layers; ++j)
        if ((!rows && ((d->bf && d->bf[j]) || (d->bg && d->bg[j]))) || (d->bp && d->bp[j]) || (d->bs && d->bs[j])) return false;
    return true;
}

// the handle's sampling controls as the kernels take them: whatever is off has its "skip" value (top_k >= Q keeps every
// token, so it is off: the all-off launch runs the instruction stream it ran before the controls existed)
static SampleCtl launch_ctl(const Decoder* D) {
    SampleCtl c = D->ctl;
    if (c.top_k >= D->meta.Q) c.top_k = 0;
    return c;
}

// ---- packing ---------------------------------------------------------------------------------
// dst[(k*Cin + c)*ostride + ooff + o] = src[(o*Cin + c)*fw + k]
__global__ void k_pack_conv_T(const float* __restrict__ src, float* __restrict__ dst, int Cout, int Cin, int fw,
                              int ostride, int ooff) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Cout * Cin * fw) return;
    int k = i % fw;
    int c = (i / fw) % Cin;
    int o = i / (fw * Cin);
    dst[((long long)k * Cin + c) * ostride + ooff + o] = src[i];
}
// first causal layer: dst[(q*fw + k)*C + c] = src[(c*Q + q)*fw + k]
__global__ void k_pack_embed(const float* __restrict__ src, float* __restrict__ dst, int C, int Q, int fw) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * Q * fw) return;
    int k = i % fw;
    int q = (i / fw) % Q;
    int c = i / (fw * Q);
    dst[((long long)q * fw + k) * C + c] = src[i];
}
__global__ void k_copy_off(const float* __restrict__ src, float* __restrict__ dst, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}
// ring[(col mod D)*C + c] = src[col*C + c] for col in [W-D, W) (zero where col < 0)
__global__ void k_load_ring(const float* __restrict__ src, float* __restrict__ ring, int W, int D, int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= D * C) return;
    int c = i % C;
    int m = i / C;                       // 0 .. D-1: column W-D+m
    long long col = (long long)W - D + m;
    float v = col >= 0 ? src[col * C + c] : 0.f;
    long long slot = ((col % D) + D) % D;
    ring[slot * C + c] = v;
}
__global__ void k_load_tok_ring(const int32_t* __restrict__ tokens, int* __restrict__ ring, int W, int D) {
    int m = threadIdx.x;
    if (m >= D) return;
    long long col = (long long)W - D + m;
    long long slot = ((col % D) + D) % D;
    ring[slot] = col >= 0 ? tokens[col] : 0;
}

// ---- the step loop ---------------------------------------------------------------------------
// (DecFrames, the frame table of one utterance as a step loop takes it: decoder_types.hpp)
// (DecAnyUtt, one utterance as the any-shape kernels take it: decoder_types.hpp)
__device__ __forceinline__ int pmod(long long a, int D) {
    long long r = a % D;
    return (int)(r < 0 ? r + D : r);
}
__device__ __forceinline__ float block_reduce(float v, bool is_max, float* red) {
    for (int o = 32; o > 0; o >>= 1) {
        float w = __shfl_xor(v, o);
        v = is_max ? fmaxf(v, w) : v + w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
    return r;
}
// The step loop of one utterance on one workgroup: k_decode runs it for its handle, workgroup u of k_decode_batch for
// utterance u.  Everything it touches -- arena, token ring, uniforms, outputs -- is the utterance's own; `sc` and the flags
// are the same for every thread of the workgroup.
// FORCED (WN_DECODER_FORCED_TOKENS handles): a step may emit the token out_tokens[it] holds instead of drawing; without it the
// loop is what it was
// RING (WN_DECODER_FRAME_RING handles): the table is a ring of fr.ring rows -- the step's row is a walked slot that wraps, not a
// quotient per step; without it the loop is what it was
template <bool LERP, bool FORCED, bool RING>         // LERP: the table is interpolated (DecFrames.interp); without it the loop is what it was
__device__ __forceinline__ void decode_steps(
    const DecMeta& M, const DecCausal* __restrict__ causal, const DecLayer* __restrict__ layers,
    const DecHead* __restrict__ heads, float* __restrict__ arena, int* __restrict__ tok_ring, long long n0,
    int nsteps, int first_token, const double* __restrict__ uniforms, int32_t* __restrict__ out_tokens,
    float* __restrict__ prob_out, int prob_stride, int apply_softmax, int do_sample, const SampleCtl& sc, const DecFrames& fr) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, NT = blockDim.x;
    const bool filt = sc.top_k > 0 || sc.top_p < 1.0;      // workgroup-uniform: kernel arguments, or the workgroup's own table entry
    float* xcur = sm;                    // [maxc] current column of the residual stream / causal stack
    float* xnew = xcur + M.maxc;         // [maxc]
    float* ab = xnew + M.maxc;           // [2*maxc] gate pre-activations
    float* zz = ab + 2 * M.maxc;         // [maxc]
    float* skip = zz + M.maxc;           // [maxc]
    float* hbuf = skip + M.maxc;         // [maxc]
    float* red = hbuf + M.maxc;          // [16]
    __shared__ int s_token;
    if (tid == 0) s_token = first_token;
    __syncthreads();
    // RING: slot = (pos0 / hop) mod ring and p % hop of the first step once, then one increment per step (workgroup-uniform)
    int rslot = 0, rrem = 0;
    if (RING && fr.tab) {
        const long long j = fr.pos0 / fr.hop;
        rslot = (int)(j % fr.ring);
        rrem = (int)(fr.pos0 - j * fr.hop);
    }

    for (int it = 0; it < nsteps; ++it) {
        const long long n = n0 + it;
        const int token = s_token;
        // FORCED: the entry this step may have to emit, read by every thread ahead of the network (one address for all: uniform) --
        // thread 0 writes out_tokens[it] only at the draw below; unsigned compare: a garbage entry is no index
        const int f_tok = FORCED && do_sample ? __builtin_amdgcn_readfirstlane(out_tokens[it]) : -1;
        const bool given = FORCED && (unsigned)f_tok < (unsigned)M.Q;
        // ---- causal layer 0: two (fwc) gathered rows of the packed table ---------------------
        {
            const DecCausal L = causal[0];
            const int Dc = M.fwc - 1;
            for (int c = tid; c < L.cout; c += NT) {
                float acc = L.b >= 0 ? arena[L.b + c] : 0.f;
                for (int k = 0; k < M.fwc; ++k) {
                    int m = M.fwc - 1 - k;      // age of the tap
                    int q = m == 0 ? token : tok_ring[pmod(n - m, Dc)];
                    acc += arena[L.w + ((long long)q * M.fwc + k) * L.cout + c];
                }
                xcur[c] = acc;
            }
            __syncthreads();
            if (tid == 0 && Dc > 0) tok_ring[pmod(n, Dc)] = token;
        }
        // ---- further causal layers (d = 1), generic ------------------------------------------
        for (int i = 1; i < M.ncausal; ++i) {
            const DecCausal L = causal[i];
            const int Dc = M.fwc - 1;
            for (int o = tid; o < L.cout; o += NT) {
                float acc = L.b >= 0 ? arena[L.b + o] : 0.f;
                for (int k = 0; k < M.fwc; ++k) {
                    int m = M.fwc - 1 - k;
                    const float* src = m == 0 ? nullptr : arena + L.ring + (long long)pmod(n - m, Dc) * L.cin;
                    for (int c = 0; c < L.cin; ++c) {
                        float xv = m == 0 ? xcur[c] : src[c];
                        acc += arena[L.w + ((long long)k * L.cin + c) * L.cout + o] * xv;
                    }
                }
                xnew[o] = acc;
            }
            __syncthreads();
            if (Dc > 0)
                for (int c = tid; c < L.cin; c += NT) arena[L.ring + (long long)pmod(n, Dc) * L.cin + c] = xcur[c];
            __syncthreads();
            for (int o = tid; o < L.cout; o += NT) xcur[o] = xnew[o];
            __syncthreads();
        }
        for (int o = tid; o < M.Cs; o += NT) skip[o] = 0.f;
        // the step's frame row, computed once per step (workgroup-uniform); layer j's 2 cd values lie at the running offset
        const float* __restrict__ frow = !fr.tab ? nullptr
                                         : RING ? fr.tab + rslot * (long long)fr.row
                                                : fr.tab + ((fr.pos0 + it) / fr.hop) * (long long)fr.row;
        // linear interpolation: the next row and its weight, likewise once per step (ring: the row after slot ring - 1 is slot 0)
        const float* __restrict__ fnext = !(LERP && frow) ? nullptr : RING && rslot + 1 == fr.ring ? fr.tab : frow + fr.row;
        const float falpha = fnext ? __fdiv_rn(RING ? (float)rrem : (float)(int)((fr.pos0 + it) % fr.hop), (float)fr.hop) : 0.f;
        if (RING && ++rrem == fr.hop) {          // the walk, for the next step
            rrem = 0;
            if (++rslot == fr.ring) rslot = 0;
        }
        // ---- residual layers ------------------------------------------------------------------
        for (int j = 0; j < M.nlayers; ++j) {
            const DecLayer L = layers[j];
            const int D = (M.fw - 1) * L.d;
            const int n2 = 2 * L.cd;
            // gate: ab[o2] = b + sum_k sum_c WfgT[k*Cr+c][o2] x[n-(fw-1-k)d][c]
            for (int o = tid; o < n2; o += NT) {
                float acc = L.bfg >= 0 ? arena[L.bfg + o] : 0.f;
                // (static bias or 0) + frame value, then the taps: a table of zeros changes no bit
                if (LERP && fnext) acc += bias_lerp(frow[o], fnext[o], falpha);
                else if (frow) acc += frow[o];
                for (int k = 0; k < M.fw; ++k) {
                    int m = M.fw - 1 - k;
                    const float* w = arena + L.wfg + (long long)k * M.Cr * n2 + o;
                    if (m == 0) {
                        for (int c = 0; c < M.Cr; ++c) acc += w[(long long)c * n2] * xcur[c];
                    } else {
                        const float* src = arena + L.ring + (long long)pmod(n - (long long)m * L.d, D) * M.Cr;
                        for (int c = 0; c < M.Cr; ++c) acc += w[(long long)c * n2] * src[c];
                    }
                }
                ab[o] = acc;
            }
            __syncthreads();
            for (int o = tid; o < L.cd; o += NT) zz[o] = fast_tanh(ab[o]) * fast_sigmoid(ab[L.cd + o]);
            // the ring slot of column n is the one that held column n-(fw-1)d: all reads are done
            if (D > 0)
                for (int c = tid; c < M.Cr; c += NT) arena[L.ring + (long long)pmod(n, D) * M.Cr + c] = xcur[c];
            __syncthreads();
            // projections: rows [0,Cr) residual, rows [Cr,Cr+Cs) skip
            const int no = M.Cr + M.Cs;
            for (int o = tid; o < no; o += NT) {
                float acc = L.bps >= 0 ? arena[L.bps + o] : 0.f;
                const float* w = arena + L.wps + o;
                for (int c = 0; c < L.cd; ++c) acc += w[(long long)c * no] * zz[c];
                if (o < M.Cr) xnew[o] = acc + xcur[o];
                else skip[o - M.Cr] += acc;
            }
            __syncthreads();
            for (int c = tid; c < M.Cr; c += NT) xcur[c] = xnew[c];
            __syncthreads();
            if (frow) frow += n2;
            if (LERP && fnext) fnext += n2;
        }
        // ---- head on the newest column only ---------------------------------------------------
        float* hin = skip;
        float* hout = hbuf;
        for (int i = 0; i < M.nhead; ++i) {
            const DecHead H = heads[i];
            for (int o = tid; o < H.cout; o += NT) {
                float acc = H.b >= 0 ? arena[H.b + o] : 0.f;
                const float* w = arena + H.w + o;
                for (int c = 0; c < H.cin; ++c) acc += w[(long long)c * H.cout] * act_apply(hin[c], M.head_act);
                hout[o] = acc;
            }
            __syncthreads();
            float* t = hin; hin = hout; hout = t;
        }
        // hin holds the Q logits
        if (apply_softmax) {
            // temperature: the fp32 logits times 1/T (a thread only ever touches its own entries up to the barrier below)
            if (sc.inv_temp != 1.f)
                for (int q = tid; q < M.Q; q += NT) hin[q] *= sc.inv_temp;
            float m = -INFINITY;
            for (int q = tid; q < M.Q; q += NT) m = fmaxf(m, hin[q]);
            m = block_reduce(m, true, red);
            float s = 0.f;
            for (int q = tid; q < M.Q; q += NT) s += expf(hin[q] - m);
            s = block_reduce(s, false, red);
            float inv = 1.f / s;
            __syncthreads();
            for (int q = tid; q < M.Q; q += NT) hin[q] = expf(hin[q] - m) * inv;
            __syncthreads();
        }
        if (prob_out && prob_stride)          // the full row; prob_stride == 0 (kProbChosen): one float per step, at the draw below
            for (int q = tid; q < M.Q; q += NT) prob_out[(long long)it * prob_stride + q] = hin[q];
        if (do_sample && given) {
            // a given step: no filter, no draw; out_tokens[it] holds the token already, and it enters the next step as a drawn one
            if (tid == 0) {
                s_token = f_tok;
                if (prob_out && !prob_stride) prob_out[it] = hin[f_tok];     // the untruncated row's entry, nothing clamped
            }
        } else if (do_sample) {
            if (filt)                    // top-k / top-p: the trace above holds the row as the filter receives it
                sample_filter<false>(hin, M.Q, tid, NT, sc.top_k, sc.top_p);
            if (tid == 0) {
                // numpy legacy choice: float64 cumsum, divide by the total, first index with cdf > u
                double tot = 0.0;
                for (int q = 0; q < M.Q; ++q) tot += (double)hin[q];
                double c = 0.0, u = uniforms[it];
                int idx = M.Q;
                for (int q = 0; q < M.Q; ++q) {
                    c += (double)hin[q];
                    if (c / tot > u) { idx = q; break; }
                }
                if (idx >= M.Q) idx = M.Q - 1;
                s_token = idx;
                out_tokens[it] = idx;
                // WN_DECODER_TRACE_CHOSEN: the drawn token's entry of the row the draw consumed (the filter leaves a kept entry
                // as it was, and a drawn token is a kept one); nothing clamped
                if (prob_out && !prob_stride) prob_out[it] = hin[idx];
            }
        }
        __syncthreads();
    }
}

template <bool LERP, bool FORCED, bool RING>
__global__ __launch_bounds__(kDecThreads) void k_decode(
    DecMeta M, const DecCausal* __restrict__ causal, const DecLayer* __restrict__ layers,
    const DecHead* __restrict__ heads, float* __restrict__ arena, int* __restrict__ tok_ring, long long n0,
    int nsteps, int first_token, const double* __restrict__ uniforms, int32_t* __restrict__ out_tokens,
    float* __restrict__ prob_out, int prob_stride, int apply_softmax, int do_sample, const SampleCtl sc, const DecFrames fr) {
    decode_steps<LERP, FORCED, RING>(M, causal, layers, heads, arena, tok_ring, n0, nsteps, first_token, uniforms, out_tokens, prob_out, prob_stride,
                 apply_softmax, do_sample, sc, fr);
}

// wn_decoder_run_batch on any-shape handles: workgroup u is utterance u's k_decode.  The workgroups share nothing and
// never wait for each other, so any number of them may be queued behind the CUs -- and each runs its utterance's own step
// count (DecAnyUtt.nsteps; the launch has no count of its own): an utterance that ends early simply ends.  prob_stride is the
// launch's (M.Q, or kProbChosen when the handles were created with WN_DECODER_TRACE_CHOSEN: they must agree), and so is FORCED
// (the handles agree on WN_DECODER_FORCED_TOKENS), and RING (they agree on WN_DECODER_FRAME_RING).
template <bool LERP, bool FORCED, bool RING>
__global__ __launch_bounds__(kDecThreads) void k_decode_batch(DecMeta M, const DecAnyUtt* __restrict__ tab, int n_utt, int prob_stride) {
    if ((int)blockIdx.x >= n_utt) return;
    const DecAnyUtt q = tab[blockIdx.x];
    decode_steps<LERP, FORCED, RING>(M, q.causal, q.layers, q.heads, q.arena, q.tok_ring, q.n0, q.nsteps, q.first_token, q.uniforms, q.out_tokens,
                 q.prob_out, prob_stride, 1, 1, q.sc, q.fr);
}

// ---- host side -------------------------------------------------------------------------------
static int validate(const WnDecoderDesc* d) {
    WN_CHECK_ARG(d, "decoder: desc is NULL");
    WN_CHECK_ARG(d->Q > 0 && d->fw_causal > 0 && d->n_causal > 0 && d->fw > 0 && d->n_blocks > 0 &&
                     d->n_layers > 0 && d->Cr > 0 && d->Cs > 0 && d->n_head > 0,
                 "decoder: non-positive size in desc");
    WN_CHECK_ARG(d->causal_channels && d->cd && d->head_channels && d->causal_W && d->Wf && d->Wg && d->Wp &&
                     d->Ws && d->head_W,
                 "decoder: NULL table in desc");
    WN_CHECK_ARG(d->causal_channels[d->n_causal - 1] == d->Cr, "decoder: last causal width != Cr");
    WN_CHECK_ARG(d->head_channels[0] == d->Cs && d->head_channels[d->n_head] == d->Q,
                 "decoder: head channels must run Cs ... Q");
    WN_CHECK_ARG(d->head_act == WN_ACT_RELU || d->head_act == WN_ACT_ELU || d->head_act == WN_ACT_NONE,
                 "decoder: bad head_act");
    WN_CHECK_ARG(d->step_limit >= 0, "decoder: step_limit = %d is negative (0: no limit)", d->step_limit);
    return WN_OK;
}

static inline long long align64(long long x) { return (x + 63) & ~63ll; }

// ---- local conditioning: the handle's frame table ----------------------------------------------
static DecFrames launch_frames(const Decoder* D) {
    const FrameTable& F = D->frames;
    DecFrames f{};
    if (F.n > 0) { f.tab = F.tab; f.hop = F.hop; f.row = F.row; f.pos0 = F.phase + D->since_set; f.interp = F.interp; }
    if (F.n > 0 && D->frame_ring) { f.tab = F.ring; f.ring = F.n; }       // (F.row is the caller's stride)
    return f;
}
static bool lerp_table(const Decoder* D) { return D->frames.n > 0 && D->frames.interp != 0; }   // the LERP kernels
static int row_width(const Decoder* D) {           // floats of one table row: the sum of 2 cd over the layers
    int row = 0;
    for (const DecLayer& L : D->layers) row += 2 * L.cd;
    return row;
}
// n more steps must not read past row frames.n - 1 (refused before any device work; no clamping)
static int check_frames(const char* fn, const Decoder* D, long long n) {
    const FrameTable& F = D->frames;
    if (F.n <= 0) return WN_OK;
    if (D->frame_ring) {
        // a ring: which frames it holds is the caller's business; a launch cannot be refilled while it runs, so the frames of
        // its steps -- the first step's to the last step's, one more under linear interpolation -- must fit the ring at once
        const long long p0 = F.phase + D->since_set;
        const long long reads = (p0 + n - 1) / F.hop - p0 / F.hop + 1 + (F.interp ? 1 : 0);
        WN_CHECK_ARG(reads <= F.n, "%s: %lld more steps read %lld frames of a ring of %d rows (WN_DECODER_FRAME_RING; hop %d, phase %d, "
                                   "%lld steps run on it%s): a launch cannot be refilled while it runs", fn, n, reads, F.n, F.hop,
                     F.phase, D->since_set, F.interp ? "; linear interpolation reads the frame after the step's own" : "");
        return WN_OK;
    }
    // (linear interpolation: the last step reads row j + 1 as well)
    const long long last = (F.phase + D->since_set + n - 1) / F.hop + (F.interp ? 1 : 0);
    WN_CHECK_ARG(last < F.n, "%s: %lld more steps would read row %lld of a frame table of %d rows (hop %d, phase %d, %lld steps "
                             "run on it%s)", fn, n, last, F.n, F.hop, F.phase, D->since_set,
                 F.interp ? "; linear interpolation reads the row after the step's own" : "");
    return WN_OK;
}
static int check_frame_desc(const Decoder* D, const WnDecoderDesc* d) {
    const bool ring = (d->flags & WN_DECODER_FRAME_RING) != 0;
    WN_CHECK_ARG(!ring || d->frame_bias, "decoder: WN_DECODER_FRAME_RING without frame_bias: the flag makes frame_bias a ring of "
                                         "n_frames rows read in place");
    // the kernels read a row one float per lane / thread: 4-byte reads.  frame_stride counts floats, so every row of an aligned
    // ring is aligned
    WN_CHECK_ARG(!ring || (uintptr_t)d->frame_bias % sizeof(float) == 0, "decoder: WN_DECODER_FRAME_RING: frame_bias = %p is not a "
                 "multiple of 4 bytes (sizeof(float)), the alignment the kernels' row reads need", (const void*)d->frame_bias);
    if (!d->frame_bias) return WN_OK;
    const int row = row_width(D);
    WN_CHECK_ARG(d->n_frames > 0 && d->frame_hop > 0, "decoder: a frame table needs n_frames > 0 and frame_hop > 0 (got %d, %d)",
                 d->n_frames, d->frame_hop);
    WN_CHECK_ARG(d->frame_phase >= 0 && d->frame_phase < d->frame_hop, "decoder: frame_phase = %d outside [0, frame_hop = %d)",
                 d->frame_phase, d->frame_hop);
    WN_CHECK_ARG(d->frame_interp == 0 || d->frame_interp == 1, "decoder: frame_interp = %d is neither 0 (repeat) nor 1 (linear)",
                 d->frame_interp);
    WN_CHECK_ARG(d->frame_stride >= row, "decoder: frame_stride = %d below the row width %d (sum of 2 cd over the layers)",
                 d->frame_stride, row);
    WN_CHECK_ARG(!D->fastP || D->gate_rows, "decoder: this handle runs the specialised 32/256-channel kernels, which take no frame table: create the "
                            "handle with the table");
    return WN_OK;
}
// copy the table (after check_frame_desc), or drop it when the description has none, and take the step limit; the step count
// that both are measured against starts again, with or without a table
static int take_frames(Decoder* D, const WnDecoderDesc* d, hipStream_t s) {
    D->since_set = 0;
    D->step_limit = d->step_limit;
    FrameTable& F = D->frames;
    if (!d->frame_bias) { F.n = 0; return WN_OK; }
    if (D->frame_ring) {                  // by reference: the pointer, the stride and R; nothing is copied, nothing launched
        F.ring = d->frame_bias;
        F.n = d->n_frames; F.hop = d->frame_hop; F.phase = d->frame_phase; F.row = d->frame_stride; F.interp = d->frame_interp;
        return WN_OK;
    }
    const int row = row_width(D);
    if (d->n_frames > F.cap || row != F.row) {
        if (F.tab) { WN_HIP(hipFree(F.tab)); F.tab = nullptr; F.cap = 0; }
        WN_HIP(hipMalloc(&F.tab, (size_t)d->n_frames * row * sizeof(float)));
        F.cap = d->n_frames;
    }
    WN_HIP(hipMemcpy2DAsync(F.tab, (size_t)row * sizeof(float), d->frame_bias, (size_t)d->frame_stride * sizeof(float),
                            (size_t)row * sizeof(float), (size_t)d->n_frames, hipMemcpyDeviceToDevice, s));
    F.n = d->n_frames; F.hop = d->frame_hop; F.phase = d->frame_phase; F.row = row; F.interp = d->frame_interp;
    return WN_OK;
}

// one utterance's launch arguments of the specialised kernels (decoder_fast.hip), from its handle
// a WN_DECODER_GATE_ROWS handle that holds something to add: static gate biases or a table (else the launch is the plain one)
static bool gate_launch(const Decoder* D) {
    if (!D->gate_rows) return false;
    return D->frames.n > 0 || D->gate_bias;
}
static DecUtt fast_utt(const Decoder* D, int first_token, const double* uniforms, int32_t* out_tokens, float* prob_out,
                       const SampleCtl& sc) {
    DecUtt q{};
    q.P = D->fastP; q.hbias = D->head_bias_off >= 0 ? D->arena + D->head_bias_off : nullptr;
    q.E = D->arena + D->causal[0].w; q.layers = D->d_layers; q.arena = D->arena; q.tok_ring = D->tok_ring; q.n0 = D->step;
    q.uniforms = uniforms; q.out_tokens = out_tokens; q.prob_out = prob_out; q.first_token = first_token; q.sc = sc;
    if (D->gate_rows) q.fr = launch_frames(D);
    return q;
}
// ... and of the any-shape kernels
static DecAnyUtt any_utt(const Decoder* D, int first_token, const double* uniforms, int32_t* out_tokens, float* prob_out,
                         int nsteps, const SampleCtl& sc) {
    DecAnyUtt q{};
    q.causal = D->d_causal; q.layers = D->d_layers; q.heads = D->d_heads; q.arena = D->arena; q.tok_ring = D->tok_ring;
    q.n0 = D->step; q.uniforms = uniforms; q.out_tokens = out_tokens; q.prob_out = prob_out;
    q.first_token = first_token; q.nsteps = nsteps; q.sc = sc; q.fr = launch_frames(D);
    return q;
}

// before the first pack launch: a refused wn_decoder_update_weights leaves the handle as it was
static int check_weight_ptrs(const Decoder* D, const WnDecoderDesc* d) {
    for (int i = 0; i < d->n_causal; ++i) WN_CHECK_ARG(d->causal_W[i], "decoder: causal_W[%d] NULL", i);
    for (int j = 0; j < (int)D->layers.size(); ++j)
        WN_CHECK_ARG(d->Wf[j] && d->Wg[j] && d->Wp[j] && d->Ws[j], "decoder: layer %d has a NULL weight", j);
    for (int i = 0; i < d->n_head; ++i) WN_CHECK_ARG(d->head_W[i], "decoder: head_W[%d] NULL", i);
    return WN_OK;
}

static int pack_weights(Decoder* D, const WnDecoderDesc* d, hipStream_t s) {
    const int T = 256;
    {   // FNV-1a over every weight / bias pointer of the description, in a fixed order
        // (h: src_key; t: tile_key, the same walk without the gate-bias pointers)
        unsigned long long h = 1469598103934665603ull, t = h;
        auto mix1 = [](unsigned long long& k, const void* p) { k = (k ^ (unsigned long long)(uintptr_t)p) * 1099511628211ull; };
        auto mix = [&](const void* p) { mix1(h, p); mix1(t, p); };
        for (int i = 0; i < d->n_causal; ++i) { mix(d->causal_W[i]); mix(d->causal_b ? d->causal_b[i] : nullptr); }
        for (int j = 0; j < (int)D->layers.size(); ++j) {
            mix(d->Wf[j]); mix(d->Wg[j]); mix(d->Wp[j]); mix(d->Ws[j]);
            // (a WN_DECODER_GATE_ROWS handle keeps its gate biases out of the packed weights that same_weights shares: handles of
            // one model holding different classes' biases still carry one key)
            if (!D->gate_rows) { mix1(h, d->bf ? d->bf[j] : nullptr); mix1(h, d->bg ? d->bg[j] : nullptr); }
            mix(d->bp ? d->bp[j] : nullptr); mix(d->bs ? d->bs[j] : nullptr);
        }
        for (int i = 0; i < d->n_head; ++i) { mix(d->head_W[i]); mix(d->head_b ? d->head_b[i] : nullptr); }
        D->src_key = h;
        D->tile_key = t;
    }
    for (int i = 0; i < d->n_causal; ++i) {
        const DecCausal& L = D->causal[i];
        int n = L.cout * L.cin * d->fw_causal;
        if (i == 0)
            hipLaunchKernelGGL(k_pack_embed, dim3(cdiv(n, T)), dim3(T), 0, s, d->causal_W[i], D->arena + L.w, L.cout,
                               L.cin, d->fw_causal);
        else
            hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(n, T)), dim3(T), 0, s, d->causal_W[i], D->arena + L.w,
                               L.cout, L.cin, d->fw_causal, L.cout, 0);
        if (L.b >= 0)
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(L.cout, T)), dim3(T), 0, s, d->causal_b[i], D->arena + L.b,
                               L.cout);
    }
    D->gate_bias = false;
    for (int j = 0; j < (int)D->layers.size(); ++j) {
        const DecLayer& L = D->layers[j];
        int cd = L.cd, Cr = d->Cr, Cs = d->Cs;
        int n = cd * Cr * d->fw;
        hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(n, T)), dim3(T), 0, s, d->Wf[j], D->arena + L.wfg, cd, Cr, d->fw,
                           2 * cd, 0);
        hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(n, T)), dim3(T), 0, s, d->Wg[j], D->arena + L.wfg, cd, Cr, d->fw,
                           2 * cd, cd);
        hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(Cr * cd, T)), dim3(T), 0, s, d->Wp[j], D->arena + L.wps, Cr, cd, 1,
                           Cr + Cs, 0);
        hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(Cs * cd, T)), dim3(T), 0, s, d->Ws[j], D->arena + L.wps, Cs, cd, 1,
                           Cr + Cs, Cr);
        if (L.bfg >= 0 && d->bf && d->bf[j]) {
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(cd, T)), dim3(T), 0, s, d->bf[j], D->arena + L.bfg, cd);
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(cd, T)), dim3(T), 0, s, d->bg[j], D->arena + L.bfg + cd, cd);
            D->gate_bias = true;
        } else if (L.bfg >= 0) {           // a WN_DECODER_GATE_ROWS handle (every layer has room) given no bias for this layer: 0
            WN_HIP(hipMemsetAsync(D->arena + L.bfg, 0, 2 * (size_t)cd * sizeof(float), s));
        }
        if (L.bps >= 0) {
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(Cr, T)), dim3(T), 0, s, d->bp[j], D->arena + L.bps, Cr);
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(Cs, T)), dim3(T), 0, s, d->bs[j], D->arena + L.bps + Cr, Cs);
        }
    }
    for (int i = 0; i < d->n_head; ++i) {
        const DecHead& H = D->heads[i];
        hipLaunchKernelGGL(k_pack_conv_T, dim3(cdiv(H.cin * H.cout, T)), dim3(T), 0, s, d->head_W[i], D->arena + H.w,
                           H.cout, H.cin, 1, H.cout, 0);
        if (H.b >= 0)
            hipLaunchKernelGGL(k_copy_off, dim3(cdiv(H.cout, T)), dim3(T), 0, s, d->head_b[i], D->arena + H.b, H.cout);
    }
    WN_LAUNCH_CHECK();
    if (D->fastP) return decode_fast_pack(d, D->fastP, s);
    return WN_OK;
}

// wn_decoder_create, first half: meta, the three host tables, arena_floats and lds_bytes.  Host arithmetic only.
static int lay_out(Decoder* D, const WnDecoderDesc* d) {
    DecMeta& M = D->meta;
    M.Q = d->Q; M.fwc = d->fw_causal; M.ncausal = d->n_causal; M.fw = d->fw;
    M.nlayers = d->n_blocks * d->n_layers; M.Cr = d->Cr; M.Cs = d->Cs; M.nhead = d->n_head;
    M.head_act = d->head_act;
    long long off = 0;
    // a WN_DECODER_GATE_ROWS handle of the specialised shape keeps room for every layer's gate biases, given or not: an update
    // may bring biases to a handle created without them (and the other way round)
    const bool rows = (d->flags & WN_DECODER_GATE_ROWS) && fast_shape(d);
    int maxc = d->Q > d->Cs ? d->Q : d->Cs;
    if (d->Cr > maxc) maxc = d->Cr;
    int cin = d->Q;
    for (int i = 0; i < d->n_causal; ++i) {
        DecCausal L{};
        L.cin = cin; L.cout = d->causal_channels[i];
        if (L.cout > maxc) maxc = L.cout;
        L.w = (int)off; off = align64(off + (long long)L.cin * L.cout * d->fw_causal);
        bool hb = d->causal_b && d->causal_b[i];
        L.b = hb ? (int)off : -1; if (hb) off = align64(off + L.cout);
        L.ring = (int)off;
        if (i > 0) off = align64(off + (long long)(d->fw_causal - 1) * L.cin);
        D->causal.push_back(L);
        cin = L.cout;
    }
    for (int b = 0; b < d->n_blocks; ++b) {
        int dil = 1;
        for (int l = 0; l < d->n_layers; ++l) {
            int j = b * d->n_layers + l;
            DecLayer L{};
            L.cd = d->cd[l]; L.d = dil;
            if (L.cd > maxc) maxc = L.cd;
            L.wfg = (int)off; off = align64(off + (long long)d->fw * d->Cr * 2 * L.cd);
            bool hb = d->bf && d->bf[j];
            WN_CHECK_ARG(hb == (d->bg && d->bg[j]), "decoder: bf/bg must both be present or absent");
            L.bfg = hb || rows ? (int)off : -1; if (hb || rows) off = align64(off + 2 * L.cd);
            L.wps = (int)off; off = align64(off + (long long)L.cd * (d->Cr + d->Cs));
            bool hp = d->bp && d->bp[j];
            WN_CHECK_ARG(hp == (d->bs && d->bs[j]), "decoder: bp/bs must both be present or absent");
            L.bps = hp ? (int)off : -1; if (hp) off = align64(off + d->Cr + d->Cs);
            L.ring = (int)off; off = align64(off + (long long)(d->fw - 1) * dil * d->Cr);
            D->layers.push_back(L);
            dil *= d->fw;
        }
    }
    for (int i = 0; i < d->n_head; ++i) {
        DecHead H{};
        H.cin = d->head_channels[i]; H.cout = d->head_channels[i + 1];
        if (H.cout > maxc) maxc = H.cout;
        H.w = (int)off; off = align64(off + (long long)H.cin * H.cout);
        bool hb = d->head_b && d->head_b[i];
        H.b = hb ? (int)off : -1; if (hb) off = align64(off + H.cout);
        D->heads.push_back(H);
    }
    WN_CHECK_SHAPE(off < (1ll << 31), "decoder: arena too large");
    M.maxc = maxc;
    D->arena_floats = off;
    D->lds_bytes = (size_t)(7 * maxc + 16) * sizeof(float);
    WN_CHECK_SHAPE(D->lds_bytes <= 150 * 1024, "decoder: channel width %d too large", maxc);
    return WN_OK;
}

// dynamic LDS of a tile of U utterances: U x decode_steps' (7 maxc + 16) floats.  (k_decode_tile's own U slot records are
// static LDS on top: 2.2 KB at U = 16, inside what the 150 KiB bound leaves of a CU's 160 KiB.)
static size_t tile_lds(const Decoder* D, int U) { return (size_t)U * (7 * (size_t)D->meta.maxc + 16) * sizeof(float); }
static constexpr size_t kDecLdsMax = 150 * 1024;

}  // namespace wn

using namespace wn;

extern "C" {

int wn_decoder_create(void** handle, const WnDecoderDesc* d, void* stream) {
    WN_CHECK_ARG(handle, "wn_decoder_create: handle is NULL");
    int rc = validate(d);
    if (rc) return rc;
    // a handle that is not handed out is destroyed, with whatever it holds by then
    std::unique_ptr<Decoder, int (*)(void*)> built(new (std::nothrow) Decoder(), wn_decoder_destroy);
    Decoder* D = built.get();
    WN_CHECK_ARG(D, "wn_decoder_create: out of host memory");
    if ((rc = lay_out(D, d))) return rc;
    if ((rc = check_frame_desc(D, d))) return rc;
    if ((rc = check_weight_ptrs(D, d))) return rc;
    // second half: the device memory, zeroed, and the device copies of the three tables
    hipStream_t s = as_stream(stream);
    const size_t ring = sizeof(int) * (d->fw_causal > 1 ? d->fw_causal - 1 : 1);
    const size_t nc = D->causal.size() * sizeof(DecCausal), nl = D->layers.size() * sizeof(DecLayer), nh = D->heads.size() * sizeof(DecHead);
    WN_HIP(hipMalloc(&D->arena, (size_t)D->arena_floats * sizeof(float)));
    WN_HIP(hipMemsetAsync(D->arena, 0, (size_t)D->arena_floats * sizeof(float), s));
    WN_HIP(hipMalloc(&D->tok_ring, ring));
    WN_HIP(hipMemsetAsync(D->tok_ring, 0, ring, s));
    WN_HIP(hipMalloc(&D->dmeta, nc + nl + nh));
    D->d_causal = (DecCausal*)D->dmeta;
    D->d_layers = (DecLayer*)((char*)D->dmeta + nc);
    D->d_heads = (DecHead*)((char*)D->dmeta + nc + nl);
    WN_HIP(hipMemcpyAsync(D->d_causal, D->causal.data(), nc, hipMemcpyHostToDevice, s));
    WN_HIP(hipMemcpyAsync(D->d_layers, D->layers.data(), nl, hipMemcpyHostToDevice, s));
    WN_HIP(hipMemcpyAsync(D->d_heads, D->heads.data(), nh, hipMemcpyHostToDevice, s));
    WN_HIP(hipStreamSynchronize(s));      // the host vectors above must outlive the copies
    if (fast_shape(d)) {
        WN_HIP(hipMalloc(&D->fastP, decode_fast_pack_floats(D->meta.nlayers) * sizeof(float)));
        D->head_bias_off = D->heads[0].b;
        D->three_wgs = !(d->flags & WN_DECODER_ONE_WORKGROUP);
        D->gate_rows = (d->flags & WN_DECODER_GATE_ROWS) != 0;
    }
    D->trace_chosen = (d->flags & WN_DECODER_TRACE_CHOSEN) != 0;
    D->forced = (d->flags & WN_DECODER_FORCED_TOKENS) != 0;
    D->frame_ring = (d->flags & WN_DECODER_FRAME_RING) != 0;
    if ((rc = pack_weights(D, d, s))) return rc;
    if ((rc = take_frames(D, d, s))) return rc;
    *handle = built.release();
    return WN_OK;
}

int wn_decoder_destroy(void* handle) {
    Decoder* D = (Decoder*)handle;
    if (!D) return WN_OK;
    if (D->arena) (void)hipFree(D->arena);
    if (D->fastP) (void)hipFree(D->fastP);
    if (D->tok_ring) (void)hipFree(D->tok_ring);
    if (D->dmeta) (void)hipFree(D->dmeta);
    if (D->frames.tab) (void)hipFree(D->frames.tab);
    if (D->batch_tab) (void)hipFree(D->batch_tab);
    if (D->batch_img) (void)hipHostFree(D->batch_img);
    if (D->batch_copied) (void)hipEventDestroy(D->batch_copied);
    delete D;
    return WN_OK;
}

int wn_decoder_update_weights(void* handle, const WnDecoderDesc* d, void* stream) {
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D, "wn_decoder_update_weights: NULL handle");
    int rc = validate(d);
    if (rc) return rc;
    WN_CHECK_ARG(d->n_blocks * d->n_layers == D->meta.nlayers && d->Cr == D->meta.Cr && d->Cs == D->meta.Cs &&
                     d->Q == D->meta.Q && d->n_causal == D->meta.ncausal && d->n_head == D->meta.nhead,
                 "wn_decoder_update_weights: topology differs from the handle's");
    // a handle's form is fixed at create (the flag is ignored on other shapes, at create and here)
    WN_CHECK_ARG(!D->fastP || ((d->flags & WN_DECODER_GATE_ROWS) != 0) == D->gate_rows,
                 "wn_decoder_update_weights: the description %s WN_DECODER_GATE_ROWS, the handle was created %s it: a handle's form "
                 "is fixed at create", d->flags & WN_DECODER_GATE_ROWS ? "carries" : "lacks", D->gate_rows ? "with" : "without");
    WN_CHECK_ARG(((d->flags & WN_DECODER_TRACE_CHOSEN) != 0) == D->trace_chosen,
                 "wn_decoder_update_weights: the description %s WN_DECODER_TRACE_CHOSEN, the handle was created %s it: a handle's form "
                 "is fixed at create", d->flags & WN_DECODER_TRACE_CHOSEN ? "carries" : "lacks", D->trace_chosen ? "with" : "without");
    WN_CHECK_ARG(((d->flags & WN_DECODER_FORCED_TOKENS) != 0) == D->forced,
                 "wn_decoder_update_weights: the description %s WN_DECODER_FORCED_TOKENS, the handle was created %s it: a handle's form "
                 "is fixed at create", d->flags & WN_DECODER_FORCED_TOKENS ? "carries" : "lacks", D->forced ? "with" : "without");
    WN_CHECK_ARG(((d->flags & WN_DECODER_FRAME_RING) != 0) == D->frame_ring,
                 "wn_decoder_update_weights: the description %s WN_DECODER_FRAME_RING, the handle was created %s it: a handle's form "
                 "is fixed at create", d->flags & WN_DECODER_FRAME_RING ? "carries" : "lacks", D->frame_ring ? "with" : "without");
    for (int j = 0; D->gate_rows && j < D->meta.nlayers; ++j)
        WN_CHECK_ARG(!(d->bf && d->bf[j]) == !(d->bg && d->bg[j]), "decoder: bf/bg must both be present or absent");
    if ((rc = check_frame_desc(D, d))) return rc;
    if ((rc = check_weight_ptrs(D, d))) return rc;
    if ((rc = pack_weights(D, d, as_stream(stream)))) return rc;
    return take_frames(D, d, as_stream(stream));
}

int wn_decoder_load_state(void* handle, const int32_t* tokens, int W, const float* const* causal_out,
                          const float* const* layer_in, void* stream) {
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D && tokens && layer_in && W > 0, "wn_decoder_load_state: bad argument");
    hipStream_t s = as_stream(stream);
    const DecMeta& M = D->meta;
    if (M.fwc > 1) hipLaunchKernelGGL(k_load_tok_ring, dim3(1), dim3(64), 0, s, tokens, D->tok_ring, W, M.fwc - 1);
    for (int i = 1; i < M.ncausal; ++i) {
        WN_CHECK_ARG(causal_out && causal_out[i - 1], "wn_decoder_load_state: causal_out[%d] NULL", i - 1);
        int Dd = M.fwc - 1, C = D->causal[i].cin;
        if (Dd > 0)
            hipLaunchKernelGGL(k_load_ring, dim3(cdiv((long long)Dd * C, 256)), dim3(256), 0, s, causal_out[i - 1],
                               D->arena + D->causal[i].ring, W, Dd, C);
    }
    for (int j = 0; j < M.nlayers; ++j) {
        WN_CHECK_ARG(layer_in[j], "wn_decoder_load_state: layer_in[%d] NULL", j);
        int Dd = (M.fw - 1) * D->layers[j].d;
        if (Dd > 0)
            hipLaunchKernelGGL(k_load_ring, dim3(cdiv((long long)Dd * M.Cr, 256)), dim3(256), 0, s, layer_in[j],
                               D->arena + D->layers[j].ring, W, Dd, M.Cr);
    }
    WN_LAUNCH_CHECK();
    D->step = W;
    return WN_OK;
}

// floats between the rows of a run's prob_trace: Q, or kProbChosen on a WN_DECODER_TRACE_CHOSEN handle
static int trace_stride(const Decoder* D) { return D->trace_chosen ? kProbChosen : D->meta.Q; }

// do_sample of a run's launch: kSampleGiven on a WN_DECODER_FORCED_TOKENS handle (out_tokens is read before it is written)
static int sample_mode(const Decoder* D) { return D->forced ? kSampleGiven : kSampleDraw; }

// n steps were launched: the one writer of both counters after create / update / load_state
static void advance(Decoder* D, long long n) { D->step += n; D->since_set += n; }

// wn_decoder_step / wn_decoder_run behind their own argument checks: n steps of one handle.  A run that would read past
// the frame table or pass WnDecoderDesc.step_limit is refused before any device work, never clamped
static int run_one(const char* fn, Decoder* D, int token, const double* uniforms, int n, int32_t* out_tokens, float* prob,
                   int prob_stride, int apply_softmax, int do_sample, const SampleCtl& sc, bool three_wgs, hipStream_t s) {
    WN_CHECK_ARG(D->step + n < (1ll << 31), "%s: step counter overflow", fn);
    if (int rc = check_frames(fn, D, n)) return rc;
    WN_CHECK_ARG(D->step_limit <= 0 || D->since_set + n <= D->step_limit,
                 "%s: n = %lld more steps would pass step_limit = %d (%lld steps run since it was set)", fn, (long long)n,
                 D->step_limit, D->since_set);
    if (D->fastP) {
        if (int rc = decode_fast_launch(fast_utt(D, token, uniforms, out_tokens, prob, sc), D->meta.nlayers, n, prob_stride,
                                        apply_softmax, do_sample, D->meta.head_act, three_wgs, gate_launch(D), s))
            return rc;
        if (three_wgs) D->ran_multi = n > 1;       // (a single step is on one workgroup: an earlier run's entry stays readable)
    } else {
        // (k_decode takes the record's members as loose arguments: DESIGN.md, "The library's host side, tidied likewise")
        const DecAnyUtt q = any_utt(D, token, uniforms, out_tokens, prob, n, sc);
        const bool forced = do_sample == kSampleGiven;      // (the kernel itself only asks whether do_sample != 0)
        const bool ring = q.fr.ring != 0;
        const auto kern = ring ? (forced ? (lerp_table(D) ? k_decode<true, true, true> : k_decode<false, true, true>)
                                         : (lerp_table(D) ? k_decode<true, false, true> : k_decode<false, false, true>))
                               : (forced ? (lerp_table(D) ? k_decode<true, true, false> : k_decode<false, true, false>)
                                         : (lerp_table(D) ? k_decode<true, false, false> : k_decode<false, false, false>));
        hipLaunchKernelGGL(kern, dim3(1), dim3(kDecThreads), D->lds_bytes, s, D->meta, q.causal, q.layers, q.heads, q.arena, q.tok_ring,
                           q.n0, q.nsteps, q.first_token, q.uniforms, q.out_tokens, q.prob_out, prob_stride, apply_softmax, do_sample,
                           q.sc, q.fr);
        WN_LAUNCH_CHECK();
    }
    advance(D, n);
    return WN_OK;
}

int wn_decoder_step(void* handle, int32_t token, float* prob, int apply_softmax, void* stream) {
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D && prob, "wn_decoder_step: bad argument");
    WN_CHECK_ARG(token >= 0 && token < D->meta.Q, "wn_decoder_step: token %d outside [0,%d)", token, D->meta.Q);
    return run_one("wn_decoder_step", D, (int)token, nullptr, 1, nullptr, prob, D->meta.Q, apply_softmax, 0, SampleCtl(), false,
                   as_stream(stream));
}

int wn_decoder_run(void* handle, int32_t first_token, const double* uniforms, int n, int32_t* out_tokens,
                   float* prob_trace, void* stream) {
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D && uniforms && out_tokens && n > 0, "wn_decoder_run: bad argument");
    WN_CHECK_ARG(first_token >= 0 && first_token < D->meta.Q, "wn_decoder_run: token outside [0,Q)");
    return run_one("wn_decoder_run", D, (int)first_token, uniforms, n, out_tokens, prob_trace, trace_stride(D), 1, sample_mode(D), launch_ctl(D), D->three_wgs,
                   as_stream(stream));
}

int wn_decoder_set_sampling(void* handle, float temperature, int top_k, double top_p) {
    if (int rc = check_sampling("wn_decoder_set_sampling", temperature, top_k, top_p)) return rc;
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D, "wn_decoder_set_sampling: NULL handle");
    WN_CHECK_SHAPE(D->meta.Q <= 32 * kDecThreads, "wn_decoder_set_sampling: Q = %d is more than the filter's %d tokens", D->meta.Q,
                   32 * kDecThreads);
    D->ctl.inv_temp = 1.0f / temperature;          // once, on the host, in fp32
    D->ctl.top_k = top_k;
    D->ctl.top_p = top_p >= 1.0 ? 1.0 : top_p;
    return WN_OK;
}

int wn_decoder_batch_max(void) { return kDecMaxBatch; }

// the any-shape form of wn_decoder_run_batch, after every check: the utterances' table into handle 0's device buffer (one
// async copy from its pinned image), then one launch of n_handles workgroups.  nsteps[u]: utterance u's own step count
// tile = 0: one workgroup of k_decode_batch per utterance.  tile = U >= 2 (checked): ceil(n_handles / U) workgroups of k_decode_tile<U>
static int run_batch_any(void* const* handles, int n_handles, const int32_t* first_tokens, const double* const* uniforms,
                         const int* nsteps, int32_t* const* out_tokens, float* const* prob_traces, int tile, hipStream_t s) {
    Decoder* D0 = (Decoder*)handles[0];
    if (n_handles > D0->batch_cap) {                   // first use, or a larger batch than ever before
        if (D0->batch_tab) { WN_HIP(hipFree(D0->batch_tab)); D0->batch_tab = nullptr; }      // hipFree waits for its readers
        if (D0->batch_img) { WN_HIP(hipHostFree(D0->batch_img)); D0->batch_img = nullptr; }
        D0->batch_cap = 0;
        if (!D0->batch_copied) WN_HIP(hipEventCreateWithFlags(&D0->batch_copied, hipEventDisableTiming));
        WN_HIP(hipMalloc(&D0->batch_tab, (size_t)n_handles * sizeof(DecAnyUtt)));
        WN_HIP(hipHostMalloc(&D0->batch_img, (size_t)n_handles * sizeof(DecAnyUtt), hipHostMallocDefault));
        D0->batch_cap = n_handles;
    } else {
        // the previous call's copy may still be queued (behind other work of its stream) and reads the image: a host wait
        // for that COPY, not for the launch behind it; a caller that has read its tokens back finds it done.  (Like the
        // allocation above, not something a stream capture can hold.)
        WN_HIP(hipEventSynchronize(D0->batch_copied));
    }
    DecAnyUtt* img = (DecAnyUtt*)D0->batch_img;
    for (int u = 0; u < n_handles; ++u) {
        const Decoder* D = (const Decoder*)handles[u];
        img[u] = any_utt(D, (int)first_tokens[u], uniforms[u], out_tokens[u], prob_traces ? prob_traces[u] : nullptr, nsteps[u],
                         launch_ctl(D));
    }
    WN_HIP(hipMemcpyAsync(D0->batch_tab, img, (size_t)n_handles * sizeof(DecAnyUtt), hipMemcpyHostToDevice, s));
    WN_HIP(hipEventRecord(D0->batch_copied, s));
    const bool ring = D0->frame_ring && D0->frames.n > 0;                         // (the handles agree on all three modes)
    if (tile)
        return decode_tile_launch(tile, lerp_table(D0), D0->forced, ring, D0->meta, (const DecAnyUtt*)D0->batch_tab, n_handles,
                                  trace_stride(D0), tile_lds(D0, tile), s);
    const auto kern = ring ? (D0->forced ? (lerp_table(D0) ? k_decode_batch<true, true, true> : k_decode_batch<false, true, true>)
                                         : (lerp_table(D0) ? k_decode_batch<true, false, true> : k_decode_batch<false, false, true>))
                           : (D0->forced ? (lerp_table(D0) ? k_decode_batch<true, true, false> : k_decode_batch<false, true, false>)
                                         : (lerp_table(D0) ? k_decode_batch<true, false, false> : k_decode_batch<false, false, false>));
    hipLaunchKernelGGL(kern, dim3(n_handles), dim3(kDecThreads), D0->lds_bytes, s, D0->meta, (const DecAnyUtt*)D0->batch_tab,
                       n_handles, trace_stride(D0));
    WN_LAUNCH_CHECK();
    return WN_OK;
}

// wn_decoder_run_batch: utterance u's handle holds utterance 0's model
static int same_model(const Decoder* D, const Decoder* D0, int u, int same_weights) {
    WN_CHECK_SHAPE(!D->fastP == !D0->fastP, "wn_decoder_run_batch: utterance %d is %s decoder, utterance 0 is not: one launch takes one form", u,
                   D->fastP ? "a nine-workgroup (config 4's shape)" : "an any-shape");
    const DecMeta &A = D->meta, &B = D0->meta;
    WN_CHECK_SHAPE(A.nlayers == B.nlayers && A.head_act == B.head_act && A.Q == B.Q && A.Cr == B.Cr && A.Cs == B.Cs && A.fw == B.fw &&
                       A.fwc == B.fwc && A.ncausal == B.ncausal && A.nhead == B.nhead && A.maxc == B.maxc &&
                       D->layers.size() == D0->layers.size(),
                   "wn_decoder_run_batch: utterance %d's model differs from utterance 0's (layers, channels, filter widths, Q or head "
                   "activation)", u);
    for (size_t l = 0; l < D->layers.size(); ++l)
        WN_CHECK_SHAPE(D->layers[l].d == D0->layers[l].d && D->layers[l].cd == D0->layers[l].cd,
                       "wn_decoder_run_batch: layer %d of utterance %d has another dilation / width than utterance 0's", (int)l, u);
    for (size_t i = 0; i < D->causal.size(); ++i)
        WN_CHECK_SHAPE(D->causal[i].cin == D0->causal[i].cin && D->causal[i].cout == D0->causal[i].cout,
                       "wn_decoder_run_batch: causal layer %d of utterance %d has other channels than utterance 0's", (int)i, u);
    for (size_t i = 0; i < D->heads.size(); ++i)
        WN_CHECK_SHAPE(D->heads[i].cin == D0->heads[i].cin && D->heads[i].cout == D0->heads[i].cout,
                       "wn_decoder_run_batch: head layer %d of utterance %d has other channels than utterance 0's", (int)i, u);
    // same_weights = 1 reads ONE copy of the packed weights (handle 0's) for every utterance: only sound when every
    // handle was packed from the same model -- the same weight pointers at its last create / update_weights.  (The
    // any-shape form checks the claim and then reads each utterance's own copy all the same.)
    const bool tile = same_weights >= 2 && !D0->fastP;
    WN_CHECK_ARG(!same_weights || tile || D->src_key == D0->src_key,
                 "wn_decoder_run_batch: same_weights = 1 but utterance %d's handle was packed from other weights than utterance 0's", u);
    if (!tile) return WN_OK;
    // a tile really reads handle 0's copy for every utterance but the static gate biases: the key without the gate-bias
    // pointers, and handle 0's arena layout offset for offset (whether a bias exists is part of the layout)
    WN_CHECK_ARG(D->tile_key == D0->tile_key, "wn_decoder_run_batch: same_weights = %d (a tile size) but utterance %d's handle was packed "
                 "from other weights than utterance 0's (gate biases apart)", same_weights, u);
    bool eq = true;
    for (size_t i = 0; i < D->causal.size(); ++i)
        eq = eq && D->causal[i].w == D0->causal[i].w && D->causal[i].b == D0->causal[i].b && D->causal[i].ring == D0->causal[i].ring;
    for (size_t l = 0; l < D->layers.size(); ++l) {
        const DecLayer &a = D->layers[l], &b = D0->layers[l];
        eq = eq && a.wfg == b.wfg && a.bfg == b.bfg && a.wps == b.wps && a.bps == b.bps && a.ring == b.ring;
    }
    for (size_t i = 0; i < D->heads.size(); ++i) eq = eq && D->heads[i].w == D0->heads[i].w && D->heads[i].b == D0->heads[i].b;
    WN_CHECK_ARG(eq, "wn_decoder_run_batch: same_weights = %d (a tile size) but the arena layout of utterance %d's handle differs from "
                 "utterance 0's (a bias one was created with and the other without): a tile reads every utterance at handle 0's offsets",
                 same_weights, u);
    return WN_OK;
}

// wn_decoder_run_batch clamps where run_one refuses: utterance u runs *nu = min(n, steps left under its handle's step_limit)
// steps, n without a limit
static int steps_left(const Decoder* D, int u, int n, bool any, int* nu) {
    const long long left = D->step_limit > 0 && D->step_limit - D->since_set < n ? D->step_limit - D->since_set : n;
    WN_CHECK_ARG(left > 0, "wn_decoder_run_batch: utterance %d has run all %d steps of its step_limit: leave a finished utterance "
                           "out of the launch", u, D->step_limit);
    // the nine-workgroup form runs two steps at least: its existing rule, here per utterance (a launch whose own n is below
    // 2 is refused as ever, by decode_fast_batch_ok)
    WN_CHECK_ARG(any || left == n || left >= 2, "wn_decoder_run_batch: utterance %d has %lld step left under its step_limit = %d: "
                                                "the nine-workgroup form runs 2 at least", u, left, D->step_limit);
    *nu = (int)left;
    WN_CHECK_ARG(D->step + left < (1ll << 31), "wn_decoder_run_batch: step counter overflow");
    return WN_OK;
}

int wn_decoder_run_batch(void* const* handles, int n_handles, const int32_t* first_tokens, const double* const* uniforms, int n,
                         int32_t* const* out_tokens, float* const* prob_traces, int same_weights, void* stream) {
    WN_CHECK_ARG(handles && first_tokens && uniforms && out_tokens && n_handles >= 1 && n > 0, "wn_decoder_run_batch: bad argument");
    Decoder* D0 = (Decoder*)handles[0];
    WN_CHECK_ARG(D0, "wn_decoder_run_batch: NULL handle of utterance 0");
    // handle 0 chooses the form: the nine-workgroup decoder (decoder_fast.hip) or one workgroup of k_decode_batch per utterance
    const bool any = !D0->fastP;
    const int limit = any ? WN_DECODER_BATCH_MAX_ANY : kDecMaxBatch;
    WN_CHECK_SHAPE(n_handles <= limit, "wn_decoder_run_batch: at most %d utterances per launch of %s decoders", limit,
                   any ? "any-shape" : "nine-workgroup");
    WN_CHECK_ARG(same_weights == 0 || same_weights == 1 || same_weights == 2 || same_weights == 4 || same_weights == 8 ||
                     same_weights == WN_DECODER_TILE_MAX,
                 "wn_decoder_run_batch: same_weights = %d is neither 0, 1 nor a tile size (2, 4, 8, %d)", same_weights, WN_DECODER_TILE_MAX);
    // a tile size on any-shape handles: U utterances per workgroup, one copy of the weights (nine-workgroup handles: as 1)
    const int tile = any && same_weights >= 2 ? same_weights : 0;
    if (tile && tile_lds(D0, tile) > kDecLdsMax) {
        int fit = 1;
        for (int U = 2; U <= WN_DECODER_TILE_MAX; U *= 2)
            if (tile_lds(D0, U) <= kDecLdsMax) fit = U;
        WN_CHECK_SHAPE(false, "wn_decoder_run_batch: a tile of %d utterances needs %zu bytes of LDS (%d x (7 x %d + 16) floats), more than "
                       "%zu: the largest tile that fits this model is %d", tile, tile_lds(D0, tile), tile, D0->meta.maxc, kDecLdsMax, fit);
    }
    DecUtt utt[kDecMaxBatch];
    int nu[WN_DECODER_BATCH_MAX_ANY];              // the utterances' own step counts
    bool gate = false;                             // nine-workgroup form: some utterance has gate rows to add
    for (int u = 0; u < n_handles; ++u) {          // per utterance: arguments, same model, steps, frames, record
        const Decoder* D = (const Decoder*)handles[u];
        WN_CHECK_ARG(D && uniforms[u] && out_tokens[u], "wn_decoder_run_batch: NULL handle / uniforms / out_tokens of utterance %d", u);
        for (int v = 0; v < u; ++v) WN_CHECK_ARG(handles[v] != handles[u], "wn_decoder_run_batch: handle %d given twice", u);
        WN_CHECK_SHAPE(!D->fastP || D->three_wgs, "wn_decoder_run_batch: utterance %d's decoder was created with WN_DECODER_ONE_WORKGROUP: "
                                                  "the one-workgroup specialised kernel has no batched form", u);
        if (int rc = same_model(D, D0, u, same_weights)) return rc;
        // the trace's form is the launch's (one stride for every workgroup)
        WN_CHECK_ARG(D->trace_chosen == D0->trace_chosen, "wn_decoder_run_batch: utterance %d was created %s WN_DECODER_TRACE_CHOSEN, "
                     "utterance 0 %s it: the handles of a launch agree on the flag", u, D->trace_chosen ? "with" : "without",
                     D0->trace_chosen ? "with" : "without");
        // ... and so is whether out_tokens is read (one mode for every workgroup)
        WN_CHECK_ARG(D->forced == D0->forced, "wn_decoder_run_batch: utterance %d was created %s WN_DECODER_FORCED_TOKENS, "
                     "utterance 0 %s it: the handles of a launch agree on the flag", u, D->forced ? "with" : "without",
                     D0->forced ? "with" : "without");
        // ... and whether the table is a ring (one walk for every workgroup)
        WN_CHECK_ARG(D->frame_ring == D0->frame_ring, "wn_decoder_run_batch: utterance %d was created %s WN_DECODER_FRAME_RING, "
                     "utterance 0 %s it: the handles of a launch agree on the flag", u, D->frame_ring ? "with" : "without",
                     D0->frame_ring ? "with" : "without");
        WN_CHECK_ARG(first_tokens[u] >= 0 && first_tokens[u] < D->meta.Q, "wn_decoder_run_batch: token outside [0,Q)");
        if (int rc = steps_left(D, u, n, any, &nu[u])) return rc;
        const FrameTable &F = D->frames, &F0 = D0->frames;
        WN_CHECK_ARG((F.n > 0) == (F0.n > 0) && (F.n <= 0 || F.hop == F0.hop),
                     "wn_decoder_run_batch: utterance %d and utterance 0 disagree on having a frame table or on its hop", u);
        WN_CHECK_ARG(F.n <= 0 || F.interp == F0.interp,
                     "wn_decoder_run_batch: utterance %d and utterance 0 disagree on frame_interp (repeat / linear)", u);
        if (int rc = check_frames("wn_decoder_run_batch", D, nu[u])) return rc;
        if (!any) {
            utt[u] = fast_utt(D, (int)first_tokens[u], uniforms[u], out_tokens[u], prob_traces ? prob_traces[u] : nullptr, launch_ctl(D));
            utt[u].nsteps = nu[u];
            gate = gate || gate_launch(D);
        }
    }
    WN_CHECK_SHAPE(any || decode_fast_batch_ok(D0->meta.nlayers, n_handles, n),
                   "wn_decoder_run_batch: %d utterances x 9 workgroups must all be resident on the device, and n >= 2", n_handles);
    const int rc = any ? run_batch_any(handles, n_handles, first_tokens, uniforms, nu, out_tokens, prob_traces, tile, as_stream(stream))
                       : decode_fast_launch_batch(n_handles, utt, D0->meta.nlayers, n, trace_stride(D0), sample_mode(D0), D0->meta.head_act, same_weights != 0,
                                                  gate, as_stream(stream));
    if (rc) return rc;
    for (int u = 0; u < n_handles; ++u) {
        Decoder* D = (Decoder*)handles[u];
        if (!any) D->ran_multi = true;
        advance(D, nu[u]);
    }
    return WN_OK;
}

int wn_decoder_status(void* handle, void* stream) {
    Decoder* D = (Decoder*)handle;
    WN_CHECK_ARG(D, "wn_decoder_status: NULL handle");
    if (!D->fastP || !D->ran_multi) {                   // nothing that could have given up has run
        WN_HIP(hipStreamSynchronize(as_stream(stream)));
        return WN_OK;
    }
    int gave_up = 0;
    const int rc = decode_fast_status(D->fastP, D->meta.nlayers, as_stream(stream), &gave_up);
    if (rc) return rc;
    if (gave_up) {
        wn::set_error("wn_decoder_run: a wait between the nine workgroups gave up (they were not all resident); the tokens of "
                      "that run are void -- re-create the decoder with WN_DECODER_ONE_WORKGROUP");
        return WN_ETIMEOUT;
    }
    return WN_OK;
}

}  // extern "C"
