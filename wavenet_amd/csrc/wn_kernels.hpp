// Internal host-side launchers shared between translation units of libwavenet_hip.so.
#pragma once
#include "wn_common.hpp"

namespace wn {

// ---- one entry-point call: its WnExec resolved once by the entry point and handed down the host-side call tree ----------
struct StepPlan;
int check_precision(const char* fn, const WnExec* ex);   // WN_EARG + error text unless ex is NULL or its precision is 0 .. 3
// WN_EXEC_BIAS_PER_CLIP: WN_EARG + error text unless the stride covers a row of Cd floats and both rows are given
int check_bias_rows(const char* fn, const WnExec* ex, int Cd, const void* row_f, const void* row_g, const char* names);
// Local conditioning (WnStackDesc.bias_hop > 0 under WN_EXEC_BIAS_PER_CLIP): a clip's bias row becomes a block of rows, one per
// frame of `hop` positions, `stride` floats apart; position t reads frame (t + phase) / hop.  hop == 0: one row per clip.
// interp == 1 (WnStackDesc.bias_interp, linear interpolation between frames): with p = t + phase, j = p / hop and
// alpha = float(p % hop) / float(hop), position t reads  r[j] + alpha * (r[j + 1] - r[j])  -- bias_lerp, three separately
// rounded fp32 operations, so equal neighbours (and alpha == 0) give r[j] exactly; a block holds one row more than the frames
// the call covers.  interp == 0: the row of the frame, as before.
// tab != NULL (WnStackDesc.bias_phase_tab): a phase per clip in device memory, tab[b] for clip b; `phase` is then 0 and unused.
struct BiasFrames {
    int hop, phase; long long stride; int interp; const int* tab;
    // host side, hop > 0.  The largest phase a clip can have: a table's values are not known on the host, so with one
    // everything is sized for hop - 1
    int worst_phase() const { return tab ? hop - 1 : phase; }
    // rows of a clip's block that a call of T positions covers: its frames at the worst phase, one more with interpolation
    long long rows(int T) const { return ((long long)T + worst_phase() + hop - 1) / hop + (interp ? 1 : 0); }
};
// How a layer's gate bias rows (bf, bg) are addressed -- Call::bias_mode, THE place that derives it; every launcher maps the
// value to its own kernel's template arguments.  kCondClip: one row, shared (Call.bias_stride == 0) or per clip;
// kCondFrame: a row per (clip, frame); kCondLinear: interpolated between the frame's row and the next.
enum { kCondNone = 0, kCondClip = 1, kCondFrame = 2, kCondLinear = 3 };
// THE phase of clip b -- everything that needs one asks here.  Without a table it is the call's one value.  With one, the
// value read is reduced into [0, hop): callers pass values inside that range, the reduction is a fence that keeps a garbage
// value from taking an access outside the clip's block (the geometry is sized for phase hop - 1), not a feature.  Where b is
// uniform over a wave (a tile, a workgroup) this is one scalar load.
// frame_phase_as<TAB>: "has a table" as a compile-time mode, for a kernel whose scalar-phase instantiation must stay
// the code it was (k_layer_fwd_h2_t1, which sits near its register limit); frame_phase decides at run time.
// (the fence and alpha's formula stand alone as well: the bf16-storage tile loops, w16_layer.hip, read the table entry by an
// explicit scalar load and have the position inside the frame at hand already -- they call these two, nothing is restated)
__device__ __forceinline__ int bias_phase_fence(int v, int hop) { return (int)((unsigned)v % (unsigned)hop); }
__device__ __forceinline__ float bias_alpha(int rem, int hop) { return __fdiv_rn((float)rem, (float)hop); }   // rem = p % hop
template <bool TAB>
__device__ __forceinline__ int frame_phase_as(const BiasFrames& fr, int b) {
    return TAB ? bias_phase_fence(fr.tab[b], fr.hop) : fr.phase;
}
__device__ __forceinline__ int frame_phase(const BiasFrames& fr, int b) {
    return fr.tab ? frame_phase_as<true>(fr, b) : frame_phase_as<false>(fr, b);
}
// ph = frame_phase(fr, clip of t)
__device__ __forceinline__ long long bias_frame_off(const BiasFrames& fr, int ph, int t) {
    return fr.hop ? (long long)((t + ph) / fr.hop) * fr.stride : 0;
}
// the weight of row j + 1 at position t (fr.hop > 0): float(p % hop) / float(hop), an IEEE fp32 division
__device__ __forceinline__ float bias_frame_alpha(const BiasFrames& fr, int ph, int t) {
    const int p = t + ph;
    return bias_alpha(p - (p / fr.hop) * fr.hop, fr.hop);
}
__device__ __forceinline__ float bias_lerp(float a, float b, float alpha) {      // a + alpha (b - a), never contracted
    return __fadd_rn(a, __fmul_rn(alpha, __fsub_rn(b, a)));
}
struct Call {
    explicit Call(const WnExec* ex);     // ex == NULL: bf16x3, no flags, no scratch, no plan
    int precision;                       // WN_GEMM_*; WN_GEMM_FP32 under WN_EXEC_FORCE_GENERIC
    unsigned flags;
    void* ws;                            // the caller's scratch; its last kTail bytes hold the range words
    size_t ws_bytes;
    int fwd_t1_min_blocks;               // WnExec.fwd_t1_min_blocks with the default (512) filled in
    StepPlan* plan;                      // WnExec.plan, or NULL
    long long bias_stride;               // WN_EXEC_BIAS_PER_CLIP: floats between consecutive clips' bf / bg (dbf / dbg) rows; else 0
    BiasFrames frames = {0, 0, 0, 0, nullptr};    // set by wn_stack_fwd / wn_stack_bwd from the descriptor (per-frame rows); else hop == 0

    static constexpr size_t kTail = 256;
    bool flag(unsigned f) const { return (flags & f) != 0; }
    bool bias_per_clip() const { return flag(WN_EXEC_BIAS_PER_CLIP); }
    int bias_mode(const float* bf, const float* bg) const {      // kCond*, for a layer whose gate bias rows are (bf, bg)
        if (!bf && !bg) return kCondNone;
        return frames.hop <= 0 ? kCondClip : frames.interp ? kCondLinear : kCondFrame;
    }
    bool phase_from_table() const { return frames.tab != nullptr; }   // (kCondFrame / kCondLinear) a phase per clip, read on the device
    bool generic() const { return flag(WN_EXEC_FORCE_GENERIC); }
    bool split_b3() const { return precision != WN_GEMM_FP32; }   // the bf16-split GEMM kernels (every precision but fp32)
    bool one_term() const { return precision == WN_GEMM_BF16; }
    bool fp16x2() const { return precision == WN_GEMM_FP16X2; }
    bool layer_fast_path(int Cr, int Cd, int fw) const;   // the fused 32-channel kernels for this shape
    bool wide_layer(int Cr, int Cd, int fw) const;        // wide_layer_* for this shape (when not on the fused kernels)
    size_t room() const { return ws && ws_bytes >= kTail ? ws_bytes - kTail : 0; }   // scratch bytes ahead of the range words
    bool has_scratch(size_t bytes) const { return ws && ws_bytes >= bytes + kTail; }
    void* scratch(size_t bytes, const char* what) const;   // the caller's scratch; NULL + error text when it is too small
    // Device word holding the bits of max |x[i]| (a positive float orders like an unsigned): one pass per array and call,
    // shared by the launchers below it (the word lives in the scratch tail); NULL + error text when there is no scratch.
    // Used by the fp16 split (WN_GEMM_FP16X2) to scale operands whose range is not known in advance.
    const unsigned* absmax(const float* x, long long n, hipStream_t s);
    // a zeroed word of the same kind for a maximum the caller accumulates itself (atomicMax over several arrays); *fresh says
    // whether the word is new in this call (then it has been zeroed on the stream and must be filled) or was handed out for
    // the same key before
    unsigned* word(const void* key, bool* fresh, hipStream_t s) { return tail_word(key, nullptr, 0, fresh, s); }

  private:
    static constexpr int kWords = kTail / 4;
    unsigned* tail_word(const void* key, const float* x, long long n, bool* fresh, hipStream_t s);
    const void* key_[kWords] = {};       // key of each word of the tail handed out so far
    int nkeys_ = 0;
};

// ---- api.hip: what the per-layer and skip entry points run after their argument checks (the stack calls them too) ------
int layer_fwd(Call& c, const float* x, const float* Wf, const float* bf, const float* Wg, const float* bg, const float* Wp,
              const float* bp, float* out, float* z, float* f_save, float* g_save, int B, int T, int Cr, int Cd, int fw,
              int d, int Z, hipStream_t s);
int layer_bwd(Call& c, const float* x, const float* f, const float* g, const float* Wf, const float* Wg, const float* Wp,
              const float* dout, const float* dz_skip, float* dx, float* dWf, float* dbf, float* dWg, float* dbg,
              float* dWp, float* dbp, float* dab_ws, int B, int T, int Cr, int Cd, int fw, int d, int Z, hipStream_t s);
int skip_sum_fwd(Call& c, int L, const float* const* z, const float* const* Ws, const float* const* bs, const int* cd,
                 float* skip, int B, int T, int t_off, int Tw, int Cs, int accumulate, hipStream_t s);
int skip_bwd_dz(Call& c, int L, const float* const* Ws, const int* cd, const float* dskip, float* const* dz, int B, int T,
                int t_off, int Tw, int Cs, hipStream_t s);
int skip_bwd_dw(Call& c, int L, const float* const* z, const int* cd, const float* dskip, float* const* dWs,
                float* const* dbs, int B, int T, int t_off, int Tw, int Cs, hipStream_t s);

// ---- generic_kernels.hip (any shape) --------------------------------------------------------
int generic_embed_fwd(const int32_t*, const float*, const float*, float*, int, int, int, int, int, hipStream_t);
int generic_embed_bwd(const Call& c, const int32_t*, const float*, float*, float*, int, int, int, int, int, hipStream_t);
int generic_conv_fwd(const float*, const float*, const float*, float*, int, int, int, int, int, int, int,
                     hipStream_t);
int generic_conv_bwd(const float*, const float*, const float*, float*, float*, float*, int, int, int, int, int,
                     int, int, hipStream_t);
int generic_layer_fwd(const Call& c, const float* x, const float* Wf, const float* bf, const float* Wg, const float* bg,
                      const float* Wp, const float* bp, float* out, float* z, float* fs, float* gs, int B,
                      int T, int Cr, int Cd, int fw, int d, int Z, hipStream_t s);
int generic_layer_bwd(const Call& c, const float* x, const float* f, const float* g, const float* Wf, const float* Wg,
                      const float* Wp, const float* dout, const float* dzs, float* dx, float* dWf, float* dbf,
                      float* dWg, float* dbg, float* dWp, float* dbp, float* dab, int B, int T, int Cr, int Cd,
                      int fw, int d, int Z, hipStream_t s);
int generic_pointwise_fwd(const float*, const float*, const float*, float*, long long, int, int, int,
                          hipStream_t);
int generic_pointwise_bwd(const Call& c, const float*, const float*, const float*, float*, float*, float*, long long, int,
                          int, int, hipStream_t);
int generic_skip_sum_fwd(int L, const float* const* z, const float* const* Ws, const float* const* bs,
                         const int* cd, float* skip, int B, int T, int t_off, int Tw, int Cs, int accumulate,
                         hipStream_t s);
int generic_skip_bwd_dz(int L, const float* const* Ws, const int* cd, const float* dskip, float* const* dz,
                        int B, int T, int t_off, int Tw, int Cs, hipStream_t s);
int generic_skip_bwd_dw(const Call& c, int L, const float* const* z, const int* cd, const float* dskip, float* const* dWs,
                        float* const* dbs, int B, int T, int t_off, int Tw, int Cs, hipStream_t s);
// column sums out[m] += sum A[.][m]; with ws_bytes of scratch at ws (may be NULL) through per-chunk partials in a fixed order
int generic_colsum(const float* A, int nB, int nT, int tmin, int lda, int M, float* out, void* ws, size_t ws_bytes,
                   hipStream_t s);
int generic_softmax(const float*, float*, long long, int, hipStream_t);
int generic_softmax_xent(const float*, const int32_t*, float*, float*, long long, int, long long n_norm, hipStream_t);
// the two small launches around a loss kernel that leaves its per-workgroup sums in loss[kXentPart + workgroup]: the device-side
// count of the rows that count (n_norm < 0; *ncnt = its workgroups) and the fixed-order sum into loss[0]
int generic_xent_count(const int32_t* target, long long N, int Q, float* loss, int* ncnt, hipStream_t s);
int generic_xent_final(float* loss, int nblocks, long long n_norm, int ncnt, hipStream_t s);
int generic_transpose(const float* src, float* dst, int batch, int R, int Cc, hipStream_t s);
int generic_sample(const float*, const double*, int32_t*, int, int, hipStream_t);
int generic_sample_filtered(const float*, const double*, int32_t*, int, int, int, double, hipStream_t);
int generic_mulaw_encode_pcm16(const int16_t* pcm, const int32_t* lut, int32_t* tok, long long n, hipStream_t s);
int generic_mulaw_decode(const int32_t* tok, const float* table, float* out, long long n, int Q, hipStream_t s);
int generic_sqnorm(const float* g, const float* p, long long n, float gmult, float wd, float* out, hipStream_t s);
// ---- the step plan (plan.hip, ABI 5): weight-only preparation hoisted to the start of a training step -------------------
struct CGArgs;
// launch_colgemm_b3: true + the prepared image / range word when a READY plan holds this launch's weight tiles (a recording
// plan registers the job and returns false)
bool plan_split_image(const Call& c, const CGArgs& a, int mode, int mtiles, int cps, int nchunks, int one, size_t bytes,
                      const __bf16** img, const unsigned** wmax);
const void* plan_layer_h2_images(const Call& c, int L, const float* const* Wf, const float* const* Wg,
                                 const float* const* Wp);
unsigned* plan_sync_words(const Call& c, int nwords);   // the multi-layer backward's dataflow words, zeroed by wn_plan_prepare
unsigned* plan_xmax_producer(const Call& c);            // word that receives max |out| of a GEMM (zeroed by wn_plan_prepare)
void plan_xmax_written(const Call& c, const void* out); // ... called by the launcher whose kernel really fills it
const unsigned* plan_xmax_consumer(const Call& c, const void* x);   // ... for the call that needs the range of the same array
int generic_absmax(const float* x, long long n, unsigned* slot, hipStream_t s);
int generic_zero_word(unsigned* w, hipStream_t s);        // by a kernel: see generic_kernels.hip
int generic_scale_by_dev(float* x, const float* sdev, long long n, hipStream_t s);
int generic_rule(int rule, float* p, const float* g, float* s1, float* s2, long long n, float lr, float hy, float eps,
                 float wd, const float* sqnorm, float clip, float gmult, const float* lr_dev, hipStream_t s);
int generic_adam(float* p, const float* g, float* m, float* v, long long n, float lr_t, float b1, float b2,
                 float eps, float wd, const float* sqnorm, float clip, float gmult, const float* lr_dev,
                 float dscale, hipStream_t s);

// ---- mfma_layer.hip: fp32-MFMA fused residual layer, Cr = Cd = 32, fw = 2 -------------------
bool mfma_layer_supported(int Cr, int Cd, int fw);
size_t mfma_layer_h2_image_bytes(int L);
int mfma_layer_pack_h2(int L, const float* const* Wf, const float* const* Wg, const float* const* Wp, void* img,
                       hipStream_t s);
bool mfma_layer_fwd_h2_ok(const Call& c, int B, int T, int t_live);
// bf / bg != NULL: per-clip bias rows (WN_EXEC_BIAS_PER_CLIP; 16-byte aligned, c.bias_stride % 4 == 0), the COND kernels
int mfma_layer_fwd_h2(const Call& c, const float* x, const void* img, int l, float* out, float* z, float* fs, float* gs, int B,
                      int T, int d, int Z, int t_live, hipStream_t s, const float* bf = nullptr, const float* bg = nullptr);
int mfma_layer_fwd_group_len(const int* dil, int l0, int L);   // layers from l0 on that one group launch can chain
int mfma_layer_fwd_h2_group(const float* x, const void* img, int l0, int nl, float* const* outs, float* const* zs,
                            float* const* fs, float* const* gs, const int* dil, const int* Zs, int B, int T, hipStream_t s);
int mfma_layer_fwd(const Call& c, const float* x, const float* Wf, const float* bf, const float* Wg, const float* bg,
                   const float* Wp, const float* bp, float* out, float* z, float* fs, float* gs, int B, int T,
                   int d, int Z, int t_live, hipStream_t s);

// ---- mfma_layer_bwd.hip: backward of the same shape; bias gradients come from the scratch -----
int mfma_layer_bwd(const float* x, const float* f, const float* g, const float* Wf, const float* Wg,
                   const float* Wp, const float* dout, const float* dzs, float* dx, float* dWf, float* dWg,
                   float* dWp, float* dab, int B, int T, int d, int Z, hipStream_t s, bool fixed_order = false);
// (fixed_order: the workgroups' partial weight-gradient tiles are summed without atomics -- bit-reproducible; what a call
// with per-clip bias rows asks for)
size_t mfma_layer_bwd_extra_ws_floats();
// Chained backward of the fused layer (mfma_layer_bwd.hip).  dout[t] = Vin[t] + Uin[t + dU], rows below vu_t0 taken as
// 0; dzs (may be NULL) is dz_skip for columns t >= dz_t0; columns below t_live are not computed.
int mfma_layer_bwd_chain(const Call& c, const float* x, const float* f, const float* g, const float* Wf, const float* Wg,
                         const float* Wp, const float* Vin, const float* Uin, int dU, int vu_t0, const float* dzs,
                         int dz_t0, float* Vout, float* Uout, float* part, int B, int T, int d, int Z, int t_live,
                         int* nwg, hipStream_t s, bool from_z = false);   // from_z: `f` holds z, tanh = z / sigmoid
int mfma_chain_multi_max_layers();
int mfma_layer_bwd_chain_multi(const Call& c, int n, const int* layer, const float* const* Wf, const float* const* Wg,
                               const float* const* Wp, const int* d, const int* Z, const int* t_live, const int* vu_t0,
                               const int* dU, const float* x0, const float* xs, const float* z, const float* g,
                               const float* dz, float* const* V, float* const* U, float* part, size_t part_stride,
                               unsigned* sync, int B, int T, int dz_t0, int* nwg, hipStream_t s, bool sync_zeroed = false);
size_t mfma_chain_multi_sync_words(int B, int T);
size_t mfma_chain_part_floats();
int mfma_chain_reduce_all(const float* part, int L, const int* nwg, float* const* dWf, float* const* dWg,
                          float* const* dWp, hipStream_t s, const float* V = nullptr, const float* U = nullptr,
                          float* dx = nullptr, int B = 0, int T = 0, int dU = 0, int vu_t0 = 0);
int mfma_chain_combine(const float* V, const float* U, float* dx, int B, int T, int dU, int vu_t0, hipStream_t s);
int generic_layer_bwd_biases(const Call& c, const float* dab, const float* dout, float* dbf, float* dbg, float* dbp, int B,
                             int T, int Cr, int Cd, int Z, hipStream_t s);
// WN_EXEC_BIAS_PER_CLIP: the bias gradients of both gates, one launch, no atomics, no scratch, by c.bias_mode(dbf, dbg).
// kCondClip: dbf[b * c.bias_stride + m] += sum_{t in [tmin, T)} da[(b T + t) lda + m], dbg likewise from dg, m < Cd, in the
// summation order of the shared-bias column sums of a B = 1 call.  kCondFrame: row f of the clip's block receives the t of
// frame f; rows of frames wholly below tmin are not touched.  kCondLinear: row f of a block of frames + 1 rows receives
// sum (1 - alpha_t) d[t] over the t of frame f + sum alpha_t d[t] over those of frame f - 1.  The orders: generic_kernels.hip.
int generic_colsum_bias_rows(const Call& c, const float* da, const float* dg, int lda, int B, int T, int tmin, int Cd,
                             float* dbf, float* dbg, hipStream_t s);

// ---- wide_layer.hip: residual layer for any Cr, Cd multiple of 32 and any fw, composed from the channel GEMMs
bool wide_layer_supported(int Cr, int Cd, int fw);
int wide_layer_fwd(Call& c, const float* x, const float* Wf, const float* bf, const float* Wg, const float* bg, const float* Wp,
                   const float* bp, float* out, float* z, float* fs, float* gs, int B, int T, int Cr, int Cd, int fw,
                   int d, int Z, hipStream_t s);
int wide_layer_bwd(Call& c, const float* x, const float* f, const float* g, const float* Wf, const float* Wg, const float* Wp,
                   const float* dout, const float* dzs, float* dx, float* dWf, float* dbf, float* dWg, float* dbg,
                   float* dWp, float* dbp, float* ws, int B, int T, int Cr, int Cd, int fw, int d, int Z,
                   hipStream_t s, const float* z = nullptr);   // z = f g when the caller still has it (dWp reads one tensor)

// ---- mfma_gemm.hip: fp32-MFMA channel GEMMs over time columns (all widths multiples of 32) ---
bool mfma_skip_supported(int L, const int* cd, int Cs);
int mfma_skip_sum_fwd(Call& c, int L, const float* const* z, const float* const* Ws, const float* const* bs, const int* cd,
                      float* skip, int B, int T, int t_off, int Tw, int Cs, int accumulate, hipStream_t s);
int mfma_skip_bwd_dz(Call& c, int L, const float* const* Ws, const int* cd, const float* dskip, float* const* dz, int B,
                     int T, int t_off, int Tw, int Cs, bool window_only, hipStream_t s);
bool mfma_pointwise_supported(int Cin, int Cout);
int mfma_head_xent(Call& c, const float* x, const float* W, const float* bias, const int32_t* target, float* loss, float* dlogits,
                   long long N, int Cin, int Cout, int act, long long n_norm, int ncnt, hipStream_t s);
int mfma_pointwise_fwd(Call& c, const float* x, const float* W, const float* bias, float* out, long long N, int Cin,
                       int Cout, int act, hipStream_t s);
int mfma_pointwise_bwd_dx(Call& c, const float* x, const float* W, const float* dout, float* dx, long long N, int Cin,
                          int Cout, int act, hipStream_t s);

int mfma_skip_bwd_dw(Call& c, int L, const float* const* z, const int* cd, const float* dskip, float* const* dWs, int B, int T,
                     int t_off, int Tw, int Cs, hipStream_t s);
// dbias != NULL: dbias[o] += sum_n dout[n][o] is taken along where the kernel can (then *dbias_done = true)
int mfma_pointwise_bwd_dw(const Call& c, const float* x, const float* dout, float* dW, long long N, int Cin, int Cout, int act,
                          float* dbias, bool* dbias_done, hipStream_t s);

}  // namespace wn
