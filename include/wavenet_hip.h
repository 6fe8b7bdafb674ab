/*
 * wavenet_hip.h -- C ABI of libwavenet_hip.so (MI355X / gfx950).
 *
 * The reference (musyoku/wavenet) has no native boundary: its hot path sits behind a Python
 * class API and every FLOP is executed by Chainer.  This header is the boundary the reference
 * would bind if it had one: each entry point replaces the Chainer call sequence of the cited
 * reference lines.  wavenet_amd/{wavenet,faster_wavenet}.py call it through ctypes and keep the
 * reference's Python face (class / method / Params names) on top.
 *
 * Conventions (all entry points)
 *   - return 0 on success; <0 on failure (WN_EARG bad argument, WN_ESHAPE unsupported shape,
 *     WN_EHIP a HIP runtime error, WN_ETIMEOUT a device-side wait that gave up).  wn_last_error() gives a thread-local
 *     message.
 *   - every tensor pointer is a DEVICE pointer owned by the caller; nothing is retained after the
 *     call returns except by decoder handles, which copy what they need at create / load time.
 *   - no allocation, no synchronisation: work is enqueued on `stream` (a hipStream_t; NULL = the
 *     default stream) and the call returns immediately.  Scratch memory (operand images of the split-product GEMMs,
 *     per-workgroup partial tiles, embedding-gradient tables) comes from the caller through WnExec.
 *   - no mutable process state: the arithmetic of the channel GEMMs is an argument of every call that has one (WnExec).
 *   - activations are float32, time-major / channel-minor:  x[b][t][c]  == the reference's
 *     (B, C, 1, T) tensor in channels-last memory format.
 *   - convolution weights keep the reference's element order: a (Cout, Cin, 1, fw) or
 *     (Cout, Cin, fw, 1) Chainer W (wavenet.py:418-424) is the same memory as W[o][c][k], tap
 *     k = 0 the OLDEST sample.  1x1 weights are W[o][c].  A NULL bias pointer means "no bias".
 *   - Z is the reference's zero prefix (columns t < Z of a d > 1 dilated conv are exactly 0, no
 *     bias; wavenet.py:303-340).  The host computes it: Z = max(0, (fw-1)d - pad).  Pass 0 for the
 *     textbook convolution.
 */
#ifndef WAVENET_HIP_H
#define WAVENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: the functions declared between this push and the pop at the end of the
 * header are its ONLY dynamic symbols (tests/test_host_cpu.py holds `nm -D` to this list). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define WN_ABI_VERSION 5
#define WN_OK      0
#define WN_EARG   -1
#define WN_ESHAPE -2
#define WN_EHIP   -3
#define WN_ETIMEOUT -4   /* ABI 4: a device-side wait between co-resident workgroups gave up (wn_decoder_status) */

#define WN_ACT_NONE 0
#define WN_ACT_RELU 1   /* wavenet.py:588 */
#define WN_ACT_ELU  2   /* faster_wavenet.py:108 */

#define WN_MAX_SRC 64   /* sources per wn_skip_sum_* launch; longer lists are chunked by the caller */

int wn_abi_version(void);
const char* wn_last_error(void);

/* Per-call execution options of the entry points that contain a channel GEMM (the skip sum, the head convolutions, the
 * layers of widths other than 32/32/2, their backward) or need scratch memory.  The reference computes these contractions
 * in fp32 (cuDNN / cuBLAS under Chainer); here
 *   WN_GEMM_FP32    fp32-input MFMA                                        (exact fp32 products)
 *   WN_GEMM_BF16X3  every operand split into three bf16 parts, six products (fp32-accurate; what NULL selects)
 *   WN_GEMM_BF16    operands rounded to bf16 once, fp32 accumulation
 *   WN_GEMM_FP16X2  the skip contraction and its two backward GEMMs: operands scaled by a power of two and split into two
 *                   fp16 parts, three products (fp32-accurate to 2^-21 at half the matrix work of BF16X3).  tanh*sigmoid
 *                   outputs use a fixed scale (|z| <= 1); weights and gradients the power of two that fits their absolute
 *                   maximum, measured on the device by one small extra pass each (no host synchronisation; ABI 3: the
 *                   weights too -- a fixed 2^8 used to saturate weights above ~254).  The fused 32-channel layer kernels
 *                   run the same split products with per-tile scales taken from the wave's own maximum.  The head
 *                   convolutions keep the BF16X3 split.
 * Storage and accumulation stay fp32 in all of them; under FP32 / BF16X3 / BF16 the fused 32-channel layer kernels multiply
 * in exact fp32 (v_mfma_f32_32x32x2_f32).
 * ws / ws_bytes: device scratch, at least wn_exec_workspace_bytes() for the model and batch; its contents are dead when the
 * call's kernels have run, so ONE buffer per stream serves every call on that stream (never one buffer for two streams).
 * flags (ABI 3; the library reads NO environment variable and keeps no switch of its own -- what used to be
 * WAVENET_HIP_FORCE_GENERIC / _FWD_T1_MIN_BLOCKS inside the .so are per-call fields here):
 *   WN_EXEC_FORCE_GENERIC   every kernel of the call from the any-shape correctness path (generic_kernels.hip), fp32
 *   WN_EXEC_BIAS_PER_CLIP   wn_layer_* / wn_stack_*: one row of gate biases per clip (global conditioning; see the define)
 *   WN_EXEC_NO_FWD_GROUPS, WN_EXEC_NO_PIPELINED_GEMM, WN_EXEC_NO_MULTI_LAYER_BWD   see the defines
 *   WN_EXEC_HEAD_ROW_NLL    wn_head_xent only: per-row negative log-likelihoods instead of the gradient (see there)
 * fwd_t1_min_blocks: launch size (workgroups of four 32-column tiles) from which the fused 32-channel layer forward takes its
 * one-tile-per-wave form; 0 = the library's default (512: every CU gets two to four workgroups), n > 0 = n (1 = always:
 * parity tests of that kernel at small sizes), < 0 = never.
 * plan (ABI 5): a step plan or NULL ("step plan" at the end of this header).
 * ex == NULL means { WN_GEMM_BF16X3, 0, NULL, 0, 0 }: fine for calls that need no scratch, WN_EARG (with the byte count)
 * otherwise. */
enum { WN_GEMM_FP32 = 0, WN_GEMM_BF16X3 = 1, WN_GEMM_BF16 = 2, WN_GEMM_FP16X2 = 3 };
#define WN_EXEC_FORCE_GENERIC 1u
#define WN_EXEC_BIAS_PER_CLIP 2u   /* Global conditioning (van den Oord et al. 2016, eq. 3: z = tanh(Wf*x + Vf h) sigmoid(Wg*x + Vg h), h one
                                      vector per clip): to a layer Vf h / Vg h are a convolution bias that is constant over time
                                      and differs from clip to clip.  Honoured by wn_layer_fwd / wn_layer_bwd / wn_stack_fwd /
                                      wn_stack_bwd; every other entry point ignores the bit.  WnExec.reserved is then the stride,
                                      in floats, between consecutive clips' rows:
                                        forward   bf / bg (per layer: bf[l] / bg[l]) point at clip 0's row of cd floats, clip b
                                                  reads ptr + b * stride; bp / bs stay per channel.  The zero prefix is
                                                  unchanged: for t < Z neither the convolution nor the bias contributes.
                                        backward  dbf / dbg (dbf[l] / dbg[l]) point at clip 0's row; row b is accumulated (+=)
                                                  with the sums of da[b, t, :] / dg[b, t, :] over t >= Z of that clip only.  One
                                                  launch per layer writes both gates (k_colsum_per_clip: a fixed summation
                                                  order -- the order of the shared-bias column sums of a B = 1 call --, no float
                                                  atomics, no scratch: bit-reproducible from run to run).
                                      WN_EARG before any device work: stride < cd, a NULL bf / bg (forward) or dbf / dbg
                                      (backward) entry.  The fp16 x 2 stack forward loads a lane's bias values as float4: there
                                      the stride must be a multiple of 4 floats and the rows 16-byte aligned (WN_EARG with a
                                      message otherwise, never another path); it adds them in fp32 AFTER the accumulator is
                                      rescaled -- they never pass through the power-of-two tile scale -- and runs every layer as
                                      its own launch, as under WN_EXEC_NO_FWD_GROUPS.  The stack backward takes the per-layer
                                      path (bias-gradient tables always do), so wn_stack_saves_tanh is 1.  wn16_* (bf16 storage)
                                      takes rows through the descriptor alone (WN16_BWD_ROW_GRADS).  A step plan holds
                                      weight images only, never a bias pointer.
                                      Local conditioning (eq. 4 with y = the features repeated over time): wn_stack_fwd /
                                      wn_stack_bwd read three trailing WnStackDesc fields under this flag.  bias_hop = h > 0
                                      turns clip b's row into a block of n = ceil((T + bias_phase) / h) rows: bf[l] / bg[l]
                                      point at (clip 0, frame 0), clip b's block starts b * WnExec.reserved floats on, frame
                                      f lies f * bias_frame_stride floats on inside the block, and position t of every clip
                                      -- t counted inside the call's T columns, whatever t_off / window_only say -- reads
                                      frame (t + bias_phase) / h.  For t < Z neither the convolution nor the bias counts.
                                        backward  dbf[l] / dbg[l] point at (clip 0, frame 0) of a gradient block of the same
                                                  geometry; row (b, f) is accumulated (+=) with the sums of da[b, t, :] /
                                                  dg[b, t, :] over the t >= Z of clip b that read frame f
                                                  (k_colsum_per_frame: one launch per layer, a workgroup per 64 columns of a
                                                  (clip, frame) segment, a fixed order, no float atomics, no scratch; a
                                                  segment that covers a whole clip adds exactly what the per-clip form
                                                  adds).  Rows of frames wholly below Z are not touched.  The path is the one
                                                  per-clip rows select: nothing is order-dependent.
                                      WN_EARG before any device work: bias_hop < 0; bias_phase outside [0, bias_hop);
                                      T + bias_phase beyond 32 bits; bias_frame_stride below a layer's cd;
                                      reserved < n * bias_frame_stride; bias_hop > 0 without the flag; on the fp16 x 2 path rows that are not 16-byte aligned or a clip /
                                      frame stride that is no multiple of 4 floats (refused, never sent down another path).
                                      bias_hop == 0: the other two fields are ignored.  wn_layer_fwd / wn_layer_bwd take no
                                      descriptor and keep per-clip rows only; wn16_*: see WN16_BWD_ROW_GRADS.
                                      Linear interpolation between frames (WnStackDesc.bias_interp = 1; 0, the default, is
                                      the above, unchanged): row k is ANCHORED at the first position of its frame, k * h --
                                      the alignment rule above is untouched, a value is reached exactly at its frame's first
                                      sample and the next frame's is approached over the frame.  With p = t + bias_phase,
                                      j = p / h and alpha = float32(p % h) / float32(h), position t reads
                                          y(t) = r[j] + alpha * (r[j + 1] - r[j])
                                      three separately rounded fp32 operations in every kernel, so equal neighbours and
                                      alpha = 0 give r[j] bit for bit.  The last position reads row j + 1 too: a block holds
                                      n + 1 rows and WN_EARG is returned for reserved < (n + 1) * bias_frame_stride -- the
                                      library never clamps.  On the fp16 x 2 path the interpolated value is formed in fp32
                                      and added where the per-frame one is: behind the rescale.
                                        backward  row (b, f), f = 0 .. n, is accumulated (+=) with the sum of
                                                  (1 - alpha_t) d[b, t, :] over the t >= Z of frame f plus the sum of
                                                  alpha_t d[b, t, :] over the t >= Z of frame f - 1, d = da and dg
                                                  (k_colsum_per_frame_lerp: one launch per layer, a workgroup per 64 columns
                                                  of a (clip, row); the first segment on reduction lanes 0 .. 7, the second
                                                  on lanes 8 .. 15, chunks of 32 rows in ascending order, the 16 partials in
                                                  index order; no float atomics, no scratch, bit-reproducible).
                                                  A row whose two segments hold no t >= Z is not touched.
                                      WN_EARG before any device work: bias_interp outside {0, 1}; bias_interp != 0 with
                                      bias_hop == 0
                                      A phase per clip (WnStackDesc.bias_phase_tab != NULL; NULL, the default, is all of the
                                      above, the same kernels and the same bits): a device array of B int32, read when the
                                      kernels run -- one captured step serves crops that start at any sample.  Position t of
                                      clip b uses p = t + bias_phase_tab[b] wherever it used t + bias_phase: the frame index
                                      p / h and, with bias_interp = 1, alpha = float32(p % h) / float32(h).  Row layout and
                                      strides are unchanged; the per-frame column sums of the backward add, for a clip of
                                      phase p, exactly the rows in exactly the chunks a bias_phase = p call adds.  The host
                                      cannot see the values, so the geometry is sized for the worst phase h - 1: a clip's
                                      block (and its gradient block) holds n_max = ceil((T + h - 1) / h) rows, one more with
                                      bias_interp = 1, and WN_EARG is returned for reserved < n_max * bias_frame_stride.
                                      Rows that no position of a clip reads are neither read nor written.  The caller passes
                                      values in [0, h).  As a FENCE, not a feature, every kernel reduces the value it reads
                                      to (unsigned) v % h -- once per tile or workgroup where the clip is uniform -- so a
                                      garbage value cannot take an access outside the clip's block.
                                      WN_EARG before any device work, each naming bias_phase_tab: a table with bias_hop == 0;
                                      a table without the flag; a table together with bias_phase != 0 (ambiguous); a pointer
                                      that is not 4-byte aligned; T + bias_hop - 1 beyond 32 bits */
#define WN_EXEC_NO_FWD_GROUPS 4u   /* fp16x2 stack forward: every layer its own launch (no k_layer_fwd_h2_grp); same results,
                                      bit for bit -- A/B timing and the parity tests of the per-layer kernel */
#define WN_EXEC_NO_PIPELINED_GEMM 8u /* fp16x2 skip contractions (skip sum, dz, dWs): the older kernels (k_colgemm_b3,
                                        k_wgrad_b3w) instead of k_colgemm_h2q / k_dz_ws / k_wgrad_h2p; same results, bit for
                                        bit -- A/B timing, parity tests */
#define WN_EXEC_NO_MULTI_LAYER_BWD 16u /* fp16x2 chained stack backward: one launch per layer instead of the multi-layer
                                          launch (k_layer_bwd_chain_multi).  That launch has NO grid barrier: co-resident
                                          workgroups follow one dataflow word per 32-column tile ("layers completed"),
                                          (V, U) rotate through three buffer pairs, the deal of tiles to waves rotates from
                                          layer to layer.  Results agree with the per-layer launches to fp32 summation order
                                          (which wave sums which tiles; ~1e-7) and are bit-reproducible from run to run */
#define WN_EXEC_HEAD_ROW_NLL 32u /* wn_head_xent: the scoring form -- its sixth argument receives N floats, one negative
                                    log-likelihood per row, and no gradient is formed or stored.  Every other entry point
                                    ignores the bit */
typedef struct WnExec {
    int precision;
    unsigned flags;
    void* ws;
    size_t ws_bytes;
    int fwd_t1_min_blocks;
    int reserved;                     /* WN_EXEC_BIAS_PER_CLIP: floats between consecutive clips' bias rows; ignored otherwise */
    void* plan;                       /* ABI 5: a step plan (wn_plan_create) or NULL -- see "step plan" below */
} WnExec;
/* 1 if the fused MFMA kernels cover this residual-layer shape (a pure shape query; a call with WN_EXEC_FORCE_GENERIC
 * runs the generic kernels whatever this says), 0 if the generic / wide paths run */
int wn_layer_fast_path(int Cr, int Cd, int fw);

/* ---- A10: first causal layer on integer tokens (data.py:61-68 one-hot + wavenet.py:298-301) ----
 * out[b,t,:] = sum_k W[:, idx[b, t-(fw-1-k)], k]  (+bias), taps with t-(fw-1-k) < 0 contribute 0.
 * Equals DilatedConvolution1D(d=1) applied to onehot_pixel_image(idx).                        */
int wn_embed_fwd(const int32_t* idx, const float* W, const float* bias, float* out,
                 int B, int T, int Q, int C, int fw, void* stream);
/* dW[o][q][k] += sum over (b,t) with idx[b,t-(fw-1-k)] == q of dout[b,t,o]; dbias += sum dout. */
int wn_embed_bwd(const int32_t* idx, const float* dout, float* dW, float* dbias,
                 int B, int T, int Q, int C, int fw, const WnExec* ex, void* stream);

/* ---- A5: dense dilated causal convolution, any shape (DilatedConvolution1D.__call__,
 * wavenet.py:294-342):  out[b,t,o] = sum_k sum_c W[o,c,k] x[b, t-(fw-1-k)d, c] + bias[o] for
 * t >= Z, 0 for t < Z.  Used for dense (non one-hot) inputs and for extra causal layers.       */
int wn_conv_fwd(const float* x, const float* W, const float* bias, float* out,
                int B, int T, int Cin, int Cout, int fw, int d, int Z, void* stream);
/* dx (overwritten, may be NULL), dW / dbias (accumulated, may be NULL). */
int wn_conv_bwd(const float* x, const float* W, const float* dout, float* dx, float* dW, float* dbias,
                int B, int T, int Cin, int Cout, int fw, int d, int Z, void* stream);

/* ---- A7: fused residual layer (ResidualConvLayer.__call__, wavenet.py:358-368) -------------
 *   a = conv(x; Wf,bf,d,Z)  g = conv(x; Wg,bg,d,Z)   z = tanh(a) * sigmoid(g)
 *   out = Wp z + bp + x
 * z (B,T,Cd) is always written: the skip projection Ws z is deferred to wn_skip_sum_fwd (one
 * contraction over all layers instead of L read-modify-write passes over a (B,T,Cs) tensor).
 * f_save / g_save (B,T,Cd), when non-NULL, receive tanh(a) and sigmoid(g) for wn_layer_bwd.    */
int wn_layer_fwd(const float* x,
                 const float* Wf, const float* bf, const float* Wg, const float* bg,
                 const float* Wp, const float* bp,
                 float* out, float* z, float* f_save, float* g_save,
                 int B, int T, int Cr, int Cd, int fw, int d, int Z, const WnExec* ex, void* stream);

/* Backward of one layer (Chainer autograd through wavenet.py:358-368).
 *   dz = Wp^T dout + dz_skip      da = dz g (1-f^2)      dg = dz f g (1-g)     (0 for t < Z)
 *   dWp += dout z^T  dbp += dout   dWf_k += da x[t-(fw-1-k)d]^T  dbf += da   (same for g)
 *   dx[t] = dout[t] + sum_k (Wf_k^T da + Wg_k^T dg)[t + (fw-1-k)d]
 * dz_skip (B,T,Cd) is this layer's slice of Ws^T dskip (wn_skip_sum_bwd_dz); NULL = none.
 * dout NULL = zero (the last layer's residual output is discarded, train_audio/train.py:72).
 * dab_ws is caller-provided scratch of wn_layer_bwd_workspace_floats() floats ((da,dg) for every
 * column, plus per-workgroup partial weight-gradient tiles on the MFMA path).  dWp/dbp may be
 * NULL (last layer).                                                                            */
size_t wn_layer_bwd_workspace_floats(int B, int T, int Cr, int Cd, int fw);
int wn_layer_bwd(const float* x, const float* f, const float* g,
                 const float* Wf, const float* Wg, const float* Wp,
                 const float* dout, const float* dz_skip,
                 float* dx, float* dWf, float* dbf, float* dWg, float* dbg, float* dWp, float* dbp,
                 float* dab_ws,
                 int B, int T, int Cr, int Cd, int fw, int d, int Z, const WnExec* ex, void* stream);

/* ---- 1x1 convolution with the activation the reference applies BEFORE it -------------------
 * out[n,:] = W act(x[n,:]) + b.   Head layers (wavenet.py:587-590: relu then conv; elu in
 * faster_wavenet.py:107-110), projection_block / projection_softmax with WN_ACT_NONE.           */
int wn_pointwise_fwd(const float* x, const float* W, const float* bias, float* out,
                     int N, int Cin, int Cout, int act, const WnExec* ex, void* stream);
/* dx[n,:] = act'(x[n,:]) * (W^T dout[n,:]) (overwritten; NULL to skip);  dW += dout act(x)^T;
 * dbias += sum dout. */
int wn_pointwise_bwd(const float* x, const float* W, const float* dout, float* dx, float* dW,
                     float* dbias, int N, int Cin, int Cout, int act, const WnExec* ex, void* stream);

/* ---- A11: the skip sum, deferred:  skip[b,t,:] = sum_l (Ws_l z_l[b, t_off+t, :] + bs_l) ------
 * (wavenet.py:574-582: sum_skip_connections += projection_softmax, all blocks, all layers).
 * z[l] is (B,T,cd[l]); skip is (B,Tw,Cs) for columns t_off .. t_off+Tw-1 (the harness keeps
 * only the last train_width columns, train_audio/train.py:73).  accumulate != 0 adds to skip.  */
int wn_skip_sum_fwd(int L, const float* const* z, const float* const* Ws, const float* const* bs,
                    const int* cd, float* skip, int B, int T, int t_off, int Tw, int Cs,
                    int accumulate, const WnExec* ex, void* stream);
/* dz[l][b,t,:] = Ws_l^T dskip[b,t-t_off,:] for t >= t_off, 0 before (dz[l] is (B,T,cd[l])). */
int wn_skip_sum_bwd_dz(int L, const float* const* Ws, const int* cd, const float* dskip,
                       float* const* dz, int B, int T, int t_off, int Tw, int Cs, const WnExec* ex, void* stream);
/* dWs[l] += dskip^T z_l (Cs x cd[l]);  dbs[l] += sum dskip  (either table entry may be NULL). */
int wn_skip_sum_bwd_dw(int L, const float* const* z, const int* cd, const float* dskip,
                       float* const* dWs, float* const* dbs, int B, int T, int t_off, int Tw, int Cs,
                       const WnExec* ex, void* stream);

/* ---- A11 + A15 as one call each: the reference's per-layer Python loop (wavenet.py:572-582 and
 * Chainer's backward over it) executed inside the library on one stream.                        */
typedef struct WnStackDesc {
    int n_layers, Cr, Cs, fw;              /* n_layers = blocks * layers per block                */
    const int* cd;                         /* host, per layer: gate width                          */
    const int* dilation;                   /* host, per layer: fw ** layer_index (wavenet.py:429)  */
    /* host arrays (n_layers) of device pointers; bias tables or entries may be NULL             */
    const float* const* Wf; const float* const* bf; const float* const* Wg; const float* const* bg;
    const float* const* Wp; const float* const* bp; const float* const* Ws; const float* const* bs;
    const int* bias_phase_tab;             /* NULL (the default): bias_phase below holds for every clip.  Else a DEVICE pointer to B
                                              int32 values, the phase of clip b, read when the kernels run: position t of clip b
                                              uses p = t + bias_phase_tab[b] wherever it used t + bias_phase (see the define).
                                              Declared ahead of the local-conditioning group; descriptors are filled by field name */
    /* local conditioning (read only under WN_EXEC_BIAS_PER_CLIP -- see the define; all 0 = one row per clip) */
    int bias_interp;                      /* 0: position t reads its frame's row; 1: linear interpolation towards the next row
                                              (declared at the head of the group; descriptors are filled by field name)         */
    int bias_hop;                          /* > 0: a bias row per (clip, frame); position t reads frame (t + bias_phase) / bias_hop */
    int bias_phase;                        /* 0 <= bias_phase < bias_hop, one value per call (a phase per clip: bias_phase_tab
                                              above, and this field 0)                                                             */
    int bias_frame_stride;                 /* floats between consecutive frames' rows inside a clip's block (>= the layer's cd)    */
} WnStackDesc;
/* xs (n_layers,B,T,Cr) receives every layer's output (xs[n_layers-1] is the stack output); z, f, g
 * are layer-major (layer l at offset sum_{i<l} B*T*cd[i]); f/g NULL for inference; skip (B,T-t_off,Cs)
 * may be NULL.  The zero prefix is derived from T per layer when compat_zero_prefix != 0.
 * window_only != 0 (training, train_audio/train.py:72-73 keeps skip[t_off:] only and discards the residual
 * output): columns that cannot influence skip[t_off:] -- further below t_off than the layers above a layer
 * reach -- are not computed; xs / z / f / g are left untouched there and wn_stack_bwd must then be called
 * with dout == NULL.  Loss and gradients are unchanged.                                              */
/* 1 if wn_stack_bwd needs tanh saved (f); 0 if every layer runs on the fused 32-channel kernels without conv / projection
 * biases: then f may be NULL in both calls (only z and sigmoid are kept; tanh = z / sigmoid is recovered by the backward). */
int wn_stack_saves_tanh(const WnStackDesc* d, const WnExec* ex);
int wn_stack_fwd(const WnStackDesc* d, const float* x, float* xs, float* z, float* f, float* g,
                 float* skip, int B, int T, int t_off, int compat_zero_prefix, int window_only, const WnExec* ex, void* stream);
size_t wn_stack_bwd_workspace_bytes(const WnStackDesc* d, int B, int T);
/* Upper bound of the WnExec scratch any call on this model needs at batch (B, T): head_channels = softmax_conv_channels
 * (n entries), causal_channels / causal_fw describe the first causal layer (its gradient tables).  d may be NULL. */
size_t wn_exec_workspace_bytes(const WnStackDesc* d, int Q, int causal_channels, int causal_fw, const int* head_channels,
                               int n_head_channels, int B, int T);
/* dout: gradient of the last layer's output (NULL = unused, train_audio/train.py:72); dskip
 * (B,T-t_off,Cs): gradient of the skip sum (NULL = unused); dx (B,T,Cr) may be NULL.  Gradient
 * tables are host arrays of device pointers, accumulated into (the flat gradient arena).          */
int wn_stack_bwd(const WnStackDesc* d, const float* x, const float* xs, const float* z, const float* f,
                 const float* g, const float* dout, const float* dskip, float* dx,
                 float* const* dWf, float* const* dbf, float* const* dWg, float* const* dbg,
                 float* const* dWp, float* const* dbp, float* const* dWs, float* const* dbs,
                 float* ws, size_t ws_bytes, int B, int T, int t_off, int compat_zero_prefix, const WnExec* ex, void* stream);

/* ---- softmax over the channel axis (wavenet.py:592) and A14 (wavenet.py:597-617) ------------ */
int wn_softmax_fwd(const float* logits, float* prob, int N, int Q, void* stream);
/* loss[0] = sum over rows of -log softmax(logits[n])[target[n]] / n_norm (loss points at WN_XENT_LOSS_WORDS floats: the
 * rest holds per-workgroup sums that one workgroup adds in a fixed order -- no float atomics); dlogits (may be NULL) =
 * (softmax - onehot) / n_norm.  Rows are b*Tw + t, as after the reference's transpose(0,3,2,1) + reshape.  A row whose
 * target is -1 is ignored (no loss, zero gradient) as chainer.functions.softmax_cross_entropy does; so is any other target
 * outside [0, Q) -- nothing is read out of bounds.  n_norm = the number of rows that count (Chainer: labels != -1);
 * n_norm == 0 means N; n_norm < 0 (ABI 3): counted on the device from the labels (rows with a label in [0, Q), at least
 * 1), for targets the host never saw -- one extra small launch, no synchronisation.                                 */
#define WN_XENT_LOSS_WORDS 2056
int wn_softmax_xent(const float* logits, const int32_t* target, float* loss, float* dlogits, int N, int Q,
                    int64_t n_norm, void* stream);
/* ABI 4.  The LAST head convolution and the loss in ONE launch (wavenet.py:584-593 with apply_softmax = False followed by
 * wavenet.py:597-617): logits = W act(x) + b are formed and consumed on the chip -- they never reach memory --, dlogits (N, Cout)
 * receives d loss / d logits for an upstream gradient of 1 (what wn_softmax_xent writes), loss as for wn_softmax_xent
 * (WN_XENT_LOSS_WORDS floats, n_norm with the same meaning).  Covered: WN_GEMM_FP16X2, Cout = 256, Cin a multiple of 32
 * and N <= 253,952 rows -- one 128-row workgroup per partial-sum slot of `loss` -- (wn_head_xent_supported, which takes N since
 * ABI 5; WN_ESHAPE otherwise: run wn_pointwise_fwd + wn_softmax_xent, which has no row limit).  The input has no known range: every
 * 32-channel chunk of a wave's 32 columns is scaled by the power of two that fits the wave's own maximum before the fp16 split
 * (error <= 2^-21 per product as elsewhere under FP16X2).  Backward: wn_pointwise_bwd(x, W, dlogits, ...) as after the two calls.
 * Scoring form (ex->flags & WN_EXEC_HEAD_ROW_NLL; same coverage, same WN_ESHAPE before any device work): the sixth argument
 * points at N floats and receives row_nll[n] = m + log sum exp(l - m) - l[target[n]] (m = the row's largest logit; what
 * wn_softmax_xent sums), NOT divided by n_norm, and exactly 0.0f for a row whose target lies outside [0, Cout).  No gradient is
 * formed or stored and nothing beyond those N floats is written; loss is filled as in the training form (loss[0] = the mean
 * over the rows that count, n_norm with its three meanings), so a caller can check the rows against the mean. */
int wn_head_xent_supported(int64_t N, int Cin, int Cout, const WnExec* ex);
int wn_head_xent(const float* x, const float* W, const float* bias, const int32_t* target, float* loss, float* dlogits,
                 int N, int Cin, int Cout, int act, int64_t n_norm, const WnExec* ex, void* stream);

/* x[i] *= *scale_dev (a device scalar), and nothing at all when *scale_dev == 1: the backward of the loss node
 * (chainer's softmax_cross_entropy backward multiplies by the upstream gradient, which is 1 for `loss.backward()`).  */
int wn_scale_by_dev(float* x, const float* scale_dev, int64_t n, void* stream);

/* ---- layout conversion at the boundary: (B,C,1,T) T-contiguous <-> (B,T,C) ------------------ */
int wn_nchw_to_btc(const float* src, float* dst, int B, int C, int T, void* stream);
int wn_btc_to_nchw(const float* src, float* dst, int B, int C, int T, void* stream);

/* ---- A16/A17: queue-cached autoregressive decoder (faster_wavenet.py:50-113) -----------------
 * Persistent per-layer state in HBM: a ring of (fw-1)*d input columns per residual layer (and
 * per extra causal layer) instead of the reference's full-window caches that are rolled every
 * step; the head runs on the newest column only.                                               */
#define WN_DECODER_ONE_WORKGROUP 64u
/* WnDecoderDesc.flags: on a description that is otherwise of the specialised decoder's shape (config 4's: Q = 256, one causal
 * layer of filter width 2, 32 / 32 / 256 channels, filter width 2, head 256 -> 256, at most 128 layers), gate biases (bf[j] /
 * bg[j], both or neither per layer; a layer without them adds 0) and / or a frame table do NOT deselect that decoder: the
 * handle runs k_decode_fast / k_decode_fast3 / k_decode_fast3_batch, and only wave 1 of the chain workgroup changes -- the
 * wave that runs ahead of the layer chain and forms the x[n-d] half of every gate row.  For step k of a launch, p = pos0 + k,
 * j = p / frame_hop, alpha = float32(p % frame_hop) / float32(frame_hop), lane `lane` of flat layer l starts its accumulator at
 * (static bias or 0) + y with y = r[j][64 l + lane] (repeat) or r[j] + alpha * (r[j + 1] - r[j]) (linear: three separately
 * rounded fp32 operations, WnStackDesc.bias_interp's rule); the row is fetched one layer ahead like the weights, nothing is
 * added to the chain wave, the skip workgroups or the exchange between workgroups, and a table of zeros changes no bit.
 * Without the flag every call does what it did before the flag existed (such a description gives an any-shape handle); bp, bs,
 * a causal bias and WN_EXEC_FORCE_GENERIC deselect the specialised decoder with or without it, and on a description of any
 * other shape the flag is ignored.  A handle's form is fixed at create: wn_decoder_update_weights on a flagged handle takes new
 * gate biases (or none), a new table, another one or none, and a description whose flag differs from the handle's is WN_EARG
 * before any device work.  The frame-table rules (refusals, messages, the step counter shared with step_limit, "nothing
 * clamps") are the any-shape decoder's.  wn_decoder_run_batch on flagged handles is the nine-workgroup form with its rules
 * (28 utterances, n >= 2, n_u >= 2) and the any-shape form's agreement on having a table, frame_hop and frame_interp; under
 * same_weights != 0 the utterances share handle 0's packed weights, while every utterance's static gate biases and table
 * rows come from its OWN handle -- they are not part of the shared weights, and the same_weights check does not look at a
 * flagged handle's bf / bg pointers, so utterances of different classes (speakers) and different tables share one copy.
 * The specialised kernels sum a gate row in another order than the any-shape decoder: probabilities agree to rounding, and
 * a conditioned model's sampled tokens can differ from the any-shape decoder's at a near-tie of the cumulative distribution
 * (as for WN_DECODER_ONE_WORKGROUP); each form is deterministic. */
#define WN_DECODER_GATE_ROWS 128u
/* WnDecoderDesc.flags, on every shape: the handle's probability trace is the probability of each token it emits -- ONE float per
 * step instead of a row of Q.  wn_decoder_run: prob_trace, when not NULL, points at n floats; element i receives the fp32
 * probability of out_tokens[i] exactly as the row the draw consumed held it (post-temperature; top-k / top-p leave a kept
 * entry's value untouched and the drawn token is a kept entry) -- the very float an unflagged handle in the same state writes to
 * prob_trace[i * Q + out_tokens[i]].  The fallback at the end of the cumulative distribution (token Q - 1) reports whatever that
 * entry holds then, 0.0f included; nothing is clamped.  wn_decoder_run_batch: prob_traces[u] is n_u floats (elements n_u .. n are
 * not written), and all handles of a launch must agree on the flag (WN_EARG naming the first utterance that differs, before any
 * device work).  The flag never changes which decoder a description selects, nor a token: a flagged and an unflagged handle in
 * the same state, given the same uniforms, emit the same tokens bit for bit.  wn_decoder_step is not affected.  A handle's
 * form is fixed at create: wn_decoder_update_weights with a description whose bit differs from the handle's is WN_EARG before
 * any device work (the WN_DECODER_GATE_ROWS rule; the two bits and WN_DECODER_ONE_WORKGROUP combine freely).  In the kernels the
 * thread that owns the drawn token stores its entry with one ordinary store per step; the full-row write and this one exclude
 * each other per launch.  Without the flag every call does what it did before the flag existed. */
#define WN_DECODER_TRACE_CHOSEN 256u
/* WnDecoderDesc.flags, on every shape: the handle keeps the samples it is given and draws the rest.  out_tokens of wn_decoder_run
 * (out_tokens[u] of wn_decoder_run_batch) is READ BEFORE IT IS WRITTEN: with f = out_tokens[i] on entry,
 *   - 0 <= f < Q: step i emits f.  No truncation and no draw run; uniforms[i] has no effect (the array is still n doubles, and a
 *     NaN there is harmless); out_tokens[i] stays f; the token enters the rings and the next step exactly as a drawn one does;
 *   - any other value (-1 by convention): step i draws exactly as an unflagged handle does -- the row, the controls, uniforms[i],
 *     the token and the trace are the same, bit for bit.
 * The kernels decide with (unsigned)f < (unsigned)Q: a fence, so that a garbage buffer cannot index outside the embedding, not
 * a feature -- callers write -1 or a token.  There is no separate input buffer because no export, field or signature was free
 * to carry one; the buffer the run writes anyway is the one it reads.  The full-row trace is what it was: row i is the
 * post-temperature, pre-truncation row.  On a WN_DECODER_TRACE_CHOSEN handle element i of a given step is row_i[f] -- post-
 * temperature and never truncated, because the filter did not run; nothing is clamped, 0.0f is reported as 0.0f -- so a run
 * with every sample given is the decoder's own likelihood of those samples.  wn_decoder_run_batch: only elements [0, n_u) of
 * out_tokens[u] are read (and, as ever, written), and all handles of a launch must agree on the flag (WN_EARG naming the first
 * utterance that differs from utterance 0, before any device work, every handle's state and every buffer left alone).  A handle's
 * form is fixed at create: wn_decoder_update_weights with a description whose bit differs from the handle's is WN_EARG before
 * any device work.  The bit combines freely with WN_DECODER_GATE_ROWS, WN_DECODER_TRACE_CHOSEN and WN_DECODER_ONE_WORKGROUP
 * and never changes which decoder a description selects; wn_decoder_step is not affected.  In the kernels the entry is fetched
 * at the top of its step, off the layer chain, and a given step skips the sampler behind the network; the mode sits in
 * template instantiations of its own, so without the flag every call does what it did before the flag existed, and out_tokens
 * is write-only again. */
#define WN_DECODER_FORCED_TOKENS 512u
/* WnDecoderDesc.flags, on every shape: the frame table is a RING of R = n_frames rows in the caller's memory, read in place --
 * streaming synthesis: the caller keeps writing rows ahead of the decoder and runs the handle in pieces.
 *   - By reference.  frame_bias is NOT copied: the handle keeps the pointer, frame_stride and n_frames, and the kernels read the
 *     caller's memory when they run.  The caller keeps it alive until the handle is destroyed or updated with another ring, and
 *     writes rows only in the stream it runs the handle on: stream order is the only synchronisation.
 *   - Ring addressing.  Frame J (J = p / frame_hop, p = frame_phase + the steps run since the create / update call, as for the
 *     flat table) lives in row J mod R; with frame_interp = 1 the second row is (J + 1) mod R.  Everything else is the flat
 *     table's rule, bit for bit: (static bias or 0) + y, the interpolation, alpha, the layout of a row.
 *   - Which frames ARE in the ring is the caller's business: the flat table's refusal for reading past row n_frames - 1 does not
 *     apply, and no call can tell a row that was not refilled in time from one that was.  What is refused (WN_EARG, before any
 *     device work, the handle's state left alone) is a run of n steps that reads more than R frames -- frames p0 / hop ...
 *     (p0 + n - 1) / hop, one more with frame_interp = 1: a launch cannot be refilled while it runs.
 *   - The flag without frame_bias is WN_EARG.  The kernels read a row one float per lane, so frame_bias must be a multiple of
 *     4 bytes (sizeof(float)); frame_stride counts floats, and any stride >= the row width keeps every row so aligned.  A
 *     pointer that is not is WN_EARG at create / update, naming the 4 bytes.
 *   - A handle's form is fixed at create: wn_decoder_update_weights with the bit flipped is WN_EARG; with the bit kept it may
 *     bring another ring, R, phase or step limit, and restarts the step count as ever.
 *   - wn_decoder_run_batch: the handles of a launch agree on the flag (WN_EARG naming the first utterance that differs from
 *     utterance 0); pointer, R, position and phase are per utterance.
 * The bit combines freely with WN_DECODER_GATE_ROWS, WN_DECODER_TRACE_CHOSEN, WN_DECODER_FORCED_TOKENS and
 * WN_DECODER_ONE_WORKGROUP and never changes which decoder a description selects.  In the kernels the wrap is a wave-uniform
 * compare on the walked row (specialised decoder: wave 1 of the chain workgroup, inside the gate-row instantiations) or
 * instantiations of its own (any-shape decoder); a handle created without the flag does exactly what it did before. */
#define WN_DECODER_FRAME_RING 1024u
typedef struct WnDecoderDesc {
    int Q, fw_causal, n_causal, fw, n_blocks, n_layers;  /* n_layers per block; dilation fw^l */
    int Cr, Cs, n_head;
    const int* causal_channels;       /* host, n_causal entries                                */
    const int* cd;                    /* host, n_layers entries (per layer index in a block)    */
    const int* head_channels;         /* host, n_head+1 entries: Cs, ..., Q                     */
    /* device pointers to weights in creation order (wavenet.py:461-472); biases may be NULL   */
    const float* const* causal_W; const float* const* causal_b;                 /* n_causal    */
    const float* const* Wf; const float* const* bf;                             /* blocks*layers */
    const float* const* Wg; const float* const* bg;
    const float* const* Wp; const float* const* bp;
    const float* const* Ws; const float* const* bs;
    const float* const* head_W; const float* const* head_b;                     /* n_head      */
    int head_act;                     /* WN_ACT_ELU for FasterWaveNet, WN_ACT_RELU for WaveNet  */
    unsigned flags;                   /* WN_EXEC_FORCE_GENERIC: never the specialised 32/256-channel decode kernel;
                                         WN_DECODER_GATE_ROWS (see the define): gate biases and a frame table do not
                                         deselect that kernel;
                                         WN_DECODER_TRACE_CHOSEN (see the define): prob_trace is one float per step, the
                                         emitted token's probability, on every shape;
                                         WN_DECODER_FORCED_TOKENS (see the define): out_tokens is read before it is written, and
                                         a step whose entry is a token emits it instead of drawing, on every shape;
                                         WN_DECODER_FRAME_RING (see the define): frame_bias is a ring of n_frames rows read in
                                         place, not a table the handle copies, on every shape;
                                         WN_DECODER_ONE_WORKGROUP: wn_decoder_run of that kernel on ONE workgroup instead of
                                         nine (the chain | eight workgroups of skip rows and their share of the logits):
                                         same products, another summation order for the skip rows and the logits --
                                         probabilities agree to ~1e-7, sampled tokens can differ at a near-tie of the
                                         cumulative distribution; each form is deterministic */
    /* A length per utterance (declared ahead of the local-conditioning group; descriptors are filled by field name).  Applied by
     * wn_decoder_create and wn_decoder_update_weights, as the frame table is.  0, the default: no limit -- every call executes
     * what it executed before the field existed.  Negative: WN_EARG before any device work.  L > 0: the handle runs at most L
     * steps since the create / update call that set it, counted by the ONE counter the frame table uses ("steps run since the
     * create / update call": that call sets both, and resets the count with or without a table).  wn_decoder_step and
     * wn_decoder_run never clamp: more steps than are left is WN_EARG before any device work, the handle's state left alone --
     * the rule of a frame-table overrun.  wn_decoder_run_batch clamps per utterance (see there).  wn_decoder_update_weights is
     * the one way to set a new limit (or to start the count again); it re-packs the weights, as it does for a new table. */
    int step_limit;
    /* Local conditioning (trailing fields; frame_bias == NULL: every decode kernel executes what it executed before).  Applied
     * by wn_decoder_create and wn_decoder_update_weights; the handle COPIES the table, as it copies weights.  frame_bias: a
     * device pointer to n_frames rows, frame_stride floats apart; inside a row flat layer l (block-major, as bf / bg are
     * ordered) holds its cd filter values at offset sum_{i<l} 2 cd_i, then its cd gate values.  The k-th step run on the handle
     * (k = 0, 1, ...) since the create / update call that set the table -- whichever of wn_decoder_step, wn_decoder_run or
     * wn_decoder_run_batch runs it -- adds row (frame_phase + k) / frame_hop to every layer's gate pre-activations, in fp32, on
     * top of the static bf / bg where those exist: per output (static bias or 0) + frame value, then the taps, so a table of
     * zeros changes no bit.  A run that would read past row n_frames - 1 is refused with WN_EARG before any device work (no
     * clamping).  Without WN_DECODER_GATE_ROWS a handle with a table is an any-shape one, as with biased layers (a handle created
     * WITHOUT one on config 4's shape runs the specialised kernels and refuses a table in wn_decoder_update_weights); with the
     * flag a description of config 4's shape gives a handle of the specialised kernels that takes tables (see the define).  An
     * update without a table drops it.  wn_decoder_run_batch: the handles must agree on having a table and on frame_hop; phase, row count and contents are
     * per utterance.
     * frame_interp = 1 (0, the default: the above, unchanged; read only with a table): linear interpolation, the rule of
     * WnStackDesc.bias_interp with rows anchored at the first step of their frame -- step k, p = frame_phase + k, j = p /
     * frame_hop, alpha = float32(p % frame_hop) / float32(frame_hop), adds (static bias or 0) + (r[j] + alpha * (r[j + 1] -
     * r[j])).  A run whose last step would read row j + 1 > n_frames - 1 is refused with WN_EARG and leaves the handle's
     * state alone; a value outside {0, 1} is refused; wn_decoder_run_batch also demands agreement on it. */
    int frame_interp;                 /* declared at the head of the group; descriptors are filled by field name */
    const float* frame_bias;
    int n_frames, frame_hop, frame_phase, frame_stride;
} WnDecoderDesc;

int wn_decoder_create(void** handle, const WnDecoderDesc* desc, void* stream);
int wn_decoder_destroy(void* handle);
/* re-copy the weights (after an optimiser step) */
int wn_decoder_update_weights(void* handle, const WnDecoderDesc* desc, void* stream);
/* Seed the rings from a full-window forward (faster_wavenet.py:13-47): tokens (W) are the window's
 * tokens, causal_out[i] is (1,W,C_i) and layer_in[j] (1,W,Cr) is the INPUT of residual layer j
 * (blocks*layers entries), all produced by the ordinary forward kernels over the same window.  */
int wn_decoder_load_state(void* handle, const int32_t* tokens, int W,
                          const float* const* causal_out, const float* const* layer_in, void* stream);
/* One step (FasterWaveNet._forward_one_step): consume `token` (the newest sample), advance all
 * rings, write the probabilities (or logits if apply_softmax == 0) of the next sample to prob (Q). */
int wn_decoder_step(void* handle, int32_t token, float* prob, int apply_softmax, void* stream);
/* n steps entirely on device (train_audio/generate.py:24-43 with --fast): each step consumes the
 * previous token, computes p, draws with numpy's algorithm from uniforms[i] (float64 cumsum,
 * normalise, searchsorted right) and appends.  first_token is the newest token of the window the
 * state was loaded from plus one draw, i.e. the token emitted by the prefill step.  out_tokens (n)
 * receives the n emitted tokens; prob_trace (n*Q; n on a WN_DECODER_TRACE_CHOSEN handle) is optional.
 * On a WN_DECODER_FORCED_TOKENS handle out_tokens is an input as well: see the define. */
int wn_decoder_run(void* handle, int32_t first_token, const double* uniforms, int n,
                   int32_t* out_tokens, float* prob_trace, void* stream);
/* ABI 4.  n_handles independent utterances in ONE launch (generate.py:9-60 is batch 1 with a strict sample-to-sample
 * dependency, wavenet.py:286,290,354: a single utterance can use 9 of the GPU's 256 CUs at most -- the rest can only run OTHER
 * utterances; SURVEY 8(e) "replicas only", on one GPU).  Every handle is a decoder of its own (wn_decoder_create +
 * wn_decoder_load_state: its rings, its packed weights, its wn_decoder_set_sampling), all of the same model shape; uniforms[u]
 * (n doubles), out_tokens[u] (n) and the optional prob_traces[u] (n * Q; the array itself may be NULL) are device pointers held
 * in HOST arrays, first_tokens is a host array.  The utterances share nothing: an utterance's tokens and probability trace are
 * those of its own wn_decoder_run on the same handle with the same uniforms, bit for bit, and every handle's step counter
 * advances by n.  Handle 0 chooses between two forms, and all handles must be of its form (WN_ESHAPE otherwise):
 *   - nine workgroups per utterance: handles of the specialised decoder (config 4's shape, no WN_EXEC_FORCE_GENERIC; with
 *     WN_DECODER_GATE_ROWS also such handles with gate biases and / or a frame table, which must agree on having a table, on
 *     frame_hop and on frame_interp, and whose gate biases and rows stay per utterance under same_weights).  At most
 *     wn_decoder_batch_max() (28) utterances, 9 * n_handles workgroups must fit the device's CUs (WN_ESHAPE otherwise), and
 *     n >= 2.  same_weights != 0 is the caller's word that every handle was created from (and updated with) the SAME weights:
 *     all utterances then read handle 0's packed weights (one copy through the L2s instead of n_handles; each keeps its own
 *     state) -- same tokens, higher rate.  wn_decoder_status(handle) reports per utterance as after wn_decoder_run.
 *   - one workgroup per utterance: handles of the any-shape decoder (every other shape, or WN_EXEC_FORCE_GENERIC).  At most
 *     WN_DECODER_BATCH_MAX_ANY utterances, n >= 1; the workgroups never wait for each other, so nothing has to be resident
 *     and wn_decoder_status stays "synchronise, WN_OK".  The handles must agree in Q, channels, filter widths, every layer's
 *     dilation and width, and head activation.  same_weights is checked as above and otherwise ignored: each utterance
 *     reads its own packed weights.  The per-utterance arguments travel in a device table owned by handle 0, allocated at
 *     the first call and grown only by a larger batch: a repeated call allocates nothing and waits on the host only for the
 *     previous call's table copy (not its launch) before it rewrites the pinned image of the table.
 * A handle created with WN_DECODER_ONE_WORKGROUP is refused (WN_ESHAPE): that kernel has no batched form.  Every refusal
 * comes before any device work.
 * WN_DECODER_TRACE_CHOSEN: the trace's form is the launch's, so the handles must all carry the flag or all lack it (WN_EARG
 * naming the first utterance that differs from utterance 0, every handle's state left alone); with it prob_traces[u] is n_u
 * floats -- the probability of each token utterance u emitted -- instead of n_u rows of Q.
 * A length per utterance (WnDecoderDesc.step_limit).  Utterance u runs n_u = min(n, left_u) steps, left_u = its handle's
 * step_limit minus the steps run since the create / update call that set it (the counter the frame table shares), or n without a
 * limit; handles with and without a limit may share a launch.  Everything per utterance uses n_u: the frame-table check, the
 * step-counter overflow check, the advance of the handle's counters; uniforms[u] needs n_u doubles; out_tokens[u][n_u .. n) and
 * rows n_u .. n of a probability trace are NOT written; the first n_u tokens and rows are those of the utterance's own
 * wn_decoder_run(..., n_u, ...), bit for bit.  WN_EARG before any device work, the message naming the utterance: a handle with
 * left_u == 0 (the caller leaves finished utterances out), and on the nine-workgroup form a handle whose limit leaves it n_u < 2.
 * In the kernels the count is a word of the utterance's entry (read by all nine workgroups of its group; by its one workgroup
 * in the any-shape form); the batched kernels take NO launch-wide step count any more -- n remains the host-side bound of the
 * checks.  With every n_u == n a launch computes what it computed before.  same_weights != 0: an utterance 0 that ends first
 * leaves its packed weights in place, and the others keep reading them.  wn_decoder_status is unchanged.
 * Utterance tiles.  The tile size is a property of a launch and travels in same_weights:
 *   same_weights | any-shape handles                                          | nine-workgroup handles
 *   0            | every utterance reads its own copy                         | every utterance reads its own copy
 *   1            | the claim is checked, own copies are read                  | one copy (handle 0's)
 *   2, 4, 8, 16  | workgroup g decodes utterances [gU, gU + U) of the launch  | treated as 1
 *                | (the last tile may be short), all reading handle 0's copy  |
 * Any other value is WN_EARG.  A tile shares handle 0's embedding, causal weights and biases, every layer's filter / gate and
 * projection weights and projection biases, and the head; an utterance keeps its own rings, token ring, static gate biases
 * (bf / bg: a class per utterance), frame table or ring with its phase, sampling controls, counters, uniforms and outputs --
 * so utterances of different speakers, features, phases, controls, prompts and lengths share a tile, and each one's tokens and
 * trace stay those of its own wn_decoder_run, bit for bit.  The claim is checked on a key of the weight pointers that leaves
 * bf / bg out, and every handle's arena layout (which biases exist included) must equal handle 0's: WN_EARG naming the
 * utterance.  A tile keeps U x (7 maxc + 16) floats in LDS, maxc the widest channel count of the model; a U beyond 150 KiB is
 * WN_ESHAPE, the message naming the largest U that fits (never clamped).  The limit of WN_DECODER_BATCH_MAX_ANY utterances per
 * launch and the agreement rules above are unchanged. */
#define WN_DECODER_BATCH_MAX_ANY 1024      /* utterances per launch of the one-workgroup-per-utterance form */
#define WN_DECODER_TILE_MAX 16             /* the largest tile: utterances per workgroup under same_weights = 2, 4, 8, 16 */
/* the limit of the nine-workgroup form (28) */
int wn_decoder_batch_max(void);
int wn_decoder_run_batch(void* const* handles, int n_handles, const int32_t* first_tokens, const double* const* uniforms, int n,
                         int32_t* const* out_tokens, float* const* prob_traces, int same_weights, void* stream);
/* ABI 4.  wn_decoder_run's default form runs on nine workgroups that hand values to each other through device memory and
 * therefore must all be resident.  The library uses the one-workgroup kernel by itself on a device with fewer than nine
 * CUs; what it cannot know in advance -- other work holding the CUs for seconds -- ends in a wait that GIVES UP after
 * ~1-2 s: no trap, no hang, the launch runs to its end, the HIP context survives, but the tokens of that run are void.
 * wn_decoder_status synchronises `stream` and returns WN_OK, or WN_ETIMEOUT when the last wn_decoder_run on this handle
 * gave up a wait (re-create the handle with WN_DECODER_ONE_WORKGROUP and decode again). */
int wn_decoder_status(void* handle, void* stream);
/* categorical draw with numpy's algorithm for n independent rows (generate.py:39) */
int wn_sample_categorical(const float* prob, const double* uniforms, int32_t* out, int n, int Q,
                          void* stream);
/* Sampling controls (an extension: train_audio/generate.py:39 draws from the raw softmax; ABI stays 5, new functions only).
 * Per row of fp32 probabilities p, all order-exact (integer ranks, float64 sums in index order):
 *   order:  j precedes i iff p[j] > p[i], or p[j] == p[i] and j < i; rank(i) = number of tokens preceding i;
 *   top-k:  pk[i] = rank(i) < top_k ? p[i] : 0                                     (top_k == 0 or >= Q: off)
 *   top-p:  total = sum pk, before(i) = sum of pk[j] over the j preceding i; keep i iff before(i) < top_p * total, the
 *           rank-0 token always                                                    (top_p == 1: off)
 *   draw:   excluded entries are 0.0f, kept entries keep their value (no renormalisation); then generate.py:39's draw as
 *           wn_sample_categorical makes it.  With both controls off the tokens ARE wn_sample_categorical's.
 * WN_EARG before any device work: NULL pointer, top_k < 0, top_p outside (0, 1] or NaN.  At most 8192 tokens per row
 * when a control is on (WN_ESHAPE).  wavenet_amd/sampling.py restates the rule in numpy. */
int wn_sample_categorical_filtered(const float* prob, const double* uniforms, int32_t* out, int n, int Q, int top_k,
                                   double top_p, void* stream);
/* The same controls inside the persistent decode kernels (generate.py:24-43 with --fast, every draw of it): state of the
 * handle, off at create (temperature 1, top_k 0, top_p 1), honoured by wn_decoder_run and -- per handle, so utterances of one
 * launch may differ -- by wn_decoder_run_batch.  Temperature: the fp32 logits are multiplied by 1.0f / temperature
 * (computed once, here, in fp32) in front of the fp32 softmax; prob_trace receives those post-temperature, pre-truncation
 * probabilities, the very values the truncation and the draw consume.  Whatever is off is skipped, not computed
 * neutrally: with all three off a run executes what it executed before the controls existed, bit for bit.
 * wn_decoder_step is NOT affected (it returns probabilities or logits; its caller draws).  WN_EARG: NULL handle, temperature
 * not finite or <= 0, top_k < 0, top_p outside (0, 1] or NaN. */
int wn_decoder_set_sampling(void* handle, float temperature, int top_k, double top_p);

/* ---- A2 on the device (optional path; data.py:18-23 and 37-43) --------------------------------------
 * Table lookups: lut65536[v + 32768] is the token of the int16 sample v, table[q] the sample value of token q;
 * both tables are built on the host with the reference's float64 formulas (wavenet_amd/data.py), so the device
 * results are the host's bit for bit.  Tokens outside [0, Q) are clamped on decode.                        */
int wn_mulaw_encode_pcm16(const int16_t* pcm, const int32_t* lut65536, int32_t* tokens, int64_t n, void* stream);
int wn_mulaw_decode(const int32_t* tokens, const float* table, float* out, int64_t n, int Q, void* stream);

/* ---- the step either side of backward ------------------------- */
/* out[0] = sum (grad*grad_mult + weight_decay*param)^2: the squared norm GradientClipping sees after the
 * WeightDecay hook (wavenet.py:175-199, 477-480).  out points at WN_SQNORM_WORDS floats: out[0] is ASSIGNED (no
 * zeroing by the caller), the rest holds per-workgroup partial sums that one workgroup adds in a fixed order -- no
 * float atomics, the norm (and with it the clipping rate) is bit-reproducible.  param may be NULL when weight_decay == 0. */
#define WN_SQNORM_WORDS 1040
int wn_sqnorm(const float* grad, const float* param, int64_t n, float grad_mult, float weight_decay,
              float* out, void* stream);
/* Chainer Adam with the reference's hooks folded in, in hook order:
 *   g = grad*grad_mult + wd*param;   g *= min(1, clip/sqrt(*sqnorm))  (sqnorm != NULL, clip > 0)
 *   m += (1-b1)(g-m); v += (1-b2)(g^2-v); param -= lr_t * m / (sqrt(v)+eps).
 * lr_t = alpha*sqrt(1-b2^t)/(1-b1^t) is computed by the host.
 * ABI 4: when sqnorm is given (clip > 0) and *sqnorm is not finite, the WHOLE update is skipped -- param, m and v keep
 * their values (every update rule below does the same).  A void gradient (a backward whose multi-layer launch gave up
 * a wait and flagged it with a NaN, an overflow) then costs one step instead of the optimiser state; under data
 * parallelism the all-reduce carries the NaN to every rank and every rank skips the same step.  The host can read the
 * word back whenever it likes (wavenet_amd: WaveNet.last_update_applied()).                        */
int wn_adam_step(float* param, const float* grad, float* m, float* v, int64_t n,
                 float lr_t, float beta1, float beta2, float eps, float weight_decay,
                 const float* sqnorm, float clip, float grad_mult, void* stream);
/* Eve (wavenet.py:10-79, the reference's own optimizer class and its only device code, the elementwise kernel at
 * 57-65): Adam's moments with the denominator d * sqrt(v) + eps.  d is the loss-feedback scalar the host maintains
 * (wavenet.py:27-44); hooks as in wn_adam_step.                                                                   */
int wn_eve_step(float* param, const float* grad, float* m, float* v, int64_t n,
                float lr_t, float beta1, float beta2, float eps, float d, float weight_decay,
                const float* sqnorm, float clip, float grad_mult, void* stream);
/* The same update with the step size read from device memory (*lr_t_dev) at execution time: a training step
 * captured once into a hipGraph is replayed with a fresh bias-corrected step size by writing that scalar.  */
int wn_adam_step_dev(float* param, const float* grad, float* m, float* v, int64_t n,
                     const float* lr_t_dev, float beta1, float beta2, float eps, float weight_decay,
                     const float* sqnorm, float clip, float grad_mult, void* stream);
/* The other update rules get_optimizer() names (wavenet.py:81-97; chainer.optimizers.SGD / MomentumSGD / AdaGrad /
 * AdaDelta / NesterovAG / RMSprop as Chainer publishes them), behind the same hooks as wn_adam_step:
 *   SGD          p -= lr g                                  MomentumSGD  v = hyper v - lr g; p += v
 *   AdaGrad      h += g^2; p -= lr g/(sqrt(h)+eps)          NesterovAG   v = hyper v - lr g; p += hyper^2 v - (1+hyper) lr g
 *   RMSprop      ms += (1-hyper)(g^2-ms); p -= lr g/(sqrt(ms)+eps)
 *   AdaDelta     msg += (1-hyper)(g^2-msg); dx = sqrt((msdx+eps)/(msg+eps)) g; msdx += (1-hyper)(dx^2-msdx); p -= dx
 * s1 = v / h / ms / msg, s2 = msdx (AdaDelta only, else NULL); hyper = momentum / alpha / rho.  lr_dev != NULL: the
 * learning rate is read from device memory at execution time (graph replay), `lr` is ignored.
 *
 * WN_RULE_EMA is no optimiser: it keeps an exponential moving average of the weights, one more elementwise pass over
 * the flat arena.  param = the average e (read and written), grad = the current weights w (read only), lr (or *lr_dev)
 * = the rate r = 1 - decay_t:
 *   e += r (w - e)        in fp32, as fma(r, w, fma(-r, e, e)): two roundings; r == 0 leaves e, r == 1 stores w exactly
 * s1, s2 (both may be NULL), hyper and eps are ignored.  weight_decay != 0 or grad_mult != 1 is WN_EARG: they are hooks
 * on a gradient, and w is not one.  A rate passed by value must be finite and lie in [0, 1], else WN_EARG; a rate read
 * from device memory is taken as it is.  sqnorm != NULL && clip > 0 does ONLY the skip of ABI 4 -- sqrt(*sqnorm) not
 * finite: nothing is written, so a step the optimiser skipped is a step the average skips -- and never scales w.    */
enum { WN_RULE_SGD = 0, WN_RULE_MOMENTUM_SGD = 1, WN_RULE_ADAGRAD = 2, WN_RULE_ADADELTA = 3, WN_RULE_NESTEROV = 4,
       WN_RULE_RMSPROP = 5, WN_RULE_EMA = 6 };
int wn_rule_step(int rule, float* param, const float* grad, float* s1, float* s2, int64_t n, float lr,
                 const float* lr_dev, float hyper, float eps, float weight_decay, const float* sqnorm, float clip,
                 float grad_mult, void* stream);

/* ======================================================================================================
 * bf16-storage path (BASELINE.json configs[4]: 128 residual / dilation channels, 512 skip channels): activations are
 * bfloat16 in HBM (uint16_t = raw bf16 bits, same (B, T, C) layout), every contraction accumulates in fp32 on
 * v_mfma_f32_32x32x16_bf16, the weights stay fp32 (master copy, gradients, optimiser) and are repacked into bf16
 * matrix-core operand images once per step.  Same reference operations as the fp32 entry points above
 * (ResidualConvLayer.__call__ wavenet.py:358-368, forward_residual_block 572-582, forward_softmax_block 584-593 and
 * their backward).  Covers: Cr = Cd = 128, filter width 2, Cs a multiple of 256, an even number of layers (<= 48), no
 * conv / projection biases (the reference default); wn16_supported() says whether a stack qualifies.
 * The forward keeps only each layer's output and z; tanh / sigmoid are recomputed by the backward.
 * ====================================================================================================== */
int wn16_supported(const WnStackDesc* d);
/* bf16 elements of the packed operand images of a stack (per-layer images + the skip matrix and its transpose) */
size_t wn16_pack_elems(const WnStackDesc* d);
int wn16_pack_stack(const WnStackDesc* d, uint16_t* pack, void* stream);
/* A10 on tokens, bf16 output (filter width 2) */
int wn16_embed_fwd(const int32_t* idx, const float* W, const float* bias, uint16_t* out, int B, int T, int Q, int C,
                   int fw, void* stream);
/* its gradient (the backward of data.py:61-68 + wavenet.py:298-301 on tokens): dW (C,Q,2) += one-hot(tokens)^T dout on
 * the matrix cores, dbias (C) += column sums or NULL; dout (B,T,128) bf16; 128 channels, 256 token values, filter width 2 */
size_t wn16_embed_bwd_workspace_bytes(int B, int T);
int wn16_embed_bwd(const int32_t* idx, const uint16_t* dout, float* dW, float* dbias, int B, int T, int Q, int C, int fw,
                   void* ws, size_t ws_bytes, void* stream);
int wn16_cvt_to_bf16(const float* src, uint16_t* dst, int64_t n, void* stream);     /* n % 8 == 0 */
int wn16_cvt_to_f32(const uint16_t* src, float* dst, int64_t n, void* stream);
/* Gate-bias rows in bf16 storage (conditioning).  wn16_* calls take no WnExec: the descriptor alone decides.  It has rows when
 * bf[l] and bg[l] are non-NULL for every layer AND bias_frame_stride > 0 (all NULL: unconditioned; non-NULL entries with
 * bias_frame_stride == 0 are static biases and refused; a mixture of NULL and non-NULL is WN_EARG; wn16_pack_stack ignores
 * rows).  bf[l] / bg[l] point at layer l's filter / gate row -- 128 floats, 16-byte aligned -- of (clip 0, frame 0);
 * bias_frame_stride (>= 128, a multiple of 4) is the number of floats between consecutive rows of a block.  bias_hop == 0: one
 * row per clip, clip b's row b * bias_frame_stride floats on.  bias_hop = H > 0: a row per (clip, frame); bias_phase,
 * bias_interp and bias_phase_tab mean what they mean under WN_EXEC_BIAS_PER_CLIP, and the value position t reads is formed by
 * the same arithmetic (the frame's row, or r[j] + alpha (r[j + 1] - r[j]) in three separately rounded fp32 operations; a table
 * value is fenced with (unsigned) v % H).  Clip blocks are DENSE: clip b's block starts b * n * bias_frame_stride floats on, n
 * the rows the call itself needs -- ceil((T + worst phase) / H), one more with bias_interp = 1; the worst phase is bias_phase,
 * or H - 1 with a table.  For t < Z neither the convolution nor the row counts.  The row value is the start of the fp32
 * accumulator the convolution is added to.  WN_EARG before any device work, each naming its field: what the fp32 path refuses
 * (bias_hop < 0, bias_phase outside [0, bias_hop), bias_interp outside {0, 1} or without a hop, a table without a hop, with
 * bias_phase != 0 or misaligned, T + worst phase beyond 32 bits, bias_frame_stride < 128), rows that are not 16-byte aligned
 * and a stride that is no multiple of 4.
 * Backward: a descriptor with rows needs WN16_BWD_ROW_GRADS in flags, and dWf / dWg then hold 2 n_layers entries: entry
 * n_layers + l is layer l's filter / gate GRADIENT row of (clip 0, frame 0), in a block of the forward block's strides and
 * alignment.  Row j of clip b receives (+=, one addition per element) the fp32 sum over max(Z, first written row) <= t < T of
 * w_t v_t, v_t the STORED bf16 [da | dg] of position t: w = 1 over the t of frame j (over all t with one row per clip); with
 * bias_interp = 1, 1 - alpha_t over the t of frame j and alpha_t over those of frame j - 1.  One launch for all layers
 * (k16_row_grads; rows of more than 512 positions leave per-chunk sums in the workspace, added in chunk order by a second):
 * ascending t, no float atomics, bit-reproducible.  Every row of the block is written; one no live position reaches receives
 * + 0.  WN_EARG: the bit without rows, rows without the bit, any other bit. */
#define WN16_BWD_ROW_GRADS 1u
/* A11: xs (L,B,T,128) every layer's output, z (L,B,T,128), skip (B,T-t_off,Cs) or NULL */
int wn16_stack_fwd(const WnStackDesc* d, const uint16_t* pack, const uint16_t* x, uint16_t* xs, uint16_t* z,
                   uint16_t* skip, int B, int T, int t_off, int compat_zero_prefix, void* stream);
size_t wn16_stack_bwd_workspace_bytes(const WnStackDesc* d, int B, int T, int t_off);
/* A15: dout must be NULL (train_audio/train.py:72 discards the stack's residual output), dskip (B,T-t_off,Cs),
 * dx (B,T,128) or NULL; fp32 gradients accumulated.  flags: 0, or WN16_BWD_ROW_GRADS for a descriptor with gate-bias
 * rows (above: dWf / dWg then hold 2 n_layers entries). */
int wn16_stack_bwd(const WnStackDesc* d, const uint16_t* pack, const uint16_t* x, const uint16_t* xs, const uint16_t* z,
                   const uint16_t* dout, const uint16_t* dskip, uint16_t* dx, float* const* dWf, float* const* dWg,
                   float* const* dWp, float* const* dWs, void* ws, size_t ws_bytes, int B, int T, int t_off,
                   int compat_zero_prefix, unsigned flags, void* stream);
/* A12: Wb (Cout,Cin) and WbT (Cin,Cout) are the bf16 images of W; out is bf16 or fp32 (out_f32) */
int wn16_pack_pointwise(const float* W, uint16_t* Wb, uint16_t* WbT, int Cout, int Cin, void* stream);
int wn16_pointwise_fwd(const uint16_t* x, const uint16_t* Wb, const float* bias, void* out, int out_f32, int64_t N,
                       int Cin, int Cout, int act, void* stream);
/* ws (ABI 3; wn16_pointwise_bwd_workspace_bytes, may be NULL): with it the weight and bias gradients are sums of
 * per-workgroup partials added in a fixed order -- bit-reproducible; without it they accumulate through float atomics */
size_t wn16_pointwise_bwd_workspace_bytes(int64_t N, int Cout);
int wn16_pointwise_bwd(const uint16_t* x, const uint16_t* WbT, const uint16_t* dout, const float* dout_f32,
                       uint16_t* dout_scratch, uint16_t* dx, float* dW, float* dbias, int64_t N, int Cin, int Cout,
                       int act, void* ws, size_t ws_bytes, void* stream);

/* ---- step plan (ABI 5): the weight-only preparation of a training step in two launches -------------------------------
 * Between the optimiser step and the next one the weights do not change, but every entry point that holds a channel GEMM
 * prepares its operand images per call: zero a range word, measure max |W|, split -- three launch-floor kernels per GEMM --
 * and the stack packs its fp16 x 2 layer images, zeroes the multi-layer backward's dataflow words, measures max |dskip| ...:
 * ~16 of the 63 kernels of BASELINE config 2's step, ~0.1 ms of its 2.8.  A plan hoists them (wavenet.py:515-519 is the step):
 *   wn_plan_create(&plan, dev_mem, bytes)     caller-owned device memory (256-byte aligned; 16 MB covers config 2), no hipMalloc
 *   wn_plan_record(plan)                      then run ONE step whose WnExec carry .plan = plan: it runs as without a plan and
 *                                             every preparation that depends on weights only is registered (launcher arguments)
 *   wn_plan_finish(plan, stream)              lays the images out and uploads the job table (blocking; not under capture)
 *   wn_plan_prepare(plan, zero, n, stream)    FIRST call of every later step: all images, range words and plan-owned words in
 *                                             two launches; also zeroes `zero[0..n)` (the gradient arena: n % 4 == 0, 16-byte
 *                                             aligned; NULL / 0: nothing)
 * A READY plan makes an entry point skip its own preparation when the plan holds it (same weight pointers, same form) --
 * results are bit-identical to the per-call preparation -- so a call that carries one ASSERTS that wn_plan_prepare ran on the
 * same stream since the weights last changed.  Weight POINTERS are the keys: a plan belongs to one model.  Plan-owned words:
 * the dataflow words of the multi-layer backward, and the range word of the head's dx, filled by the GEMM that writes dx and
 * read by the dz contraction instead of a 100 MB pass over dskip.  A plan is a host object for ONE thread at a time;
 * wn_plan_record on a finished plan forgets its jobs and lays the images out anew at the next finish -- launches captured
 * into a graph against the old layout are void from then on (one plan per captured graph: wavenet_amd.TrainStepGraph).
 * wn_plan_stats: out[0..7] = state (0 idle, 1 recording,
 * 2 ready), weight images, layer images (layers), plan-owned words, device bytes used, prepare calls, look-ups served,
 * look-ups not served. */
int wn_plan_create(void** plan, void* dev_mem, size_t dev_bytes);
int wn_plan_destroy(void* plan);
int wn_plan_record(void* plan);
int wn_plan_finish(void* plan, void* stream);
int wn_plan_prepare(void* plan, float* zero, int64_t zero_floats, void* stream);
int wn_plan_stats(void* plan, int64_t* out8);

/* ---- measurement aid (bench.py): per-entry-point HIP-event timing on the caller's stream ------- */
int wn_prof_enable(int on);                    /* 1: clear + start recording, 0: stop               */
/* "name calls total_ms min_ms max_ms" per line into buf; returns the bytes needed (synchronises). */
int wn_prof_report(char* buf, int buflen);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WAVENET_HIP_H */
