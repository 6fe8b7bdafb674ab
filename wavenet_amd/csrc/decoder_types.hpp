// Tables shared by the generic (decoder.hip) and the specialised (decoder_fast.hip) decode kernels.
#pragma once
#include "sample_filter.hpp"
namespace wn {
struct DecCausal { int w, b, ring, cin, cout; };            // float offsets into the arena; b < 0: none
struct DecLayer { int wfg, bfg, wps, bps, ring, d, cd; };
struct DecHead { int w, b, cin, cout; };
struct DecMeta {
    int Q, fwc, ncausal, fw, nlayers, Cr, Cs, nhead, head_act;
    int maxc;          // widest vector that has to sit in LDS
};
// Local conditioning: the frame table of one utterance as a step loop takes it.  tab == NULL: no table, and the loop
// executes what it executed before tables existed.  Step `it` of the launch adds row (pos0 + it) / hop -- pos0 = the table's
// phase (FrameTable) + the steps run since the table was set (Decoder::since_set) -- to every layer's gate pre-activations.
// interp != 0 (WnDecoderDesc.frame_interp, linear interpolation): with p = pos0 + it, j = p / hop and alpha = float(p % hop) /
// float(hop) the step adds r[j] + alpha (r[j + 1] - r[j]) (bias_lerp, as the layer kernels form it).
// prob_stride of the step loops (both files): the floats between two rows of the probability trace, Q -- or kProbChosen: the
// trace is ONE float per step, the probability of the token drawn (WN_DECODER_TRACE_CHOSEN).  One or the other per launch.
static constexpr int kProbChosen = 0;
// do_sample of the launchers (both files): 0 = no draw (wn_decoder_step), kSampleDraw = every step draws, kSampleGiven
// (WN_DECODER_FORCED_TOKENS handles) = step `it` reads f = out_tokens[it] first and emits f when (unsigned)f < (unsigned)Q -- no
// filter, no draw, uniforms[it] unused -- and draws as kSampleDraw does otherwise.  One value per launch.  The launchers turn
// kSampleGiven into the FORCED instantiations of the kernels; a kernel only asks whether its do_sample is 0.
static constexpr int kSampleDraw = 1, kSampleGiven = 2;
// ring != 0 (WN_DECODER_FRAME_RING handles): tab is the caller's ring of `ring` rows, `row` floats apart, read in place -- frame j
// lives in row j mod ring, and row j + 1 of the ring's last row is row 0.  ring == 0: the flat table, addressed as ever.
struct DecFrames { const float* tab; int hop; int row; long long pos0; int interp; int ring; };
// One utterance's launch arguments of the specialised decode kernels (decoder_fast.hip): filled from its handle by
// decoder.hip, passed to the kernels by value (the batched launch passes an array of them)
struct DecUtt {
    const float* P; const float* hbias; const float* E; const DecLayer* layers; float* arena; int* tok_ring;
    long long n0; const double* uniforms; int32_t* out_tokens; float* prob_out;
    unsigned long long* X;             // exchange entries of the nine-workgroup form: set by the launch, from P
    int first_token;
    int nsteps;                        // batched launch: the utterance's own step count, the ONE word all nine of its workgroups
                                       // read (single runs pass theirs as a kernel argument and leave this 0)
    SampleCtl sc;                      // per utterance: its handle's wn_decoder_set_sampling
    DecFrames fr;                      // WN_DECODER_GATE_ROWS handles: the utterance's own frame table (tab == NULL: none)
};
// One utterance as the any-shape kernels take it, from its own handle (any_utt): k_decode's arguments, and an entry of the
// table k_decode_batch and k_decode_tile (decoder_tile.hip) read from device memory (Decoder::batch_tab of handle 0).
struct DecAnyUtt {
    const DecCausal* causal; const DecLayer* layers; const DecHead* heads;
    float* arena; int* tok_ring; long long n0; const double* uniforms; int32_t* out_tokens; float* prob_out;
    int first_token; int nsteps;       // nsteps: the utterance's own step count (batched: min(n, steps left under its step_limit))
    SampleCtl sc;
    DecFrames fr;
};
size_t decode_fast_pack_floats(int nlayers);
int decode_fast_pack(const WnDecoderDesc* d, float* dst, hipStream_t s);
// gate_rows (both launches): a WN_DECODER_GATE_ROWS handle that holds static gate biases (its own arena, DecLayer.bfg) or a frame
// table (DecUtt.fr) -- the launch takes the instantiations whose wave 1 seeds every gate row with them; without it the launch
// is the one it was before the flag existed
int decode_fast_launch(DecUtt q, int nlayers, int nsteps, int prob_stride, int apply_softmax, int do_sample, int head_act,
                       bool three_wgs, bool gate_rows, hipStream_t s);
static constexpr int kDecMaxBatch = 28;                    // utterances per batched launch: 28 x 9 workgroups on 256 CUs
int decode_fast_batch_ok(int nlayers, int n_utt, int nsteps);
// (nsteps: the launch's n, an upper bound of the utterances' counts, for the checks only: the kernel reads DecUtt.nsteps;
// do_sample: kSampleDraw or kSampleGiven, the launch's)
int decode_fast_launch_batch(int n_utt, const DecUtt* utt, int nlayers, int nsteps, int prob_stride, int do_sample, int head_act,
                             bool same_weights, bool gate_rows, hipStream_t s);
int decode_fast_status(const float* P, int nlayers, hipStream_t s, int* gave_up);
// decoder_tile.hip: one launch of k_decode_tile<U, LERP, FORCED, RING> over the n_utt entries of `tab` (device memory), ceil(n_utt / U)
// workgroups with `lds` bytes of dynamic LDS each; U in {2, 4, 8, 16} (checked by the caller)
int decode_tile_launch(int U, bool lerp, bool forced, bool ring, const DecMeta& M, const DecAnyUtt* tab, int n_utt, int prob_stride,
                       size_t lds, hipStream_t s);
}  // namespace wn
