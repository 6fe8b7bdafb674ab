// wn_corpus_gather: the training crops of one update, B crops of any files of a device-resident corpus, in ONE launch
// (include/wavenet_corpus.h is the contract; wavenet_amd/corpus.py the Python face; train_audio/train.py `_Crops` the rule).
//
// A crop's work is one flat index space: iw + tw + 1 window positions (position e feeds x[b, e] for e < iw + tw and
// tgt[b, e - iw - 1] for e > iw: both outputs are slices of the same window, so a token is read once), then F * n_cols feature
// cells.  A workgroup takes kChunk consecutive indices of one crop, lane on the fastest index: token reads, feature reads
// along a row and all writes are contiguous per wave.  The draw is read and fenced once per workgroup (uniform: scalar
// registers); the padded signal and the padded, clamped feature grid of `_Crops` are index arithmetic, never arrays.
// Tokens are uint8 or int32: two instantiations.  Byte loads, so a file may start at any offset.  No atomics, no LDS, no
// scratch; the work is a few hundred KB per update -- the point is one launch and a corpus at a quarter of the bytes.
//
// Built into libwavenet_corpus.so (include/wavenet_corpus.h), not into libwavenet_hip.so: it shares no code with that library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wavenet_corpus.h"

#define WN_SIDE_EARG WNC_EARG
#define WN_SIDE_EHIP WNC_EHIP
#include "side_host.hpp"

namespace wn {
namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;
constexpr int kChunk = kThreads * kPerThread;         // indices of one crop per workgroup

template <typename Tok>
__global__ __launch_bounds__(kThreads) void k_corpus_gather(const WnCorpusDesc d, const int32_t* __restrict__ draws,
                                                            int target_width, int n_cols, int chunks, int32_t* __restrict__ x,
                                                            int32_t* __restrict__ tgt, float* __restrict__ local,
                                                            int64_t* __restrict__ cond) {
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    // the draw, fenced: whatever the table holds, every read below stays inside file f's own tokens and columns
    int f = draws[2 * b], s = draws[2 * b + 1];
    f = min(max(f, 0), d.n_files - 1);
    const int len = d.file_len[f];
    s = min(max(s, 0), max(len - target_width - 2, 0));
    const int iw = d.input_width, W = iw + target_width;
    const int n_tok = W + 1;
    const int n_feat = d.features ? d.F * n_cols : 0;
    const Tok* __restrict__ tok = reinterpret_cast<const Tok*>(d.tokens) + d.file_offset[f];

    if (chunk == 0 && threadIdx.x == 0 && cond && d.file_class) cond[b] = d.file_class[f];

    int first = 0, last_col = 0;
    const float* __restrict__ feat = nullptr;
    if (n_feat) {
        first = (s + d.shift) / d.hop - d.pad_cols;          // column of the file under the crop's first position; < 0 in the pad
        last_col = max(d.col_count[f] - 1, 0);
        feat = d.features + d.col_offset[f];
    }
#pragma unroll
    for (int u = 0; u < kPerThread; ++u) {
        const int e = chunk * kChunk + u * kThreads + (int)threadIdx.x;
        if (e < n_tok) {
            const long long k = (long long)s + e - iw;        // index into the file; < 0: the silence in front
            const int v = (k >= 0 && k < len) ? (int)tok[k] : d.silence;
            if (e < W) x[(size_t)b * W + e] = v;
            if (e > iw) tgt[(size_t)b * target_width + (e - iw - 1)] = v;
        } else if (e < n_tok + n_feat) {
            const int q = e - n_tok;
            const int i = q / n_cols, c = q - i * n_cols;
            const int col = min(max(first + c, 0), last_col);
            local[((size_t)b * d.F + i) * n_cols + c] = feat[(size_t)i * d.total_cols + col];
        }
    }
}

}  // namespace
}  // namespace wn

using namespace wn;

int wn_corpus_abi_version(void) { return WN_CORPUS_ABI_VERSION; }
const char* wn_corpus_last_error(void) { return g_err; }

int wn_corpus_gather(const WnCorpusDesc* desc, const int32_t* draws, int B, int target_width, int n_cols, int32_t* x, int32_t* tgt,
                     float* local, int64_t* cond, void* stream) {
    WN_CHECK_ARG(desc && draws && x && tgt, "wn_corpus_gather: NULL desc, draws, x or tgt");
    const WnCorpusDesc& d = *desc;
    WN_CHECK_ARG(d.tokens && d.file_offset && d.file_len, "wn_corpus_gather: NULL tokens, file_offset or file_len in the descriptor");
    WN_CHECK_ARG(d.token_bytes == 1 || d.token_bytes == 4, "wn_corpus_gather: token_bytes = %d, it is 1 (uint8) or 4 (int32)",
                 d.token_bytes);
    WN_CHECK_ARG(d.n_files >= 1, "wn_corpus_gather: n_files = %d < 1", d.n_files);
    WN_CHECK_ARG(B >= 1, "wn_corpus_gather: B = %d < 1", B);
    WN_CHECK_ARG(target_width >= 1, "wn_corpus_gather: target_width = %d < 1", target_width);
    WN_CHECK_ARG(d.input_width >= 0, "wn_corpus_gather: input_width = %d < 0", d.input_width);
    WN_CHECK_ARG(d.silence >= 0 && (d.token_bytes == 4 || d.silence < 256),
                 "wn_corpus_gather: silence = %d is no token of %d byte(s)", d.silence, d.token_bytes);
    const long long W = (long long)d.input_width + target_width;
    long long n_feat = 0;
    if (d.features) {
        WN_CHECK_ARG(d.col_offset && d.col_count && local, "wn_corpus_gather: a corpus with features and NULL col_offset, col_count or local");
        WN_CHECK_ARG(d.F >= 1, "wn_corpus_gather: F = %d < 1", d.F);
        WN_CHECK_ARG(d.hop >= 1, "wn_corpus_gather: hop = %d < 1", d.hop);
        WN_CHECK_ARG(n_cols >= 1, "wn_corpus_gather: n_cols = %d < 1 with features", n_cols);
        WN_CHECK_ARG(d.total_cols >= 1, "wn_corpus_gather: total_cols = %lld < 1", (long long)d.total_cols);
        const long long pad = ((long long)d.input_width + d.hop - 1) / d.hop;
        WN_CHECK_ARG(d.pad_cols == pad && d.shift == pad * d.hop - d.input_width,
                     "wn_corpus_gather: pad_cols = %d, shift = %d; input_width = %d at hop = %d makes %lld and %lld", d.pad_cols,
                     d.shift, d.input_width, d.hop, pad, pad * d.hop - d.input_width);
        n_feat = (long long)d.F * n_cols;
    }
    WN_CHECK_ARG((long long)B * W < (1ll << 31) && (long long)B * n_feat < (1ll << 31),
                 "wn_corpus_gather: B = %d crops of %lld tokens and %lld feature cells: an output of 2^31 elements or more", B, W, n_feat);
    const long long chunks = (W + 1 + n_feat + kChunk - 1) / kChunk;
    WN_CHECK_ARG((long long)B * chunks < (1ll << 31), "wn_corpus_gather: %lld workgroups in one launch", (long long)B * chunks);
    const dim3 grid((unsigned)((long long)B * chunks)), block(kThreads);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (d.token_bytes == 1)
        hipLaunchKernelGGL(k_corpus_gather<uint8_t>, grid, block, 0, st, d, draws, target_width, n_cols, (int)chunks, x, tgt, local, cond);
    else
        hipLaunchKernelGGL(k_corpus_gather<int32_t>, grid, block, 0, st, d, draws, target_width, n_cols, (int)chunks, x, tgt, local, cond);
    return launch_status("wn_corpus_gather");
}
