// wn_logmel: a log-mel spectrogram of up to WN_LOGMEL_MAX_CLIPS clips in ONE launch (wavenet_amd/features.py is the definition).
//
// One workgroup (4 waves) per tile of 32 frames of one clip.  The tile's samples -- (31 hop + win) of them, contiguous --
// are read once into LDS, reflected at an end the caller flagged as the signal's and decoded from mu-law tokens on the way
// when a table is given.  The frame matrix is never formed: frame m, tap k is seg[m hop + k], read as the A operand of
// v_mfma_f32_32x32x2_f32 straight out of that segment (B = the caller's windowed cos / -sin basis, from L2).  Bins go in
// groups of 128: wave w forms Re and Im of bins [128 g + 32 w, +32) over K = win, takes the magnitude in registers and writes
// it to a (32 frames, 128 bins) LDS image; after a barrier wave w contracts that image with mel filters [32 w, +32) and
// [32 (w + 4), +32) on the same MFMA, accumulating over the groups.  The spectrum never reaches HBM.
//
// Determinism: exact-fp32 MFMA is a k-ordered fmaf chain, so a cell's bits are fixed by its own win samples, the basis and
// the filterbank: the sums run over k = 0 .. win - 1 and over bins 0 .. win / 2 in that order whatever tile, batch or call
// the column is part of.  No atomics, no scales.
//
// Built into libwavenet_logmel.so (include/wavenet_logmel.h), not into libwavenet_hip.so: it shares no code with that library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wavenet_logmel.h"

#define WN_SIDE_EARG WNL_EARG
#define WN_SIDE_EHIP WNL_EHIP
#include "side_host.hpp"

namespace wn {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 32;                 // frames per workgroup
constexpr int kGroup = 128;               // bins per pass: 32 per wave
constexpr int kMagLd = kGroup + 1;        // odd row stride: the 32 frames of a column sit in 32 different banks
constexpr int kLdsLimit = 160 * 1024;     // gfx950

struct LogmelArgs {
    WnLogmelClip clip[WN_LOGMEL_MAX_CLIPS];
    int n_clips;
};

// Samples of a row start every hop floats: with an even hop the 32 frames' tap k would share a bank.  One pad float per hop
// samples makes the row stride hop + 1 (odd) -- seg_index(s) = s + (s / hop) * pad.
__host__ __device__ inline int seg_pad(int hop) { return (hop & 1) ? 0 : 1; }
__host__ __device__ inline long long seg_floats(int hop, int win) {
    const long long n = 31ll * hop + win;
    return n + (seg_pad(hop) ? n / hop + 1 : 0);
}

__global__ __launch_bounds__(256) void k_logmel(const LogmelArgs a, const float* __restrict__ table, int Q,
                                                const float* __restrict__ basis, const float* __restrict__ fbT, int win,
                                                int hop, int n_mels) {
    extern __shared__ float lds[];
    const int nb = win / 2 + 1, ld = 2 * nb;
    const int pad = seg_pad(hop);
    const int seg_len = 31 * hop + win;
    float* seg = lds;
    float* mag = lds + seg_floats(hop, win);

    // which clip, which tile of it (at most 64 clips: a scalar scan)
    int c = 0, tile = blockIdx.x;
    for (; c < a.n_clips; ++c) {
        const int t = (a.clip[c].count + kTile - 1) / kTile;
        if (tile < t) break;
        tile -= t;
    }
    if (c >= a.n_clips) return;
    const WnLogmelClip cl = a.clip[c];
    const int f0 = tile * kTile;                                   // first frame of the tile, relative to cl.first
    const int nf = min(kTile, cl.count - f0);
    const long long j0 = cl.origin + ((long long)cl.first + f0) * hop - win / 2;   // buffer index of seg[0]
    const int need = (nf - 1) * hop + win;                          // what the nf frames read

    const float* xf = reinterpret_cast<const float*>(cl.x);
    const int32_t* xt = reinterpret_cast<const int32_t*>(cl.x);
    for (int i = threadIdx.x; i < seg_len; i += blockDim.x) {
        long long j = j0 + i;
        if (j < 0 && (cl.flags & WN_LOGMEL_REFLECT_LEFT)) j = -j;
        else if (j >= cl.n && (cl.flags & WN_LOGMEL_REFLECT_RIGHT)) j = 2 * (cl.n - 1) - j;
        float v = 0.f;
        if (i < need && j >= 0 && j < cl.n) {
            if (table) {
                int q = xt[j];
                q = q < 0 ? 0 : (q >= Q ? Q - 1 : q);
                v = table[q];
            } else {
                v = xf[j];
            }
        }
        seg[i + (pad ? i / hop : 0)] = v;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = lane & 31, h = lane >> 5;
    const int row = m * (hop + pad);                               // seg index of frame m, tap 0
    const int mel_tiles = (n_mels + 31) / 32;
    f32x16 mel0 = {0}, mel1 = {0};

    for (int g0 = 0; g0 < nb; g0 += kGroup) {
        // ---- Re, Im of 32 bins over K = win, magnitude to LDS ---------------------------------------------------------------
        const int bin = g0 + w * 32 + m;
        f32x16 re = {0}, im = {0};
        if (g0 + w * 32 < nb) {                                    // wave-uniform
            const float* bre = basis + min(bin, nb - 1);
            const float* bim = bre + nb;
            int kq = 0, kr = h;                                    // tap k = k0 + h = kq * hop + kr (even hop only; unused otherwise)
            const auto next_tap = [&] {
                if (pad) {
                    kr += 2;
                    if (kr >= hop) { kr -= hop; ++kq; }
                }
            };
            int k0 = 0;
            for (; k0 + 16 <= win; k0 += 16) {                     // eight steps' operands requested ahead of their MFMAs
                float av[8], br[8], bi[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int k = k0 + 2 * u + h;
                    av[u] = seg[row + k + kq];
                    br[u] = bre[(size_t)k * ld];
                    bi[u] = bim[(size_t)k * ld];
                    next_tap();
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    re = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], br[u], re, 0, 0, 0);
                    im = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bi[u], im, 0, 0, 0);
                }
            }
            for (; k0 < win; k0 += 2) {                            // any even win
                const int k = k0 + h;
                const float av = seg[row + k + kq];
                re = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bre[(size_t)k * ld], re, 0, 0, 0);
                im = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bim[(size_t)k * ld], im, 0, 0, 0);
                next_tap();
            }
        }
        for (int r = 0; r < 16; ++r) {
            const int frame = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float v = bin < nb ? sqrtf(re[r] * re[r] + im[r] * im[r]) : 0.f;
            mag[frame * kMagLd + w * 32 + m] = v;
        }
        __syncthreads();
        // ---- mel[filter][frame] += fb[filter][bin] * mag[frame][bin], bins in order ------------------------------------------
        const int kb = min(kGroup, nb - g0);
        if (w < mel_tiles) {
            const float* f0p = fbT + min(w * 32 + m, n_mels - 1);
            const float* f1p = fbT + min((w + 4) * 32 + m, n_mels - 1);
            const bool two = w + 4 < mel_tiles;
            for (int k0 = 0; k0 < kb; k0 += 2) {
                const int k = k0 + h;                              // k <= 127; a bin past the last one has magnitude 0
                const size_t brow = (size_t)min(g0 + k, nb - 1) * n_mels;
                const float mv = mag[m * kMagLd + k];
                mel0 = __builtin_amdgcn_mfma_f32_32x32x2f32(f0p[brow], mv, mel0, 0, 0, 0);
                if (two) mel1 = __builtin_amdgcn_mfma_f32_32x32x2f32(f1p[brow], mv, mel1, 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // ---- floor, log, store: filter on the registers, frame on the lane ---------------------------------------------------------
    if (m < nf) {
        for (int r = 0; r < 16; ++r) {
            const int f = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int fa = w * 32 + f, fb2 = (w + 4) * 32 + f;
            if (fa < n_mels) cl.out[(size_t)fa * cl.out_stride + f0 + m] = logf(fmaxf(mel0[r], 1e-5f));
            if (fb2 < n_mels) cl.out[(size_t)fb2 * cl.out_stride + f0 + m] = logf(fmaxf(mel1[r], 1e-5f));
        }
    }
}

}  // namespace
}  // namespace wn

using namespace wn;

int wn_logmel_abi_version(void) { return WN_LOGMEL_ABI_VERSION; }
const char* wn_logmel_last_error(void) { return g_err; }

int wn_logmel(const WnLogmelClip* clips, int n_clips, const float* table, int Q, const float* basis, const float* fbT,
              int win, int hop, int n_mels, void* stream) {
    WN_CHECK_ARG(clips && basis && fbT, "wn_logmel: NULL clips, basis or filterbank");
    WN_CHECK_ARG(n_clips >= 1 && n_clips <= WN_LOGMEL_MAX_CLIPS, "wn_logmel: n_clips = %d outside 1 .. %d", n_clips,
                 WN_LOGMEL_MAX_CLIPS);
    WN_CHECK_ARG(win >= 16 && win <= 4096 && win % 2 == 0, "wn_logmel: win = %d is not an even number in 16 .. 4096", win);
    WN_CHECK_ARG(hop >= 1, "wn_logmel: hop = %d < 1", hop);
    WN_CHECK_ARG(n_mels >= 1 && n_mels <= 256, "wn_logmel: n_mels = %d outside 1 .. 256", n_mels);
    WN_CHECK_ARG(!table || Q >= 1, "wn_logmel: a decode table of Q = %d entries", Q);
    const long long lds_bytes = (seg_floats(hop, win) + (long long)kTile * kMagLd) * 4;
    WN_CHECK_ARG(lds_bytes <= kLdsLimit,
                 "wn_logmel: a tile's segment of 31 * hop + win = %lld samples needs %lld bytes of LDS, the limit is %d (hop = %d, "
                 "win = %d)", 31ll * hop + win, lds_bytes, kLdsLimit, hop, win);
    LogmelArgs args;
    long long tiles = 0;
    for (int c = 0; c < n_clips; ++c) {
        const WnLogmelClip& cl = clips[c];
        WN_CHECK_ARG(cl.x && cl.out, "wn_logmel: clip %d has a NULL buffer or output", c);
        WN_CHECK_ARG(cl.n > win / 2, "wn_logmel: clip %d has %lld samples, it needs more than win / 2 = %d", c, (long long)cl.n,
                     win / 2);
        WN_CHECK_ARG(cl.n < (1ll << 40) && cl.origin > -(1ll << 40) && cl.origin < (1ll << 40),
                     "wn_logmel: clip %d: n = %lld or origin = %lld out of range", c, (long long)cl.n, (long long)cl.origin);
        WN_CHECK_ARG(cl.first >= 0 && cl.count >= 1, "wn_logmel: clip %d: first = %d < 0 or count = %d < 1", c, cl.first, cl.count);
        WN_CHECK_ARG(cl.out_stride >= cl.count, "wn_logmel: clip %d: out_stride = %lld below its %d frames", c,
                     (long long)cl.out_stride, cl.count);
        WN_CHECK_ARG((cl.flags & ~(WN_LOGMEL_REFLECT_LEFT | WN_LOGMEL_REFLECT_RIGHT)) == 0, "wn_logmel: clip %d: flags = %u", c,
                     cl.flags);
        const long long lo = cl.origin + (long long)cl.first * hop - win / 2;                          // first sample read
        const long long hi = cl.origin + ((long long)cl.first + cl.count - 1) * hop + win / 2 - 1;     // last sample read
        if (lo < 0)
            WN_CHECK_ARG((cl.flags & WN_LOGMEL_REFLECT_LEFT) && -lo <= cl.n - 1,
                         "wn_logmel: clip %d: frame %d reads sample %lld, before the buffer%s", c, cl.first, lo,
                         (cl.flags & WN_LOGMEL_REFLECT_LEFT) ? " and past what a reflection reaches" : ", and its left end is not flagged as the signal's");
        if (hi >= cl.n)
            WN_CHECK_ARG((cl.flags & WN_LOGMEL_REFLECT_RIGHT) && 2 * (cl.n - 1) - hi >= 0,
                         "wn_logmel: clip %d: frame %d reads sample %lld of %lld%s", c, cl.first + cl.count - 1, hi, (long long)cl.n,
                         (cl.flags & WN_LOGMEL_REFLECT_RIGHT) ? ", past what a reflection reaches" : ", and its right end is not flagged as the signal's");
        WN_CHECK_ARG(lo < cl.n && hi >= 0, "wn_logmel: clip %d: frames %d .. %d lie outside the buffer", c, cl.first,
                     cl.first + cl.count - 1);
        args.clip[c] = cl;
        tiles += (cl.count + kTile - 1) / kTile;
    }
    WN_CHECK_ARG(tiles < (1ll << 31), "wn_logmel: %lld frame tiles in one launch", tiles);
    args.n_clips = n_clips;
    if (const int rc = raise_lds_limit(k_logmel, "k_logmel", lds_bytes)) return rc;
    hipLaunchKernelGGL(k_logmel, dim3((unsigned)tiles), dim3(256), (size_t)lds_bytes, reinterpret_cast<hipStream_t>(stream), args,
                       table, Q, basis, fbT, win, hop, n_mels);
    return launch_status("wn_logmel");
}
