// wn_resample: sample-rate conversion of up to WN_RESAMPLE_MAX_CLIPS clips in ONE launch (wavenet_amd/resample.py is the definition).
//
// One workgroup (4 waves) per tile of WN_RESAMPLE_TILE consecutive outputs of one clip, one output per lane.  With
// q, phi = divmod(n M, L) output n reads inputs q - Kt .. q + Kt, so the tile's outputs read one contiguous span of at most
// (TILE - 1) M / L + T + 1 inputs: it is brought into LDS once, converted to float32 (int16 PCM is v / 32768, exact), with zeros
// where it leaves the buffer -- the caller flagged that end as the signal's, or the call was refused on the host; the bounds
// check is the fence either way.  n M is formed in 64 bits once per workgroup (the tile's first output); a lane adds at most
// 255 M to its remainder, which fits 32 bits.  Neighbouring lanes read LDS words M / L apart: conflict-free for an odd step
// (48 -> 16 kHz: 3), a broadcast when the rate goes up.  The tap table stays in global memory: row phi of T floats, read in t
// order, so a lane walks one cache line per 32 taps; for L == 1 every lane reads the same row and the loads are scalar.
//
// Determinism: acc = fmaf(taps[phi][t], x[q + Kt - t], acc) for t = 0 .. T - 1 from acc = 0, whatever tile, batch or call the
// output is part of and wherever the buffer starts.  No atomics, no reduction across lanes, no MFMA.
//
// Built into libwavenet_resample.so (include/wavenet_resample.h): it shares no code with the other libraries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/wavenet_resample.h"

#define WN_SIDE_EARG WNR_EARG
#define WN_SIDE_EHIP WNR_EHIP
#include "../side_host.hpp"

namespace wn {
namespace {

constexpr int kTile = WN_RESAMPLE_TILE;   // outputs per workgroup, one per lane
constexpr int kLdsLimit = 160 * 1024;     // gfx950

struct ResampleArgs {
    WnResampleClip clip[WN_RESAMPLE_MAX_CLIPS];
    int n_clips;
};

// the most inputs a tile reads: its last lane sits (L - 1 + (kTile - 1) M) / L inputs behind its first at the most
__host__ __device__ inline long long span_floats(int L, int M, int T) { return (L - 1 + (long long)(kTile - 1) * M) / L + T; }

__global__ __launch_bounds__(kTile) void k_resample(const ResampleArgs a, int in_kind, int out_kind,
                                                    const float* __restrict__ taps, int L, int M, int T,
                                                    const int32_t* __restrict__ lut) {
    extern __shared__ float seg[];

    // which clip, which tile of it (at most 64 clips: a scalar scan)
    int c = 0;
    long long tile = blockIdx.x;
    for (; c < a.n_clips; ++c) {
        const long long t = (a.clip[c].count + kTile - 1) / kTile;
        if (tile < t) break;
        tile -= t;
    }
    if (c >= a.n_clips) return;
    const WnResampleClip cl = a.clip[c];
    const long long o0 = tile * kTile;                              // first output of the tile, relative to cl.first
    const int nf = (int)min((long long)kTile, cl.count - o0);
    const long long prod = (cl.first + o0) * (long long)M;          // 64 bits: an hour at 44.1 -> 16 kHz reaches 2.5e10
    const long long q0 = prod / L;
    const int r0 = (int)(prod - q0 * L);
    const int Kt = (T - 1) / 2;
    const int used = (r0 + (nf - 1) * M) / L + T;                   // inputs q0 - Kt .. that the nf outputs read
    const long long b0 = q0 - Kt - cl.origin;                       // buffer index of seg[0]

    const int16_t* xs = reinterpret_cast<const int16_t*>(cl.x);
    const float* xf = reinterpret_cast<const float*>(cl.x);
    for (int i = threadIdx.x; i < used; i += kTile) {
        const long long b = b0 + i;
        float v = 0.f;
        if (b >= 0 && b < cl.n) v = in_kind == WN_RESAMPLE_IN_PCM16 ? (float)xs[b] * (1.f / 32768.f) : xf[b];
        seg[i] = v;
    }
    __syncthreads();

    const int i = threadIdx.x;
    if (i >= nf) return;
    const int v = r0 + i * M;
    const int dq = v / L, phi = v - dq * L;
    const float* x = seg + dq + (T - 1);                            // x[-t] is input q + Kt - t
    float acc = 0.f;
    if (L == 1) {                                                   // one row for every lane: uniform addresses
#pragma unroll 8
        for (int t = 0; t < T; ++t) acc = fmaf(taps[t], x[-t], acc);
    } else {
        const float* row = taps + (size_t)phi * T;
#pragma unroll 8
        for (int t = 0; t < T; ++t) acc = fmaf(row[t], x[-t], acc);
    }
    const long long o = o0 + i;
    if (out_kind == WN_RESAMPLE_OUT_F32) {
        reinterpret_cast<float*>(cl.out)[o] = acc;
    } else {
        const int pcm = (int)fminf(fmaxf(rintf(acc * 32768.f), -32768.f), 32767.f);
        if (out_kind == WN_RESAMPLE_OUT_PCM16) reinterpret_cast<int16_t*>(cl.out)[o] = (int16_t)pcm;
        else reinterpret_cast<int32_t*>(cl.out)[o] = lut[pcm + 32768];
    }
}

}  // namespace
}  // namespace wn

using namespace wn;

int wn_resample_abi_version(void) { return WN_RESAMPLE_ABI_VERSION; }
const char* wn_resample_last_error(void) { return g_err; }

int wn_resample(const WnResampleClip* clips, int n_clips, int in_kind, int out_kind, const float* taps, int L, int M, int T,
                const int32_t* lut, void* stream) {
    WN_CHECK_ARG(clips && taps, "wn_resample: NULL clips or taps");
    WN_CHECK_ARG(n_clips >= 1 && n_clips <= WN_RESAMPLE_MAX_CLIPS, "wn_resample: n_clips = %d outside 1 .. %d", n_clips,
                 WN_RESAMPLE_MAX_CLIPS);
    WN_CHECK_ARG(L >= 1 && L <= 1024, "wn_resample: L = %d outside 1 .. 1024", L);
    WN_CHECK_ARG(M >= 1 && M <= 1024, "wn_resample: M = %d outside 1 .. 1024", M);
    WN_CHECK_ARG(L != M, "wn_resample: L == M = %d: equal rates are the identity, there is nothing to launch", L);
    WN_CHECK_ARG(T >= 3 && T <= 2047 && T % 2 == 1, "wn_resample: T = %d is not an odd number in 3 .. 2047", T);
    WN_CHECK_ARG(in_kind == WN_RESAMPLE_IN_PCM16 || in_kind == WN_RESAMPLE_IN_F32, "wn_resample: in_kind = %d", in_kind);
    WN_CHECK_ARG(out_kind == WN_RESAMPLE_OUT_F32 || out_kind == WN_RESAMPLE_OUT_PCM16 || out_kind == WN_RESAMPLE_OUT_TOKENS,
                 "wn_resample: out_kind = %d", out_kind);
    WN_CHECK_ARG(out_kind != WN_RESAMPLE_OUT_TOKENS || lut, "wn_resample: out_kind = %d (tokens) needs lut, got NULL", out_kind);
    const long long lds_bytes = span_floats(L, M, T) * 4;
    WN_CHECK_ARG(lds_bytes <= kLdsLimit,
                 "wn_resample: a tile's span of %lld samples needs %lld bytes of LDS, the limit is %d (L = %d, M = %d, T = %d)",
                 span_floats(L, M, T), lds_bytes, kLdsLimit, L, M, T);
    const int Kt = (T - 1) / 2;
    ResampleArgs args;
    long long tiles = 0;
    for (int c = 0; c < n_clips; ++c) {
        const WnResampleClip& cl = clips[c];
        WN_CHECK_ARG(cl.count >= 0, "wn_resample: clip %d: count = %lld < 0", c, (long long)cl.count);
        WN_CHECK_ARG(cl.first >= 0, "wn_resample: clip %d: first = %lld < 0", c, (long long)cl.first);
        WN_CHECK_ARG(cl.n >= 0 && cl.n < (1ll << 40) && cl.origin >= 0 && cl.origin < (1ll << 40) && cl.first < (1ll << 40) &&
                         cl.count < (1ll << 40),
                     "wn_resample: clip %d: n = %lld, origin = %lld, first = %lld or count = %lld out of range", c, (long long)cl.n,
                     (long long)cl.origin, (long long)cl.first, (long long)cl.count);
        WN_CHECK_ARG((cl.flags & ~(WN_RESAMPLE_START | WN_RESAMPLE_END)) == 0, "wn_resample: clip %d: flags = %u", c, cl.flags);
        WN_CHECK_ARG(!(cl.flags & WN_RESAMPLE_START) || cl.origin == 0,
                     "wn_resample: clip %d: origin = %lld under WN_RESAMPLE_START, where x[0] is input 0", c, (long long)cl.origin);
        if (cl.count > 0) {
            WN_CHECK_ARG(cl.x && cl.out, "wn_resample: clip %d has a NULL buffer or output", c);
            const long long lo = cl.first * (long long)M / L - Kt;                        // first input read
            const long long hi = (cl.first + cl.count - 1) * (long long)M / L + Kt;       // last input read
            WN_CHECK_ARG(lo >= cl.origin || (cl.flags & WN_RESAMPLE_START),
                         "wn_resample: clip %d: output %lld reads input %lld, before the buffer (origin %lld), and its start is not "
                         "flagged as the signal's", c, (long long)cl.first, lo, (long long)cl.origin);
            WN_CHECK_ARG(hi < cl.origin + cl.n || (cl.flags & WN_RESAMPLE_END),
                         "wn_resample: clip %d: output %lld reads input %lld, the buffer ends with %lld, and its end is not flagged "
                         "as the signal's", c, (long long)(cl.first + cl.count - 1), hi, (long long)(cl.origin + cl.n - 1));
        }
        args.clip[c] = cl;
        tiles += (cl.count + kTile - 1) / kTile;
    }
    WN_CHECK_ARG(tiles < (1ll << 31), "wn_resample: %lld output tiles in one launch", tiles);
    if (tiles == 0) return WNR_OK;
    args.n_clips = n_clips;
    if (const int rc = raise_lds_limit(k_resample, "k_resample", lds_bytes)) return rc;
    hipLaunchKernelGGL(k_resample, dim3((unsigned)tiles), dim3(kTile), (size_t)lds_bytes, reinterpret_cast<hipStream_t>(stream),
                       args, in_kind, out_kind, taps, L, M, T, lut);
    return launch_status("wn_resample");
}
