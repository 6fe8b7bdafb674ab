// wn_pitch: YIN pitch tracking of up to WN_PITCH_MAX_CLIPS clips in ONE launch (wavenet_amd/pitch.py is the definition).
//
// One workgroup per tile of `ft` consecutive frames of one clip (ft = 1 .. 8, as many as fill 256 lanes with groups of kLags
// lags).  The tile's samples -- (ft - 1) hop + S of them, S = win + tau_max, contiguous -- are read once into LDS, zero beyond
// an edge that the caller flagged as the signal's and decoded from mu-law tokens on the way when a table is given.
//   1. A lane owns kLags consecutive lags of one frame and walks j = 0 .. win - 1: s[j] is a broadcast read, the lag window
//      slides through registers (one new LDS word per j), acc = fmaf(diff, diff, acc).  d goes to LDS.
//   2. One lane per frame forms the running sums r_tau = d[1] + ... + d[tau] in index order.
//   3. All lanes form c[tau] = d[tau] * tau / r_tau in place (and write the curve where it is asked for).
//   4. One wave per frame: the first lag below the threshold and the first argmin are integer reductions over the wave; lane 0
//      walks to the local minimum, refines and stores the two values.
// This is plain fp32 VALU work; there is nothing for the MFMA here.
//
// Determinism: every d[tau] is one j-ordered fmaf chain, every r_tau one tau-ordered chain of additions, and everything
// behind them is a function of those values, so a column's bits are fixed by its own S samples and the scalar arguments
// whatever tile, batch, range or call it is part of.  No atomics.
//
// Built into libwavenet_pitch.so (include/wavenet_pitch.h), not into libwavenet_hip.so: it shares no code with that library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/wavenet_pitch.h"

#define WN_SIDE_EARG WNP_EARG
#define WN_SIDE_EHIP WNP_EHIP
#include "../side_host.hpp"

namespace wn {
namespace {

// consecutive lags per lane.  Odd: neighbouring lanes read their windows kLags LDS words apart, and ds_read_b32 banks by the word
// address mod 32 over 32 lanes, so an odd step is conflict-free where a step of 4 is 4-way
constexpr int kLags = 7;
constexpr int kMaxTile = 8;               // frames per workgroup, at most
constexpr int kSegPad = 8;                // zeros behind the segment: the sliding window reads up to kLags words past it
constexpr int kThreads = 256;
constexpr int kLdsLimit = 160 * 1024;     // gfx950

// what the kernel needs of a WnPitchClip (64 of them and the scalars stay below the 4 KB of kernel arguments).  The flags stay
// on the host: it has refused every frame they do not allow, and the kernel reads any index outside the buffer as zero.
struct PitchClip {
    const void* x;
    long long n;
    long long base;                       // buffer index of the first sample of frame `first`
    float* out;
    long long out_stride;
    float* curve;
    int count;
};
struct PitchArgs {
    PitchClip clip[WN_PITCH_MAX_CLIPS];
    int n_clips;
};

inline int lag_groups(int tau_max) { return (tau_max + kLags) / kLags; }          // ceil((tau_max + 1) / kLags)
inline int tile_frames(int tau_max) {
    const int ft = kThreads / lag_groups(tau_max);
    return ft < 1 ? 1 : (ft > kMaxTile ? kMaxTile : ft);
}
inline long long lds_floats(int win, int hop, int tau_max, int ft) {
    return (long long)(ft - 1) * hop + win + tau_max + kSegPad + 2ll * ft * (tau_max + 1);
}

__global__ __launch_bounds__(kThreads) void k_pitch(const PitchArgs a, const float* __restrict__ table, int Q, int win, int hop,
                                                    int tau_min, int tau_max, float threshold, float rate, int ft) {
    extern __shared__ float lds[];
    const int S = win + tau_max, nl = tau_max + 1;
    const int seg_len = (ft - 1) * hop + S + kSegPad;
    float* seg = lds;
    float* dls = lds + seg_len;                                    // (ft, nl): d, then c in place
    float* rls = dls + ft * nl;                                    // (ft, nl): running sums

    // which clip, which tile of it (at most 64 clips: a scalar scan)
    int c = 0, tile = blockIdx.x;
    for (; c < a.n_clips; ++c) {
        const int t = (a.clip[c].count + ft - 1) / ft;
        if (tile < t) break;
        tile -= t;
    }
    if (c >= a.n_clips) return;
    const PitchClip cl = a.clip[c];
    const int f0 = tile * ft;                                      // first frame of the tile, relative to the clip's first
    const int nf = min(ft, cl.count - f0);
    const long long j0 = cl.base + (long long)f0 * hop;            // buffer index of seg[0]
    const int need = (nf - 1) * hop + S;                           // what the nf frames read

    const float* xf = reinterpret_cast<const float*>(cl.x);
    const int32_t* xt = reinterpret_cast<const int32_t*>(cl.x);
    for (int i = threadIdx.x; i < seg_len; i += blockDim.x) {
        const long long j = j0 + i;
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
        seg[i] = v;
    }
    __syncthreads();

    // ---- 1. d[f][tau]: a lane takes kLags lags of one frame ---------------------------------------------------------------------
    const int groups = (nl + kLags - 1) / kLags;
    for (int item = threadIdx.x; item < nf * groups; item += blockDim.x) {
        const int f = item / groups, tau0 = (item - f * groups) * kLags;
        const float* s = seg + f * hop;
        float acc[kLags], w[kLags];
#pragma unroll
        for (int i = 0; i < kLags; ++i) {
            acc[i] = 0.f;
            w[i] = s[tau0 + i];                                    // tau0 + kLags - 1 <= tau_max + kLags - 1 < S + kSegPad
        }
        const float* nxt = s + tau0 + kLags;                       // nxt[j] <= s[win - 1 + tau_max + kLags]: inside the pad
#pragma unroll 4
        for (int j = 0; j < win; ++j) {
            const float sj = s[j];
#pragma unroll
            for (int i = 0; i < kLags; ++i) {
                const float diff = sj - w[i];
                acc[i] = fmaf(diff, diff, acc[i]);
            }
#pragma unroll
            for (int i = 0; i + 1 < kLags; ++i) w[i] = w[i + 1];
            w[kLags - 1] = nxt[j];
        }
#pragma unroll
        for (int i = 0; i < kLags; ++i)
            if (tau0 + i < nl) dls[f * nl + tau0 + i] = acc[i];
    }
    __syncthreads();

    // ---- 2. running sums, one lane per frame, in index order ---------------------------------------------------------------------
    if (threadIdx.x < nf) {
        const float* d = dls + threadIdx.x * nl;
        float* r = rls + threadIdx.x * nl;
        float run = 0.f;
        r[0] = 0.f;
        for (int tau = 1; tau < nl; ++tau) {
            run += d[tau];
            r[tau] = run;
        }
    }
    __syncthreads();

    // ---- 3. c = d tau / r in place ----------------------------------------------------------------------------------------------------
    for (int i = threadIdx.x; i < nf * nl; i += blockDim.x) {
        const int f = i / nl, tau = i - f * nl;
        const float r = rls[i];
        const float v = (tau > 0 && r > 0.f) ? (dls[i] * (float)tau) / r : 1.f;
        dls[i] = v;
        if (cl.curve) cl.curve[(size_t)(f0 + f) * nl + tau] = v;
    }
    __syncthreads();

    // ---- 4. selection and refinement: one wave per frame ------------------------------------------------------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int f = wave; f < nf; f += waves) {
        const float* cv = dls + f * nl;
        int below = 0x7fffffff, arg = tau_min;
        float best = cv[tau_min];
        for (int tau = tau_min + lane; tau < tau_max; tau += 64) {  // tau_min .. tau_max - 1
            const float v = cv[tau];
            if (v < threshold && tau < below) below = tau;
            if (v < best) {                                        // ascending tau per lane: the first of equals stays
                best = v;
                arg = tau;
            }
        }
        for (int off = 32; off; off >>= 1) {
            const int ob = __shfl_xor(below, off);
            const float ov = __shfl_xor(best, off);
            const int oa = __shfl_xor(arg, off);
            below = min(below, ob);
            if (ov < best || (ov == best && oa < arg)) {
                best = ov;
                arg = oa;
            }
        }
        if (lane == 0) {
            int tau = arg;
            if (below != 0x7fffffff) {
                tau = below;
                while (tau + 1 <= tau_max - 1 && cv[tau + 1] < cv[tau]) ++tau;
            }
            const float ca = cv[tau - 1], cb = cv[tau], cg = cv[tau + 1];   // tau_min >= 2, tau <= tau_max - 1
            const float den = (ca - 2.f * cb) + cg;
            float shift = den > 0.f ? (0.5f * (ca - cg)) / den : 0.f;
            shift = fminf(fmaxf(shift, -1.f), 1.f);
            const float hz = rate / ((float)tau + shift);
            cl.out[f0 + f] = cb < threshold ? hz : 0.f;
            cl.out[cl.out_stride + f0 + f] = cb;
        }
    }
}

}  // namespace
}  // namespace wn

using namespace wn;

int wn_pitch_abi_version(void) { return WN_PITCH_ABI_VERSION; }
const char* wn_pitch_last_error(void) { return g_err; }

int wn_pitch(const WnPitchClip* clips, int n_clips, const float* table, int Q, int win, int hop, int tau_min, int tau_max,
             float threshold, float rate, void* stream) {
    WN_CHECK_ARG(clips, "wn_pitch: NULL clips");
    WN_CHECK_ARG(n_clips >= 1 && n_clips <= WN_PITCH_MAX_CLIPS, "wn_pitch: n_clips = %d outside 1 .. %d", n_clips, WN_PITCH_MAX_CLIPS);
    WN_CHECK_ARG(win >= 16 && win <= 4096, "wn_pitch: win = %d outside 16 .. 4096", win);
    WN_CHECK_ARG(hop >= 1, "wn_pitch: hop = %d < 1", hop);
    WN_CHECK_ARG(tau_min >= 2, "wn_pitch: tau_min = %d < 2", tau_min);
    WN_CHECK_ARG(tau_max >= tau_min + 2 && tau_max <= 2047, "wn_pitch: tau_max = %d outside tau_min + 2 = %d .. 2047", tau_max,
                 tau_min + 2);
    WN_CHECK_ARG(!table || Q >= 1, "wn_pitch: a decode table of Q = %d entries", Q);
    WN_CHECK_ARG(rate > 0.f, "wn_pitch: rate = %g is not positive", (double)rate);
    const int ft = tile_frames(tau_max);
    const int S = win + tau_max;
    const long long lds_bytes = lds_floats(win, hop, tau_max, ft) * 4;
    WN_CHECK_ARG(lds_bytes <= kLdsLimit,
                 "wn_pitch: a tile's segment of %d * hop + win + tau_max = %lld samples needs %lld bytes of LDS, the limit is %d "
                 "(hop = %d, win = %d, tau_max = %d)", ft - 1, (long long)(ft - 1) * hop + S, lds_bytes, kLdsLimit, hop, win, tau_max);
    PitchArgs args;
    long long tiles = 0;
    for (int c = 0; c < n_clips; ++c) {
        const WnPitchClip& cl = clips[c];
        WN_CHECK_ARG(cl.first >= 0 && cl.count >= 0, "wn_pitch: clip %d: first = %d or count = %d is negative", c, cl.first, cl.count);
        WN_CHECK_ARG(cl.out_stride >= cl.count, "wn_pitch: clip %d: out_stride = %lld below its %d frames", c,
                     (long long)cl.out_stride, cl.count);
        WN_CHECK_ARG((cl.flags & ~(WN_PITCH_START | WN_PITCH_END)) == 0, "wn_pitch: clip %d: flags = %u", c, cl.flags);
        WN_CHECK_ARG(cl.n >= 0 && cl.n < (1ll << 40) && cl.origin > -(1ll << 40) && cl.origin < (1ll << 40),
                     "wn_pitch: clip %d: n = %lld or origin = %lld out of range", c, (long long)cl.n, (long long)cl.origin);
        PitchClip& k = args.clip[c];
        k.x = cl.x;
        k.n = cl.n;
        k.base = cl.origin + (long long)cl.first * hop - S / 2;
        k.out = cl.out;
        k.out_stride = cl.out_stride;
        k.curve = cl.curve;
        k.count = cl.count;
        if (cl.count == 0) continue;
        WN_CHECK_ARG(cl.out && (cl.x || cl.n == 0), "wn_pitch: clip %d has a NULL buffer or output", c);
        const long long lo = k.base;                                                   // first sample read
        const long long hi = k.base + (long long)(cl.count - 1) * hop + S - 1;         // last sample read
        WN_CHECK_ARG(lo >= 0 || (cl.flags & WN_PITCH_START),
                     "wn_pitch: clip %d: frame %d reads sample %lld, before the buffer, and its start is not flagged as the signal's", c,
                     cl.first, lo);
        WN_CHECK_ARG(hi < cl.n || (cl.flags & WN_PITCH_END),
                     "wn_pitch: clip %d: frame %d reads sample %lld of %lld, and the buffer's end is not flagged as the signal's", c,
                     cl.first + cl.count - 1, hi, (long long)cl.n);
        tiles += (cl.count + ft - 1) / ft;
    }
    WN_CHECK_ARG(tiles < (1ll << 31), "wn_pitch: %lld frame tiles in one launch", tiles);
    if (tiles == 0) return WNP_OK;                                                     // nothing to do: nothing is launched
    args.n_clips = n_clips;
    const int items = ft * lag_groups(tau_max);
    const int threads = items >= kThreads ? kThreads : (items + 63) / 64 * 64;
    if (const int rc = raise_lds_limit(k_pitch, "k_pitch", lds_bytes)) return rc;
    hipLaunchKernelGGL(k_pitch, dim3((unsigned)tiles), dim3(threads), (size_t)lds_bytes, reinterpret_cast<hipStream_t>(stream), args,
                       table, Q, win, hop, tau_min, tau_max, threshold, rate, ft);
    return launch_status("wn_pitch");
}
