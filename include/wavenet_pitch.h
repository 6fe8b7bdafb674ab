/*
 * wavenet_pitch.h -- C ABI of libwavenet_pitch.so (MI355X / gfx950): YIN pitch tracking on the device.
 *
 * A library of its own next to libwavenet_hip.so and the log-mel, corpus and resample libraries, with their conventions: 0 on
 * success, WNP_EARG (-1) for a bad argument -- checked before any device work, wn_pitch_last_error() then names the value --
 * and WNP_EHIP (-3) for a failed HIP call; no allocation, no synchronisation, no table of its own, no environment variable
 * read; `stream` is a hipStream_t (NULL: the default stream); capturable in a HIP graph.
 *
 * The definition is wavenet_amd/pitch.py.  With S = win + tau_max, frame k of a clip is the S samples that start at signal index
 * k * hop - S / 2, zero outside the signal.  d[tau] = sum_{j = 0}^{win - 1} (s[j] - s[j + tau])^2 for tau = 0 .. tau_max, formed as
 * acc = fmaf(diff, diff, acc) for j ascending from acc = 0; r_tau = d[1] + ... + d[tau] in index order; c[0] = 1 and
 * c[tau] = d[tau] * tau / r_tau, or 1 where r_tau is not > 0.  Over tau_min .. tau_max - 1 the first tau with c[tau] < threshold
 * is taken and walked on while c[tau + 1] < c[tau] (voiced); if there is none, the first argmin (unvoiced).  With a, b, g =
 * c[tau* - 1], c[tau*], c[tau* + 1] and den = a - 2 b + g, shift = 0.5 (a - g) / den if den > 0 else 0, clamped to [-1, 1], and
 * f0 = rate / (tau* + shift).  out row 0 is f0 (0 for an unvoiced frame), row 1 is c[tau*]; row 0 > 0 exactly when
 * row 1 < threshold.
 * table == NULL: the buffers hold float32 samples; otherwise int32 tokens, and a sample is table[token] (Q entries, tokens
 * clamped into [0, Q)).
 * ONE launch covers up to WN_PITCH_MAX_CLIPS clips, each with its own buffer, frame range and outputs; a workgroup takes a few
 * consecutive frames of one clip and reads their samples into LDS once.  A column's bits (both rows and its row of `curve`)
 * depend on its own S samples and the scalar arguments alone: not on the frames, clips or calls it was computed with, nor on
 * `first` or `origin`, nor on whether the samples came as floats or as tokens.  No atomics.
 * A clip: frame f reads buffer samples origin + f * hop - S / 2 .. + S - 1; frames first .. first + count - 1 are written, frame
 * first + j to out[j] and out[out_stride + j], and its curve to curve[j * (tau_max + 1) ..].  A sample index below 0 is zero
 * when WN_PITCH_START says that the buffer's start is the signal's, one above n - 1 under WN_PITCH_END.
 * WNP_EARG, the message naming the value: win outside 16 .. 4096, hop < 1, tau_min < 2, tau_max outside tau_min + 2 .. 2047, a
 * workgroup's segment that does not fit the 160 KB of LDS, n_clips outside 1 .. WN_PITCH_MAX_CLIPS, out_stride < count, first
 * or count negative, and a frame that reaches past an edge of the buffer that is not flagged as the signal's.  `clips` is host
 * memory, read before the call returns.
 */
#ifndef WAVENET_PITCH_H
#define WAVENET_PITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define WN_PITCH_ABI_VERSION 1
#define WNP_OK    0
#define WNP_EARG -1
#define WNP_EHIP -3

#define WN_PITCH_MAX_CLIPS 64
#define WN_PITCH_START 1u
#define WN_PITCH_END 2u

typedef struct WnPitchClip {
    const void* x;          /* device: n float32 samples, or n int32 tokens */
    int64_t n;
    int64_t origin;         /* buffer index of frame 0's centre sample (k * hop maps to origin + k * hop); may be negative */
    float* out;             /* device: (2, count) with row stride out_stride floats: the f0 row, the aperiodicity row */
    int64_t out_stride;
    float* curve;           /* NULL, or device (count, tau_max + 1): the normalised difference, for tests and plots */
    int32_t first, count;
    uint32_t flags;         /* WN_PITCH_START / WN_PITCH_END: that edge of the buffer is the signal's, zero beyond it */
    int32_t reserved;
} WnPitchClip;

int wn_pitch_abi_version(void);
const char* wn_pitch_last_error(void);   /* thread-local; valid until the thread's next failing call */
int wn_pitch(const WnPitchClip* clips, int n_clips, const float* table, int Q, int win, int hop, int tau_min, int tau_max,
             float threshold, float rate, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WAVENET_PITCH_H */
