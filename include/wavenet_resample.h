/*
 * wavenet_resample.h -- C ABI of libwavenet_resample.so (MI355X / gfx950): sample-rate conversion on the device.
 *
 * A library of its own next to libwavenet_hip.so, libwavenet_logmel.so and libwavenet_corpus.so, with their conventions: 0 on
 * success, WNR_EARG (-1) for a bad argument -- checked before any device work, wn_resample_last_error() then names the value --
 * and WNR_EHIP (-3) for a failed HIP call; no allocation, no synchronisation, no table of its own, no environment variable
 * read; `stream` is a hipStream_t (NULL: the default stream); capturable in a HIP graph.
 *
 * The definition is wavenet_amd/resample.py: a polyphase converter by L / M.  With q, phi = divmod(n M, L) and Kt = (T - 1) / 2,
 * output n of a signal x is   sum_{t = 0}^{T - 1} taps[phi * T + t] * x[q + Kt - t],   x zero outside the signal, formed as
 * acc = fmaf(tap, sample, acc) for t = 0 .. T - 1 in that order from acc = 0.  `taps` is the caller's (L, T) float32 table.
 * ONE launch covers up to WN_RESAMPLE_MAX_CLIPS clips, each with its own buffer, range of outputs and output array; a workgroup
 * takes WN_RESAMPLE_TILE consecutive outputs of one clip and reads the input span they need into LDS once.
 *   in_kind   WN_RESAMPLE_IN_PCM16: int16 samples, a sample is v / 32768 (exact in fp32); WN_RESAMPLE_IN_F32: float32 samples
 *   out_kind  WN_RESAMPLE_OUT_F32: the sum; WN_RESAMPLE_OUT_PCM16: int16 clamp(rintf(sum * 32768), -32768, 32767);
 *             WN_RESAMPLE_OUT_TOKENS: int32 lut[pcm + 32768], `lut` the 65,536-entry table of wn_mulaw_encode_pcm16
 * An output's bits depend on its own T input samples and `taps` alone: not on the outputs, clips or calls it was computed with,
 * nor on where the buffer starts inside the signal, nor on whether the samples came as int16 or as the same values in float32.
 * WNR_EARG, the message naming the value: L or M outside 1 .. 1024, L == M, T even or outside 3 .. 2047, a tile whose input
 * span does not fit the 160 KB of LDS, n_clips outside 1 .. WN_RESAMPLE_MAX_CLIPS, an unknown kind, token output without `lut`,
 * count < 0, first < 0, origin < 0 (or not 0 under WN_RESAMPLE_START), and an output whose T samples reach past an end of the
 * buffer that is not flagged as the signal's.  `clips` is host memory, read before the call returns.
 */
#ifndef WAVENET_RESAMPLE_H
#define WAVENET_RESAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define WN_RESAMPLE_ABI_VERSION 1
#define WNR_OK    0
#define WNR_EARG -1
#define WNR_EHIP -3

#define WN_RESAMPLE_MAX_CLIPS 64
#define WN_RESAMPLE_TILE 256
#define WN_RESAMPLE_START 1u
#define WN_RESAMPLE_END 2u
#define WN_RESAMPLE_IN_PCM16 0
#define WN_RESAMPLE_IN_F32 1
#define WN_RESAMPLE_OUT_F32 0
#define WN_RESAMPLE_OUT_PCM16 1
#define WN_RESAMPLE_OUT_TOKENS 2

typedef struct WnResampleClip {
    const void* x;          /* device buffer: n int16 PCM (a sample is v / 32768, exact in fp32) or n float32 samples */
    int64_t n;
    int64_t origin;         /* absolute input index of x[0] (>= 0): a buffer may start inside the signal */
    void* out;              /* device: count float32, int16 PCM or int32 tokens */
    int64_t first, count;   /* absolute output indices first .. first + count - 1 */
    uint32_t flags;         /* WN_RESAMPLE_START: x[0] is the signal's first sample, what lies before it is zero;
                               WN_RESAMPLE_END: x[n - 1] is its last, what lies behind it is zero */
    int32_t reserved;
} WnResampleClip;

int wn_resample_abi_version(void);
const char* wn_resample_last_error(void);   /* thread-local; valid until the thread's next failing call */
int wn_resample(const WnResampleClip* clips, int n_clips, int in_kind, int out_kind, const float* taps, int L, int M, int T,
                const int32_t* lut /* 65,536 entries for token output, else NULL */, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WAVENET_RESAMPLE_H */
