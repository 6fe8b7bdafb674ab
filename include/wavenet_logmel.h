/*
 * wavenet_logmel.h -- C ABI of libwavenet_logmel.so (MI355X / gfx950): log-mel features on the device.
 *
 * A library of its own next to libwavenet_hip.so: that library's dynamic symbols are its header's functions and nothing
 * else, and the tests pin their number, so a front end that the network's kernels do not need lives beside it.  Same
 * conventions: 0 on success, WNL_EARG (-1) for a bad argument -- checked before any device work, wn_logmel_last_error()
 * then names the value -- and WNL_EHIP (-3) for a failed HIP call; no allocation, no synchronisation, no table of its own, no
 * environment variable read; `stream` is a hipStream_t (NULL: the default stream).
 *
 * The definition is wavenet_amd/features.py: frame f of a clip is the win samples centred on its sample f * hop, windowed
 * with the periodic Hann window; the value is log(max(filterbank . |rfft|, 1e-5)).  ONE launch covers up to
 * WN_LOGMEL_MAX_CLIPS clips, each with its own buffer, frame range and output; a workgroup takes 32 frames of one clip, reads
 * their samples once into LDS and contracts them on the exact-fp32 MFMA with the caller's tables:
 *   basis  (win, 2 * (win / 2 + 1)) float32, row n = [ w[n] cos(2 pi n b / win), b = 0 .. win / 2 | -w[n] sin(2 pi n b / win) ]
 *   fbT    (win / 2 + 1, n_mels) float32: the filterbank, one row per bin
 * table == NULL: the buffers hold float32 samples; otherwise int32 tokens, and a sample is table[token] (Q entries, tokens
 * clamped into [0, Q)).
 * A cell's bits depend on its own win samples, basis and fbT alone: not on the frames, clips or calls it was computed with, nor
 * on whether the samples came as floats or as tokens (the sums run over taps, then over bins, each in index order).
 * A clip: frame f reads buffer samples origin + f * hop - win / 2 .. + win - 1; frames first .. first + count - 1 are written,
 * frame first + j to out[i * out_stride + j] for filter i.  A sample index below 0 is read at its mirror image -index when
 * WN_LOGMEL_REFLECT_LEFT says that the buffer's start is the signal's, one above n - 1 at 2 (n - 1) - index under
 * WN_LOGMEL_REFLECT_RIGHT.  WNL_EARG, the message naming the value: win odd or outside 16 .. 4096, hop < 1, n_mels outside
 * 1 .. 256, a 32-frame segment (31 hop + win samples) that does not fit the 160 KB of LDS, n_clips outside
 * 1 .. WN_LOGMEL_MAX_CLIPS, a clip of n <= win / 2 samples, out_stride < count, and a frame that reaches past an end of the
 * buffer that is not flagged (or further than a reflection reaches).  `clips` is host memory, read before the call returns.
 */
#ifndef WAVENET_LOGMEL_H
#define WAVENET_LOGMEL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define WN_LOGMEL_ABI_VERSION 1
#define WNL_OK    0
#define WNL_EARG -1
#define WNL_EHIP -3

#define WN_LOGMEL_MAX_CLIPS 64
#define WN_LOGMEL_REFLECT_LEFT 1u
#define WN_LOGMEL_REFLECT_RIGHT 2u

typedef struct WnLogmelClip {
    const void* x;          /* device: n float32 samples, or n int32 tokens */
    int64_t n;
    int64_t origin;         /* buffer index of frame 0's centre; may be negative (a buffer that starts inside the signal) */
    float* out;             /* device: (n_mels, count) with row stride out_stride floats */
    int64_t out_stride;
    int32_t first, count;
    uint32_t flags;         /* WN_LOGMEL_REFLECT_* */
    int32_t reserved;
} WnLogmelClip;

int wn_logmel_abi_version(void);
const char* wn_logmel_last_error(void);   /* thread-local; valid until the thread's next failing call */
int wn_logmel(const WnLogmelClip* clips, int n_clips, const float* table, int Q, const float* basis, const float* fbT, int win,
              int hop, int n_mels, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WAVENET_LOGMEL_H */
