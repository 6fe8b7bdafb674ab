/*
 * wavenet_corpus.h -- C ABI of libwavenet_corpus.so (MI355X / gfx950): training crops gathered from a corpus that is resident
 * on the device, B crops of any files in ONE launch.
 *
 * A library of its own next to libwavenet_hip.so and libwavenet_logmel.so, for the reason wavenet_logmel.h gives: the first
 * library's dynamic symbols are pinned by its header.  Same conventions: 0 on success, WNC_EARG (-1) for a bad argument --
 * checked before any device work, wn_corpus_last_error() then names the value -- and WNC_EHIP (-3) for a failed HIP call; no
 * allocation, no synchronisation, no table of its own, no environment variable read; `stream` is a hipStream_t (NULL: the
 * default stream).  The call enqueues one kernel and nothing else, so it can be captured in a HIP graph; `desc` is host
 * memory, read before the call returns, every pointer inside it is device memory, read when the kernel runs.
 *
 * The corpus (WnCorpusDesc):
 *   tokens       all files' tokens back to back: uint8 (token_bytes = 1) or int32 (token_bytes = 4).  A file starts at ANY
 *                element offset; nothing is assumed about its alignment.
 *   file_offset  (n_files) int64: element index of a file's first token      file_len  (n_files) int32: its tokens
 *   file_class   (n_files) int64 class id of a file, or NULL
 *   features     (F, total_cols) float32 with row stride total_cols: all files' columns back to back; NULL: no features
 *   col_offset   (n_files) int64: a file's first column                      col_count (n_files) int32: its columns (>= 1)
 *   hop samples per column; input_width silence tokens stand in front of every file; pad_cols = ceil(input_width / hop);
 *   shift = pad_cols * hop - input_width.
 *
 * The rule.  The padded signal of file f is p(i) = silence for i < input_width, else tokens[file_offset[f] + i - input_width].
 * `draws` is a device (B, 2) int32 array of (file, start) pairs; for crop b = (f, s), with W = input_width + target_width:
 *   x[b, j]   = p(s + j)                    j < W                   int32 (B, W)
 *   tgt[b, j] = p(s + input_width + 1 + j)  j < target_width        int32 (B, target_width)
 *   cond[b]   = file_class[f]               written only when cond and file_class are both given
 *   local[b, i, c] = features[i, col_offset[f] + clamp(first + c - pad_cols, 0, col_count[f] - 1)],  first = (s + shift) / hop,
 *                    i < F, c < n_cols      float32 (B, F, n_cols); written only when the corpus has features
 * A start is legal in [0, file_len[f] - target_width - 1).  The kernel cannot refuse, so it fences: a file index is clamped into
 * [0, n_files) and a start into the legal range, once per workgroup, and a position at or past the file's end reads as silence
 * -- a bad draw never takes a read outside its file's own tokens or columns.  Refusing bad draws is the caller's business.
 *
 * WNC_EARG, the message naming the value: a NULL desc, draws, x or tgt; NULL tokens, file_offset or file_len; token_bytes
 * not 1 or 4; n_files < 1; B < 1; target_width < 1; input_width < 0; a silence token outside the token type; with features:
 * NULL col_offset, col_count or local, F < 1, hop < 1, n_cols < 1, total_cols < 1, pad_cols or shift that are not the values
 * above; outputs of 2^31 elements or more per array.
 */
#ifndef WAVENET_CORPUS_H
#define WAVENET_CORPUS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define WN_CORPUS_ABI_VERSION 1
#define WNC_OK    0
#define WNC_EARG -1
#define WNC_EHIP -3

typedef struct WnCorpusDesc {
    const void* tokens;
    const int64_t* file_offset;
    const int32_t* file_len;
    const int64_t* file_class;      /* or NULL */
    const float* features;          /* or NULL: the four fields below and F, hop, pad_cols, shift are then unused */
    const int64_t* col_offset;
    const int32_t* col_count;
    int64_t total_cols;
    int32_t n_files;
    int32_t token_bytes;            /* 1: uint8 tokens, 4: int32 tokens */
    int32_t F, hop;
    int32_t input_width, silence;
    int32_t pad_cols, shift;
} WnCorpusDesc;

int wn_corpus_abi_version(void);
const char* wn_corpus_last_error(void);   /* thread-local; valid until the thread's next failing call */
int wn_corpus_gather(const WnCorpusDesc* desc, const int32_t* draws, int B, int target_width, int n_cols, int32_t* x, int32_t* tgt,
                     float* local, int64_t* cond, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* WAVENET_CORPUS_H */
