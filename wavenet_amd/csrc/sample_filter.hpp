// Truncation of a categorical distribution before the draw: top-k, then top-p (nucleus) relative to the mass top-k kept.
// An extension of the reference's draw (train_audio/generate.py:39 samples the raw softmax); the contract, shared with
// wavenet_amd/sampling.py, is order-exact -- integer ranks and float64 sums in index order on the given fp32 row:
//   order   j precedes i  iff  p[j] > p[i], or p[j] == p[i] and j < i;  rank(i) = number of tokens preceding i
//   top-k   pk[i] = rank(i) < top_k ? p[i] : 0
//   top-p   total = sum_q pk[q];  before(i) = sum of pk[j] over the j preceding i  (both float64, index order);
//           keep i  iff  before(i) < top_p * total  (the rank-0 token always)
//   result  excluded entries become 0.0f, kept entries keep their fp32 value (no renormalisation: the draw divides by
//           the float64 total of the row it is given).
// One device function for every sampler (k_decode, draw_token -- the one draw of k_decode_fast and of workgroup 0 of
// k_decode_fast3 / _batch -- and the standalone k_sample_filtered): the row sits in LDS, all `nt` threads of the workgroup call it behind a
// workgroup-uniform branch, it works in place and holds its decisions in a register bit mask (one bit per token of the
// thread: Q <= 32 * nt).  No global-memory traffic.
#pragma once
#include <cmath>
namespace wn {

// the argument rules of wn_decoder_set_sampling and wn_sample_categorical_filtered (host; no HIP call)
static inline int check_sampling(const char* who, float temperature, int top_k, double top_p) {
    WN_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "%s: temperature must be finite and > 0", who);
    WN_CHECK_ARG(top_k >= 0, "%s: top_k must be >= 0 (0 = off), got %d", who, top_k);
    WN_CHECK_ARG(top_p > 0.0 && top_p <= 1.0, "%s: top_p must lie in (0, 1]", who);      // false for NaN
    return WN_OK;
}

// LDS_ONLY: wait for this wave's LDS traffic only (the persistent fast kernels keep global loads in flight across their
// barriers); otherwise __syncthreads()
template <bool LDS_ONLY>
__device__ __forceinline__ void filter_barrier() {
    if (LDS_ONLY) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    } else {
        __syncthreads();
    }
}

// top_k: 0 = off, else 1 .. Q-1;  top_p: >= 1 = off, else in (0, 1).  On entry the row is complete (a barrier lies behind
// its last write); on return it is filtered and a barrier lies behind the last write again.
template <bool LDS_ONLY>
__device__ __forceinline__ void sample_filter(float* __restrict__ p, const int Q, const int tid, const int nt,
                                              const int top_k, const double top_p) {
    if (top_k > 0) {
        // pass 1: the rank of this thread's token(s), every thread reading the same address (LDS broadcast)
        unsigned keep = 0u;
        int b = 0;
        for (int i = tid; i < Q; i += nt, ++b) {
            const float mine = p[i];
            int rank = 0;
#pragma unroll 8
            for (int j = 0; j < Q; ++j) {
                const float v = p[j];
                rank += (v > mine || (v == mine && j < i)) ? 1 : 0;
            }
            keep |= (rank < top_k ? 1u : 0u) << b;
        }
        filter_barrier<LDS_ONLY>();                 // every rank is counted: the row may change
        b = 0;
        for (int i = tid; i < Q; i += nt, ++b)
            if (!((keep >> b) & 1u)) p[i] = 0.f;
        filter_barrier<LDS_ONLY>();
    }
    if (top_p < 1.0) {
        // pass 2: float64 sums in index order, written as adds of selected values (nothing a fused multiply-add could
        // contract); every thread computes the same `total` in the same order, so there is nothing to reduce.  A token
        // top-k excluded is 0 here: it adds nothing to any sum, and stays 0 whatever this pass decides about it.
        unsigned keep = 0u;
        int b = 0;
        for (int i = tid; i < Q; i += nt, ++b) {
            const float mine = p[i];
            double total = 0.0, before = 0.0;
            int npre = 0;
#pragma unroll 4
            for (int j = 0; j < Q; ++j) {
                const float v = p[j];
                const bool pre = v > mine || (v == mine && j < i);
                const double dv = (double)v;
                total += dv;
                before += pre ? dv : 0.0;
                npre += pre ? 1 : 0;
            }
            const double thr = top_p * total;       // one float64 multiply, then a compare
            keep |= ((before < thr || npre == 0) ? 1u : 0u) << b;
        }
        filter_barrier<LDS_ONLY>();
        b = 0;
        for (int i = tid; i < Q; i += nt, ++b)
            if (!((keep >> b) & 1u)) p[i] = 0.f;
        filter_barrier<LDS_ONLY>();
    }
}

// what the host hands the kernels: everything that is off is normalised to its "skip" value
struct SampleCtl {
    float inv_temp = 1.f;      // 1 / temperature, computed once on the host in fp32; exactly 1 = no multiply
    int top_k = 0;             // 0 = off (also what top_k >= Q becomes at launch)
    double top_p = 1.0;        // 1 = off
};

}  // namespace wn
