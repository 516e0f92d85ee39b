// The candidate list of the top-K kernels (match_topk.hip: the exact scan and its reduces; scan_gemm.hip: the certified
// re-rank of the coarse scan): KP = 2 / 4 / 8 / 16 (score, row) pairs in REGISTERS, best first, under the total order
// (score descending, row ascending); an empty slot is (-inf, -1) and loses to every row.  Every index into a list is a
// compile-time constant (fully unrolled loops): a dynamically indexed list would live in scratch memory.
//   insert:      the scan's step.  One compare drops a score that is not '>' the lane's K-th entry - rows ascend
//                within a lane, so an equal score with a higher row loses, as it must; otherwise an unrolled
//                compare-and-shift puts the pair behind every entry with score >= s.
//   merge:       the K best of two sorted lists, as a bitonic merge: c[j] = better(a[j], b[KP-1-j]) holds the K best
//                of both as a bitonic sequence, log2(KP) compare-exchange stages sort it.  Used by every merge level:
//                half-waves (__shfl_xor 32), waves (LDS), blocks (workspace), shards, re-scored coarse candidates.
#pragma once
#include "common.h"

#define TOPK_EMPTY_S (-INFINITY)

// a before b in the total order; rows are distinct among real candidates, all empty slots are equal
__device__ __forceinline__ bool topk_before(float as, int64_t ai, float bs, int64_t bi) {
    return ai >= 0 && (bi < 0 || as > bs || (as == bs && ai < bi));
}

template <int KP>
struct TopK {
    float s[KP];
    int64_t i[KP];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < KP; ++j) { s[j] = TOPK_EMPTY_S; i[j] = -1; }
    }

    // scan step: row gi ascends from call to call, s is finite or NaN (a NaN is never '>': never listed)
    __device__ __forceinline__ void insert(float v, int64_t gi) {
        if (!(v > s[KP - 1])) return;
#pragma unroll
        for (int j = KP - 1; j > 0; --j) {
            if (v > s[j - 1]) { s[j] = s[j - 1]; i[j] = i[j - 1]; }
            else if (v > s[j]) { s[j] = v; i[j] = gi; }
        }
        if (v > s[0]) { s[0] = v; i[0] = gi; }
    }

    // this = the KP best of this and o (both sorted)
    __device__ __forceinline__ void merge(const TopK& o) {
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (topk_before(o.s[KP - 1 - j], o.i[KP - 1 - j], s[j], i[j])) { s[j] = o.s[KP - 1 - j]; i[j] = o.i[KP - 1 - j]; }
#pragma unroll
        for (int d = KP / 2; d >= 1; d >>= 1) {
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                if ((j & d) == 0 && topk_before(s[j + d], i[j + d], s[j], i[j])) {
                    const float ts = s[j]; const int64_t ti = i[j];
                    s[j] = s[j + d]; i[j] = i[j + d];
                    s[j + d] = ts; i[j + d] = ti;
                }
            }
        }
    }

    __device__ __forceinline__ TopK shfl_xor(int mask) const {
        TopK o;
#pragma unroll
        for (int j = 0; j < KP; ++j) { o.s[j] = __shfl_xor(s[j], mask, 64); o.i[j] = __shfl_xor(i[j], mask, 64); }
        return o;
    }

    // entries [0, K) from ps / pi (stride 1), the rest empty
    __device__ __forceinline__ void load(const float* ps, const int64_t* pi, int K) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const bool in = j < K;
            s[j] = in ? ps[j] : TOPK_EMPTY_S;
            i[j] = in ? pi[j] : -1;
        }
    }

    __device__ __forceinline__ void store(float* ps, int64_t* pi, int K) const {
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < K) { ps[j] = s[j]; pi[j] = i[j]; }
    }
};
