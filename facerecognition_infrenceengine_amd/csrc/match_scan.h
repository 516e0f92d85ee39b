// What the exact f32 gallery scans (match.hip: top-1, match_topk.hip: top-K) have in common: the geometry of a
// scan block, the padding test of a query group, the order of two candidates, the staging of a query group and
// the dot products of one 32-row gallery tile.
#pragma once
#include "common.h"

#define GD 512          // embedding dim
#define QPAD 516        // LDS row stride (floats) for the query tile: breaks the 2 KB bank stride
#define QG 32           // queries per group (MFMA N)

__device__ __forceinline__ bool group_has_valid(const int32_t* seg_counts, int seg_len, int qa, int qb) {
    // [qa, qb) spans at most a few segments; a segment contributes iff its first slot inside the range is real
    for (int q = qa; q < qb;) {
        if (slot_valid(seg_counts, seg_len, q)) return true;
        q = (q / seg_len + 1) * seg_len;
    }
    return false;
}

__device__ __forceinline__ void take_better(float& bs, int64_t& bi, float s, int64_t i) {
    // max score; lowest index on exact ties (== first maximum in row order)
    if (s > bs || (s == bs && i < bi && i >= 0)) { bs = s; bi = i; }
}

// blocks along x of a scan grid: 4 waves per block, one 32-row tile per wave and step
static inline int scan_blocks(int64_t N) {
    int64_t tiles = (N + 31) / 32;
    int64_t b = (tiles + 3) / 4;
    if (b < 1) b = 1;
    if (b > 1024) b = 1024;
    return (int)b;
}

// stage query group [q0, q0 + QG) of Q [F][GD] into qs [QG][QPAD] (zero rows beyond F); 256 threads, no barrier
__device__ __forceinline__ void stage_query_group(const float* __restrict__ Q, int F, int q0, float* qs) {
    for (int e = threadIdx.x; e < QG * (GD / 4); e += 256) {
        int r = e / (GD / 4), c = e % (GD / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q0 + r < F) v = *reinterpret_cast<const float4*>(Q + (int64_t)(q0 + r) * GD + c * 4);
        *reinterpret_cast<float4*>(&qs[r * QPAD + c * 4]) = v;
    }
}

// dot of one 512-float row with a query spread over a wave, lane l holding elements 8l .. 8l+7 of both (qv: the query's
// eight, g0 / g1: the row's): eight terms left to right, then wave_sum.  The one arithmetic form of the first-hit
// consumers (gallery_first_above in match.hip, unknown_assign_batch in unknown_assign.hip): the library is built with
// -ffp-contract=off, so both get the same bits for the same row and query.
__device__ __forceinline__ float row_dot_wave8(const float (&qv)[8], const float4 g0, const float4 g1) {
    float s = qv[0] * g0.x + qv[1] * g0.y + qv[2] * g0.z + qv[3] * g0.w + qv[4] * g1.x + qv[5] * g1.y +
              qv[6] * g1.z + qv[7] * g1.w;
    return wave_sum(s);
}

// One tile on v_mfma_f32_32x32x2_f32 (an exact k-ordered fmaf chain): A = 32 gallery rows, B = 32 queries.
// gp = this lane's gallery row + 4 * h, qp = this lane's staged query + 4 * h (h = lane >> 5); a row past the
// end (ok == false) contributes zeros.  acc[reg] = score(tile row (reg & 3) + 8 * (reg >> 2) + 4 * h, query lane & 31).
__device__ __forceinline__ float16v scan_tile_f32(const float* __restrict__ gp, const float* qp, bool ok) {
    float16v acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int kk = 0; kk < GD / 8; ++kk) {
        float4 a = *reinterpret_cast<const float4*>(gp + kk * 8);
        float4 b = *reinterpret_cast<const float4*>(qp + kk * 8);
        if (!ok) a = make_float4(0.f, 0.f, 0.f, 0.f);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    return acc;
}
