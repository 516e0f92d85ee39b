// What the exact f32 gallery scans (match.hip: top-1, match_topk.hip: top-K) have in common: the geometry of a
// scan block, the padding test of a query group, the order of two candidates, the staging of a query group and
// the dot products of one 32-row gallery tile - and the per-row arithmetic (first-hit dot, cosine, unit row) that the
// first-hit consumers and the enrolment batch (enrol_batch.hip) share with the entries of match.hip.
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
// eight, g0 / g1: the row's): eight terms left to right (row_dot_lane8: one lane's share), then wave_sum.  The one arithmetic form of the first-hit
// consumers (gallery_first_above in match.hip, unknown_assign_batch in unknown_assign.hip): the library is built with
// -ffp-contract=off, so both get the same bits for the same row and query.
__device__ __forceinline__ float row_dot_lane8(const float (&qv)[8], const float4 g0, const float4 g1) {
    return qv[0] * g0.x + qv[1] * g0.y + qv[2] * g0.z + qv[3] * g0.w + qv[4] * g1.x + qv[5] * g1.y +
           qv[6] * g1.z + qv[7] * g1.w;
}
__device__ __forceinline__ float row_dot_wave8(const float (&qv)[8], const float4 g0, const float4 g1) {
    return wave_sum(row_dot_lane8(qv, g0, g1));
}

// cosine of two D-float rows by one wave, lane l taking elements l, l + 64, ...: the arithmetic of fr_cosine_matrix_f32
// (match.hip) and of the pose-consistency test of fr_enrol_batch_f32 (enrol_batch.hip); every lane returns the value.
__device__ __forceinline__ float cosine_rows_wave(const float* a, const float* b, int D, int lane) {
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float x = a[c], y = b[c];
        ab += x * y; aa += x * x; bb += y * y;
    }
    ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
    return ab / (sqrtf(aa) * sqrtf(bb));
}

// v / ||v|| of one 512-float row held by a wave as v0 = elements 4l .. 4l+3, v1 = elements 256 + 4l .. 256 + 4l+3: the
// arithmetic of fr_gallery_update_rows_f32(normalise=1), which is also that of fr_l2norm_rows_f32 at D = 512 (its sum
// starts from 0.f + the first four squares: the same bits).
__device__ __forceinline__ void unit_row_wave4(float4& v0, float4& v1) {
    float ss = v0.x * v0.x + v0.y * v0.y + v0.z * v0.z + v0.w * v0.w;
    ss += v1.x * v1.x + v1.y * v1.y + v1.z * v1.z + v1.w * v1.w;
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    v0.x /= nrm; v0.y /= nrm; v0.z /= nrm; v0.w /= nrm;
    v1.x /= nrm; v1.y /= nrm; v1.z /= nrm; v1.w /= nrm;
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
