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

// the query slot that lane r of a grouped scan's group owns (qmap: the group's QG entries), or -1: unmapped, outside
// [0, F), or padding under seg_counts.  The one test of the grouped scans' staging, early exit and reduce.
__device__ __forceinline__ int grouped_slot(const int32_t* __restrict__ qmap, int r, int F,
                                            const int32_t* seg_counts, int seg_len) {
    const int f = qmap[r];
    if (f < 0 || f >= F) return -1;
    if (seg_counts && !slot_valid(seg_counts, seg_len, f)) return -1;
    return f;
}

// a grouped scan's group (map: its QG entries) owns at least one real query slot; the same answer in every thread
__device__ __forceinline__ bool grouped_has_real(const int32_t* __restrict__ map, int F, const int32_t* seg_counts,
                                                 int seg_len) {
    for (int r = 0; r < QG; ++r)
        if (grouped_slot(map, r, F, seg_counts, seg_len) >= 0) return true;
    return false;
}

// The argument checks the grouped entries (fr_gallery_match_grouped_f32, fr_gallery_topk_grouped_f32) share, all
// before any launch.  FR_OK with *empty = true: nothing to do.
static inline int grouped_args_check(const char* who, const void* Q, const void* G, const void* views, const void* gtab,
                                     const void* qmap, int F, int ngroups, int64_t max_view_len, int64_t capacity, int D,
                                     const void* out_idx, const void* out_score, const void* workspace,
                                     size_t workspace_bytes, size_t need, const int32_t* seg_counts, int seg_len,
                                     bool* empty) {
    *empty = true;
    FR_REQUIRE(!seg_counts || (seg_len > 0 && F % seg_len == 0), "%s: seg_len must divide F", who);
    FR_REQUIRE(D == GD, "%s: D must be %d (got %d)", who, GD, D);
    FR_REQUIRE(F >= 0 && ngroups >= 0 && max_view_len >= 0, "%s: negative size", who);
    FR_REQUIRE(capacity >= 0 && capacity < (1ll << 31), "%s: capacity %lld must be below 2^31 slots", who,
               (long long)capacity);
    FR_REQUIRE(max_view_len < (1ll << 31), "%s: max_view_len %lld must be below 2^31 rows", who, (long long)max_view_len);
    FR_REQUIRE(ngroups <= 65535, "%s: at most 65535 groups (got %d)", who, ngroups);
    if (F == 0 || ngroups == 0) return FR_OK;
    FR_REQUIRE(Q && G && views && gtab && qmap && out_idx && out_score, "%s: null pointer", who);
    FR_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    *empty = false;
    return FR_OK;
}

// stage query group [q0, q0 + QG) of Q [F][GD] into qs [QG][QPAD] (zero rows beyond F); 256 threads, no barrier.
// map (optional, the grouped scans): row r is query slot map[r] instead of q0 + r, gathered from anywhere in Q; rows
// whose grouped_slot is -1 are staged as zero rows and never read from Q.
__device__ __forceinline__ void stage_query_group(const float* __restrict__ Q, int F, int q0, float* qs,
                                                  const int32_t* __restrict__ map = nullptr,
                                                  const int32_t* seg_counts = nullptr, int seg_len = 0) {
    for (int e = threadIdx.x; e < QG * (GD / 4); e += 256) {
        int r = e / (GD / 4), c = e % (GD / 4);
        const int f = map ? grouped_slot(map, r, F, seg_counts, seg_len) : q0 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (map ? f >= 0 : f < F) v = *reinterpret_cast<const float4*>(Q + (int64_t)f * GD + c * 4);
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

// One tile on v_mfma_f32_32x32x2_f32: A = 32 gallery rows, B = 32 queries.  The instruction is an exact k-ordered fmaf
// chain (measured, docs/KERNEL_NOTES.md 4.15: acc = fmaf(a1, b1, fmaf(a0, b0, acc)), one rounding each, subnormals kept), and
// instruction 4 kk + e takes element 8 kk + e from the h = 0 lanes (k slot 0) and 8 kk + 4 + e from the h = 1 lanes (k slot 1):
// a score is the fmaf chain over elements 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ...; tests/test_gpu_scan_pins.py pins its bits.
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
