// Enrolment of a whole batch of jobs on the device: the batch form of the reference's trainingServer.py:170-247,312-398
// (largest face per pose image -> pose consistency -> mean -> duplicate check against the gallery AND against the rows
// the batch's own earlier jobs enrolled, in job order).  include/frhip.h fr_enrol_batch_f32 states the semantics.
//
// Four launches whatever J, I and N are, no allocation, no host synchronisation:
//   enrol_reduce          one workgroup per job: face selection, pairwise cosines, mean, unit row
//   first_above_blocked   the gallery first-hit scan for the jobs that got as far as a mean (fr_gallery_first_above_blocked_f32)
//   enrol_pair_flags      bit matrix flags[j] bit i = dot(q_j, r_i) > dup_thr, i < j
//   enrol_resolve         ONE workgroup walks the jobs in order over that matrix: the only sequential part
// Each launch reads what an earlier launch wrote; nothing a launch writes is read back by the same launch from global
// memory (the resolve step keeps its chain in LDS), and nothing mutable is `const __restrict__`.
//
// The arithmetic is the existing entries', through the device functions of match_scan.h: cosine_rows_wave
// (fr_cosine_matrix_f32), unit_row_wave4 (fr_gallery_update_rows_f32(normalise=1) == fr_l2norm_rows_f32 at D = 512, so the
// query q_j and the stored row r_j of a job are the same bits and ONE array holds both), row_dot_wave8
// (fr_gallery_first_above_f32); the mean is fr_mean_rows_f32's row-order sum divided by (float)K.
#include "match_scan.h"

#define EB_QB 16                                // queries a wave scores against each gallery row it loads
#define EB_U 2                                  // rows a wave has in flight
#define EB_WORDS (FR_ENROL_MAX_JOBS / 32)       // words of one row of the flag matrix
#define EB_PENDING 1                            // take[j]: the job got as far as a mean

static_assert(FR_ENROL_MAX_JOBS % 32 == 0 && FR_ENROL_MAX_POSES <= 64, "flag rows are whole words; one lane per pose");

// Sum over the wave of EB_QB values per lane, with wave_sum's pairing (xor offsets 32, 16, .., 1), so that every sum has
// wave_sum's bits: at offset o a lane keeps half of its values and hands the other half to lane ^ o, which keeps those
// (a + b == b + a: both lanes of a pair would have computed the same bits).  After offsets 32, 16, 8, 4 a lane holds ONE
// value, that of query (lane >> 2) summed over its 16-lane class; offsets 2 and 1 finish it.  17 cross-lane moves
// instead of 16 * 6.  Returns the sum of s[lane >> 2].
__device__ __forceinline__ float wave_sum_transposed16(float (&s)[EB_QB], int lane) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool hi = lane & 32;
        const float keep = hi ? s[i + 8] : s[i], send = hi ? s[i] : s[i + 8];
        s[i] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool hi = lane & 16;
        const float keep = hi ? s[i + 4] : s[i], send = hi ? s[i] : s[i + 4];
        s[i] = keep + __shfl_xor(send, 16, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const bool hi = lane & 8;
        const float keep = hi ? s[i + 2] : s[i], send = hi ? s[i] : s[i + 2];
        s[i] = keep + __shfl_xor(send, 8, 64);
    }
    const bool hi = lane & 4;
    const float keep = hi ? s[1] : s[0], send = hi ? s[0] : s[1];
    float v = keep + __shfl_xor(send, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// ---------------------------------------------------------------- blocked first-hit scan
// grid (row blocks, query blocks of EB_QB): a wave holds its 8 elements of EB_QB queries in registers, loads a gallery
// row's two float4s ONCE and scores all EB_QB queries against them; lane l then owns query q0 + (l >> 2).  The gallery
// is read once per query block, not once per query.  out_min[f]: (row << 32 | score bits), minimum over passing rows.
template <bool VIEW>
__global__ __launch_bounds__(256) void first_above_blocked(const float* __restrict__ Q, const float* __restrict__ G,
                                                           const int64_t* __restrict__ view,
                                                           const int32_t* __restrict__ take, int F, int64_t N, float thr,
                                                           int inclusive, unsigned long long* out_min) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.y * EB_QB;
    if (take) {                                  // a query block with nothing taken reads no gallery row
        bool any = false;
        for (int i = 0; i < EB_QB; ++i) any = any || (q0 + i < F && take[q0 + i] != 0);
        if (!any) return;
    }
    float qv[EB_QB][8];
#pragma unroll
    for (int i = 0; i < EB_QB; ++i) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (q0 + i < F) {
            const float4* q = reinterpret_cast<const float4*>(Q + (int64_t)(q0 + i) * GD + lane * 8);
            a = q[0]; b = q[1];
        }
        qv[i][0] = a.x; qv[i][1] = a.y; qv[i][2] = a.z; qv[i][3] = a.w;
        qv[i][4] = b.x; qv[i][5] = b.y; qv[i][6] = b.z; qv[i][7] = b.w;
    }
    const int myq = q0 + (lane >> 2);
    const bool active = myq < F && (!take || take[myq] != 0);
    unsigned long long best = ~0ull;
    for (int64_t base = ((int64_t)blockIdx.x * 4 + wave) * EB_U; base < N; base += (int64_t)gridDim.x * 4 * EB_U) {
        float4 g0[EB_U], g1[EB_U];
#pragma unroll
        for (int u = 0; u < EB_U; ++u) {
            const int64_t r = base + u < N ? base + u : N - 1;          // past the end: the last row again, not counted
            const int64_t slot = VIEW ? view[r] : r;
            const float4* g = reinterpret_cast<const float4*>(G + slot * GD + lane * 8);
            g0[u] = g[0]; g1[u] = g[1];
        }
#pragma unroll
        for (int u = 0; u < EB_U; ++u) {
            float s[EB_QB];
#pragma unroll
            for (int i = 0; i < EB_QB; ++i) s[i] = row_dot_lane8(qv[i], g0[u], g1[u]);
            const float t = wave_sum_transposed16(s, lane);
            const bool pass = active && base + u < N && (inclusive ? (t >= thr) : (t > thr));
            if (pass) {
                const unsigned long long key = ((unsigned long long)(base + u) << 32) | __float_as_uint(t);
                best = key < best ? key : best;
            }
        }
    }
    if ((lane & 3) == 0 && best != ~0ull) atomicMin(out_min + myq, best);
}

__global__ void first_above_blocked_finish(const unsigned long long* mins, const int32_t* __restrict__ take, int F,
                                           int64_t row_offset, int64_t* out_idx, float* out_score) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const unsigned long long k = mins[f];
    if (k == ~0ull || (take && take[f] == 0)) { out_idx[f] = -1; out_score[f] = 0.f; }
    else { out_idx[f] = (int64_t)(k >> 32) + row_offset; out_score[f] = __uint_as_float((unsigned)(k & 0xffffffffu)); }
}

static int scan_blocked_launch(const float* Q, const float* G, const int64_t* view, const int32_t* take, int F, int64_t N,
                               float thr, int inclusive, unsigned long long* mins, hipStream_t s) {
    int64_t bx = (N + 4 * EB_U - 1) / (4 * EB_U);
    bx = bx < 1 ? 1 : (bx > 1024 ? 1024 : bx);
    const dim3 grid((unsigned)bx, (unsigned)fr_cdiv(F, EB_QB));
    if (view && N > 0) first_above_blocked<true><<<grid, 256, 0, s>>>(Q, G, view, take, F, N, thr, inclusive, mins);
    else first_above_blocked<false><<<grid, 256, 0, s>>>(Q, G, nullptr, take, F, N, thr, inclusive, mins);
    FR_CHECK_LAUNCH("first_above_blocked");
    return FR_OK;
}

extern "C" int fr_gallery_first_above_blocked_f32(const float* Q, const float* G, const int64_t* view, const int32_t* take,
                                                  int F, int64_t N, int D, float thr, int inclusive, int64_t row_offset,
                                                  int64_t* out_idx, float* out_score, void* workspace,
                                                  size_t workspace_bytes, fr_stream_t stream) {
    FR_REQUIRE(D == GD, "fr_gallery_first_above_blocked_f32: D must be %d (got %d)", GD, D);
    if (F <= 0) return FR_OK;
    FR_REQUIRE(Q && out_idx && out_score && (G || N == 0) && N >= 0 && N < (1ll << 31),
               "fr_gallery_first_above_blocked_f32: bad argument");
    FR_REQUIRE(workspace && workspace_bytes >= (size_t)F * 8, "fr_gallery_first_above_blocked_f32: workspace needs %zu bytes",
               (size_t)F * 8);
    hipStream_t s = fr_stream(stream);
    unsigned long long* mins = reinterpret_cast<unsigned long long*>(workspace);
    if (hipMemsetAsync(mins, 0xff, (size_t)F * 8, s) != hipSuccess) {
        fr_set_error("fr_gallery_first_above_blocked_f32: memset failed");
        return FR_E_LAUNCH;
    }
    if (N > 0) {
        const int rc = scan_blocked_launch(Q, G, view, take, F, N, thr, inclusive, mins, s);
        if (rc != FR_OK) return rc;
    }
    first_above_blocked_finish<<<fr_cdiv(F, 64), 64, 0, s>>>(mins, take, F, row_offset, out_idx, out_score);
    FR_CHECK_LAUNCH("first_above_blocked_finish");
    return FR_OK;
}

// ---------------------------------------------------------------- per-job reduce
// One workgroup of 8 waves per job.  Whatever the index arrays hold, no row outside E [S] / bbox [S] is read: an image's
// first row is clamped into [0, S] and its count into [0, S - first]; a job's images into [0, I], FR_ENROL_MAX_POSES at most.
__global__ __launch_bounds__(512) void enrol_reduce(const float* __restrict__ E, const float* __restrict__ bbox, int S,
                                                    const int32_t* __restrict__ img_first,
                                                    const int32_t* __restrict__ img_count, int I,
                                                    const int32_t* __restrict__ job_first, float sim_thr, int32_t* status,
                                                    int32_t* pair, int32_t* face, float* avg, float* row,
                                                    unsigned long long* mins, int32_t* take) {
    constexpr int P = FR_ENROL_MAX_POSES, NPAIR = P * (P - 1) / 2;
    __shared__ int chosen[P];                    // per image of the job: the chosen row of E, -1 without a face
    __shared__ int found[P];                     // the K found rows, in image order
    __shared__ int K_s, bad_s;
    __shared__ float cosv[NPAIR];
    __shared__ __attribute__((aligned(16))) float avg_s[GD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x;
    int i0 = job_first[j], i1 = job_first[j + 1];
    i0 = i0 < 0 ? 0 : (i0 > I ? I : i0);
    i1 = i1 < i0 ? i0 : (i1 > I ? I : i1);
    if (i1 - i0 > P) i1 = i0 + P;
    // ---- 1. the first slot with the largest area, strict '>' in slot order (trainingServer.py:234-243)
    if (tid < P) {
        int pick = -1, slot = -1;
        if (i0 + tid < i1) {
            int first = img_first[i0 + tid], n = img_count[i0 + tid];
            first = first < 0 ? 0 : (first > S ? S : first);
            n = n < 0 ? 0 : (n > S - first ? S - first : n);
            float best = 0.f;
            for (int s = 0; s < n; ++s) {
                const float4 b = *reinterpret_cast<const float4*>(bbox + (int64_t)(first + s) * 4);
                const float w = b.z - b.x, h = b.w - b.y;
                const float area = w * h;
                if (s == 0 || area > best) { best = area; slot = s; }
            }
            if (slot >= 0) pick = first + slot;
            face[i0 + tid] = slot;
        }
        chosen[tid] = pick;
    }
    __syncthreads();
    if (tid == 0) {
        int K = 0;
        for (int p = 0; p < P; ++p) if (chosen[p] >= 0) found[K++] = chosen[p];
        K_s = K;
    }
    __syncthreads();
    const int K = K_s;
    // ---- 3. the pairwise cosines, pair p of the lexicographic order on wave p % 8
    {
        int p = 0;
        for (int a = 0; a < K; ++a)
            for (int b = a + 1; b < K; ++b, ++p)
                if ((p & 7) == wave) {
                    const float c = cosine_rows_wave(E + (int64_t)found[a] * GD, E + (int64_t)found[b] * GD, GD, lane);
                    if (lane == 0) cosv[p] = c;
                }
    }
    __syncthreads();
    if (tid == 0) {
        int bad = -1, pa = -1, pb = -1, p = 0;
        for (int a = 0; a < K && bad < 0; ++a)
            for (int b = a + 1; b < K; ++b, ++p)
                if (cosv[p] < sim_thr) { bad = p; pa = a; pb = b; break; }
        bad_s = bad;
        const int pending = K > 0 && bad < 0;
        status[j] = K == 0 ? FR_ENROL_NO_FACE : (bad >= 0 ? FR_ENROL_DIFFERENT : FR_ENROL_DONE);   // DONE: until the resolve step
        pair[2 * j] = pa; pair[2 * j + 1] = pb;
        take[j] = pending ? EB_PENDING : 0;
        mins[j] = ~0ull;
    }
    __syncthreads();
    const bool pending = K > 0 && bad_s < 0;
    // ---- 4. the mean: row-order sum / (float)K, not re-normalised (:355)
    float m = 0.f;
    if (pending) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += E[(int64_t)found[k] * GD + tid];
        m = s / (float)K;
    }
    avg[(int64_t)j * GD + tid] = m;
    avg_s[tid] = m;
    __syncthreads();
    // ---- 5. q = r = avg / ||avg||
    if (wave == 0) {
        float4 v0 = *reinterpret_cast<const float4*>(&avg_s[lane * 4]);
        float4 v1 = *reinterpret_cast<const float4*>(&avg_s[256 + lane * 4]);
        if (pending) unit_row_wave4(v0, v1);
        float* o = row + (int64_t)j * GD;
        *reinterpret_cast<float4*>(o + lane * 4) = v0;
        *reinterpret_cast<float4*>(o + 256 + lane * 4) = v1;
    }
}

// ---------------------------------------------------------------- in-batch flags
// workgroup j: flags[j] bit i = row_dot_wave8(q_j, r_i) > thr for the pending jobs i < j
__global__ __launch_bounds__(256) void enrol_pair_flags(const float* __restrict__ row, const int32_t* __restrict__ take,
                                                        float thr, uint32_t* flags) {
    __shared__ unsigned bits[EB_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x;
    if (tid < EB_WORDS) bits[tid] = 0u;
    __syncthreads();
    if (take[j] != 0) {
        const float4* q = reinterpret_cast<const float4*>(row + (int64_t)j * GD + lane * 8);
        const float4 a = q[0], b = q[1];
        const float qv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        for (int i = wave; i < j; i += 4) {
            if (take[i] == 0) continue;
            const float4* g = reinterpret_cast<const float4*>(row + (int64_t)i * GD + lane * 8);
            const float s = row_dot_wave8(qv, g[0], g[1]);
            if (lane == 0 && s > thr) atomicOr(&bits[i >> 5], 1u << (i & 31));
        }
    }
    __syncthreads();
    if (tid < EB_WORDS) flags[(int64_t)j * EB_WORDS + tid] = bits[tid];
}

// ---------------------------------------------------------------- resolve
// ONE workgroup.  Everything the chain needs is brought into LDS first; thread 0 then walks the jobs in order with the
// mask of `done` jobs (a gallery hit wins over an in-batch hit: gallery rows come first), the results leave in parallel.
__global__ __launch_bounds__(256) void enrol_resolve(const float* __restrict__ row, const int32_t* __restrict__ take,
                                                     const unsigned long long* __restrict__ mins,
                                                     const uint32_t* __restrict__ flags, int J, int64_t N,
                                                     int32_t* status, int64_t* dup_pos, float* dup_score) {
    __shared__ unsigned fl[FR_ENROL_MAX_JOBS * EB_WORDS];
    __shared__ unsigned long long mn[FR_ENROL_MAX_JOBS];
    __shared__ int tk[FR_ENROL_MAX_JOBS], hit[FR_ENROL_MAX_JOBS], st[FR_ENROL_MAX_JOBS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < J * EB_WORDS; e += 256) fl[e] = flags[e];
    for (int j = tid; j < J; j += 256) { mn[j] = mins[j]; tk[j] = take[j]; }
    __syncthreads();
    if (tid == 0) {
        unsigned done[EB_WORDS];
#pragma unroll
        for (int w = 0; w < EB_WORDS; ++w) done[w] = 0u;
        for (int j = 0; j < J; ++j) {
            int h = -1, s = -1;                                      // s: -1 = the reduce step's status stands
            if (tk[j] != 0) {
                if (mn[j] != ~0ull) s = FR_ENROL_DUPLICATE;
                else {
#pragma unroll
                    for (int w = EB_WORDS - 1; w >= 0; --w) {
                        const unsigned m = fl[j * EB_WORDS + w] & done[w];
                        if (m) h = w * 32 + __builtin_ctz(m);
                    }
                    if (h >= 0) s = FR_ENROL_DUPLICATE;
                    else {
                        s = FR_ENROL_DONE;
#pragma unroll
                        for (int w = 0; w < EB_WORDS; ++w) if (w == (j >> 5)) done[w] |= 1u << (j & 31);
                    }
                }
            }
            hit[j] = h; st[j] = s;
        }
    }
    __syncthreads();
    for (int j = tid; j < J; j += 256) {
        if (st[j] >= 0) status[j] = st[j];
        if (hit[j] >= 0) dup_pos[j] = N + hit[j];                    // its score: below
        else if (tk[j] != 0 && mn[j] != ~0ull) {
            dup_pos[j] = (int64_t)(mn[j] >> 32);
            dup_score[j] = __uint_as_float((unsigned)(mn[j] & 0xffffffffu));
        } else { dup_pos[j] = -1; dup_score[j] = 0.f; }
    }
    for (int j = wave; j < J; j += 4) {
        const int h = hit[j];
        if (h < 0) continue;
        const float4* q = reinterpret_cast<const float4*>(row + (int64_t)j * GD + lane * 8);
        const float4 a = q[0], b = q[1];
        const float qv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        const float4* g = reinterpret_cast<const float4*>(row + (int64_t)h * GD + lane * 8);
        const float s = row_dot_wave8(qv, g[0], g[1]);
        if (lane == 0) dup_score[j] = s;
    }
}

extern "C" size_t fr_enrol_batch_workspace(int J, int64_t N) {
    (void)N;                                     // the scan's partial results are one 64-bit word per job whatever N is
    const size_t j = (size_t)(J > 0 ? J : 1);
    return j * (sizeof(unsigned long long) + sizeof(int32_t) + EB_WORDS * sizeof(uint32_t)) + 256;
}

extern "C" int fr_enrol_batch_f32(const float* E, const float* bbox, int S, const int32_t* img_first,
                                  const int32_t* img_count, int I, const int32_t* job_first, int J, int max_poses, int D,
                                  const float* G, const int64_t* view, int64_t N, float sim_thr, float dup_thr,
                                  int32_t* status, int32_t* pair, int32_t* face, float* avg, float* row, int64_t* dup_pos,
                                  float* dup_score, void* workspace, size_t workspace_bytes, fr_stream_t stream) {
    FR_REQUIRE(D == GD, "fr_enrol_batch_f32: D must be %d (got %d)", GD, D);
    FR_REQUIRE(J >= 0 && I >= 0 && S >= 0 && N >= 0, "fr_enrol_batch_f32: negative size");
    if (J == 0) return FR_OK;
    FR_REQUIRE(J <= FR_ENROL_MAX_JOBS, "fr_enrol_batch_f32: at most %d jobs a batch (got %d)", FR_ENROL_MAX_JOBS, J);
    FR_REQUIRE(max_poses >= 0 && max_poses <= FR_ENROL_MAX_POSES, "fr_enrol_batch_f32: at most %d images a job (got %d)",
               FR_ENROL_MAX_POSES, max_poses);
    FR_REQUIRE(N < (1ll << 31), "fr_enrol_batch_f32: the gallery must have fewer than 2^31 rows");
    FR_REQUIRE(job_first && status && pair && face && avg && row && dup_pos && dup_score && (G || N == 0) &&
               ((E && bbox && img_first && img_count) || I == 0), "fr_enrol_batch_f32: null pointer");
    FR_REQUIRE(workspace && workspace_bytes >= fr_enrol_batch_workspace(J, N), "fr_enrol_batch_f32: workspace too small (%zu < %zu)",
               workspace_bytes, fr_enrol_batch_workspace(J, N));
    hipStream_t s = fr_stream(stream);
    unsigned long long* mins = reinterpret_cast<unsigned long long*>(workspace);
    int32_t* take = reinterpret_cast<int32_t*>(mins + J);
    uint32_t* flags = reinterpret_cast<uint32_t*>(take + J);
    enrol_reduce<<<J, 512, 0, s>>>(E, bbox, S, img_first, img_count, I, job_first, sim_thr, status, pair, face, avg, row,
                                   mins, take);
    FR_CHECK_LAUNCH("enrol_reduce");
    const int rc = scan_blocked_launch(row, G, view, take, J, N, dup_thr, 0, mins, s);       // N == 0: no row is read
    if (rc != FR_OK) return rc;
    enrol_pair_flags<<<J, 256, 0, s>>>(row, take, dup_thr, flags);
    FR_CHECK_LAUNCH("enrol_pair_flags");
    enrol_resolve<<<1, 256, 0, s>>>(row, take, mins, flags, J, N, status, dup_pos, dup_score);
    FR_CHECK_LAUNCH("enrol_resolve");
    return FR_OK;
}
