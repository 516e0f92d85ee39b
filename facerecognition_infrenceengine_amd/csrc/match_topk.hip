// Exact top-K gallery identification: the K best rows per query under the total order (score descending, row
// ascending) among rows whose score is > -1 - the reference loop's rule (best starts at -1, strict '>', first
// maximum) extended from 1 to K.  Scores are the same k-ordered f32 MFMA chains as gallery_scan_f32 (match.hip; what the
// chain is was measured: scan_tile_f32 in match_scan.h, docs/KERNEL_NOTES.md 4.15), so column 0 is bit-identical to the
// top-1 match for every K.
//
// The candidate list (TopK<KP>: registers only, insert for the scan's step, a bitonic merge for every merge level) is
// topk_list.h's; the certified re-rank of the coarse scan (scan_gemm.hip) sorts with the same merge.
#include "match_scan.h"
#include "topk_list.h"

// Same orientation and arithmetic as scan_group_best (match.hip): a lane owns ONE query and 16 rows of a tile, its list
// is lane-local inside the scan.  The whole block calls it (barriers inside) after the barrier that ends the staging of
// qs; VIEW as there.  On return threads 0 .. 31 hold the block's list of query lane tid; qs is overwritten.
template <bool VIEW, int KP>
__device__ __forceinline__ TopK<KP> scan_group_topk(const float* __restrict__ G, const int64_t* __restrict__ view,
                                                    int64_t N, float* qs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    TopK<KP> top;
    top.clear();
    const int64_t ntiles = (N + 31) / 32;
    for (int64_t t = (int64_t)blockIdx.x * 4 + wave; t < ntiles; t += (int64_t)gridDim.x * 4) {
        const int64_t row = t * 32 + r;
        const bool ok = row < N;
        const int64_t slot = VIEW ? (ok ? view[row] : 0) : (ok ? row : 0);
        const float16v acc = scan_tile_f32(G + slot * GD + 4 * h, &qs[r * QPAD + 4 * h], ok);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int64_t gi = t * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;   // ascends with reg and t
            if (gi < N) top.insert(acc[reg], gi);
        }
    }
    // the two half-waves that hold the same query, then the 4 waves through LDS
    top.merge(top.shfl_xor(32));
    __syncthreads();
    float* ls = qs;                                                          // reuse LDS: 4 x 32 lists
    int64_t* li = reinterpret_cast<int64_t*>(qs + 4 * 32 * KP);
    if (h == 0 && wave > 0) top.store(ls + (wave * 32 + r) * KP, li + (wave * 32 + r) * KP, KP);
    __syncthreads();
    if (tid < 32) {
        for (int w = 1; w < 4; ++w) {
            TopK<KP> o;
            o.load(ls + (w * 32 + tid) * KP, li + (w * 32 + tid) * KP, KP);
            top.merge(o);
        }
    }
    return top;
}

// Partial lists go to ws_score / ws_idx [gridDim.x][F][K].
template <bool VIEW, int KP>
__global__ __launch_bounds__(256) void gallery_scan_topk_f32(const float* __restrict__ Q, const float* __restrict__ G,
                                                             const int64_t* __restrict__ view, int F, int64_t N, int K,
                                                             float* __restrict__ ws_score, int64_t* __restrict__ ws_idx,
                                                             const int32_t* __restrict__ seg_counts, int seg_len) {
    __shared__ __attribute__((aligned(16))) float qs[QG * QPAD];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.y * QG;
    // a group made of padding only does no work (the reduce reports empty lists for every padding slot)
    if (seg_counts && !group_has_valid(seg_counts, seg_len, q0, min(q0 + QG, F))) return;
    stage_query_group(Q, F, q0, qs);
    __syncthreads();
    TopK<KP> top = scan_group_topk<VIEW, KP>(G, view, N, qs);
    if (tid < 32 && q0 + tid < F) {
        const int64_t at = ((int64_t)blockIdx.x * F + q0 + tid) * K;
        top.store(ws_score + at, ws_idx + at, K);
    }
}

// GROUPED (see gallery_scan_grouped_f32, match.hip): block (x, g) scans the query slots qmap[g * QG ..] names through
// view views[gtab[2g] .. + gtab[2g + 1]); partial lists go to ws [gridDim.x][ngroups * QG][K], entry g * QG + lane.
template <int KP>
__global__ __launch_bounds__(256) void gallery_scan_topk_grouped_f32(const float* __restrict__ Q, const float* __restrict__ G,
                                                                     const int64_t* __restrict__ views,
                                                                     const int64_t* __restrict__ gtab,
                                                                     const int32_t* __restrict__ qmap, int F,
                                                                     int K, float* __restrict__ ws_score,
                                                                     int64_t* __restrict__ ws_idx,
                                                                     const int32_t* __restrict__ seg_counts, int seg_len) {
    __shared__ __attribute__((aligned(16))) float qs[QG * QPAD];
    const int tid = threadIdx.x, g = blockIdx.y;
    const int64_t N = gtab[2 * g + 1];
    const int32_t* map = qmap + (int64_t)g * QG;
    if (N <= 0 || !grouped_has_real(map, F, seg_counts, seg_len)) return;
    const int64_t at = ((int64_t)blockIdx.x * gridDim.y * QG + g * QG + tid) * K;
    TopK<KP> top;
    if ((int64_t)blockIdx.x * 4 >= (N + 31) / 32) {       // no tile of this view falls to this block: empty lists, no staging
        top.clear();
        if (tid < 32) top.store(ws_score + at, ws_idx + at, K);
        return;
    }
    stage_query_group(Q, F, 0, qs, map, seg_counts, seg_len);
    __syncthreads();
    top = scan_group_topk<true, KP>(G, views + gtab[2 * g], N, qs);
    if (tid < 32) top.store(ws_score + at, ws_idx + at, K);
}

// One wave per map entry: gallery_topk_reduce over ws [nblk][ngroups * QG][K], the list written to the query slot the
// entry names; an entry that names none writes nothing.  Empty view or padding slot: (-1, -1.0) everywhere.
template <int KP>
__global__ __launch_bounds__(256) void gallery_topk_reduce_grouped(const float* __restrict__ ws_score,
                                                                   const int64_t* __restrict__ ws_idx, int nblk,
                                                                   int ngroups, const int64_t* __restrict__ gtab,
                                                                   const int32_t* __restrict__ qmap, int F, int K,
                                                                   int64_t* __restrict__ out_idx,
                                                                   float* __restrict__ out_score,
                                                                   const int32_t* __restrict__ seg_counts, int seg_len) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= ngroups * QG) return;
    const int f = qmap[e];
    if (f < 0 || f >= F) return;
    TopK<KP> top;
    top.clear();
    if (gtab[2 * (e / QG) + 1] > 0 && (!seg_counts || slot_valid(seg_counts, seg_len, f))) {
        for (int b = lane; b < nblk; b += 64) {
            TopK<KP> o;
            const int64_t at = ((int64_t)b * ngroups * QG + e) * K;
            o.load(ws_score + at, ws_idx + at, K);
            top.merge(o);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) top.merge(top.shfl_xor(m));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            if (j < K) {
                const bool has = top.i[j] >= 0 && top.s[j] > -1.0f;
                out_idx[(int64_t)f * K + j] = has ? top.i[j] : -1;
                out_score[(int64_t)f * K + j] = has ? top.s[j] : -1.0f;
            }
        }
    }
}

// One wave per query: lane l merges the lists of blocks l, l + 64, ..., six __shfl_xor levels merge the lanes, lane 0
// applies row_offset, the '> -1' rule and the padding rule.
template <int KP>
__global__ __launch_bounds__(256) void gallery_topk_reduce(const float* __restrict__ ws_score,
                                                           const int64_t* __restrict__ ws_idx, int nblk, int F, int K,
                                                           int64_t row_offset, int64_t* __restrict__ out_idx,
                                                           float* __restrict__ out_score,
                                                           const int32_t* __restrict__ seg_counts, int seg_len) {
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= F) return;
    TopK<KP> top;
    top.clear();
    if (!seg_counts || slot_valid(seg_counts, seg_len, f)) {
        for (int b = lane; b < nblk; b += 64) {
            TopK<KP> o;
            const int64_t at = ((int64_t)b * F + f) * K;
            o.load(ws_score + at, ws_idx + at, K);
            top.merge(o);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) top.merge(top.shfl_xor(m));
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            if (j < K) {
                // reference: best_score starts at -1 and only a strictly larger score replaces it
                const bool has = top.i[j] >= 0 && top.s[j] > -1.0f;
                out_idx[(int64_t)f * K + j] = has ? top.i[j] + row_offset : -1;
                out_score[(int64_t)f * K + j] = has ? top.s[j] : -1.0f;
            }
        }
    }
}

// cand int32 [R][n][K][3] (score bits, row lo, row hi; row < 0: empty): the K best of the R lists of each query
template <int KP>
__global__ __launch_bounds__(64) void match_reduce_shards_topk(const int32_t* __restrict__ cand, int R, int n, int K, int q0, int F,
                                         int64_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    TopK<KP> top;
    top.clear();
    for (int r = 0; r < R; ++r) {
        const int32_t* c = cand + ((int64_t)r * n + q0 + f) * K * 3;
        TopK<KP> o;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            int64_t i = -1;
            float s = TOPK_EMPTY_S;
            if (j < K) {
                i = (int64_t)(((uint64_t)(uint32_t)c[j * 3 + 2] << 32) | (uint32_t)c[j * 3 + 1]);
                s = __int_as_float(c[j * 3]);
            }
            o.i[j] = i < 0 ? -1 : i;
            o.s[j] = i < 0 ? TOPK_EMPTY_S : s;
        }
        top.merge(o);
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        if (j < K) {
            const bool has = top.i[j] >= 0;
            out_idx[(int64_t)f * K + j] = has ? top.i[j] : -1;
            out_score[(int64_t)f * K + j] = has ? top.s[j] : -1.0f;
        }
    }
}

static int topk_kp(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }

static size_t topk_score_bytes(int F, int64_t N, int K) {
    const size_t lists = (size_t)scan_blocks(N) * (size_t)(F > 0 ? F : 1) * (size_t)(K > 0 ? K : 1);
    return (lists * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" size_t fr_gallery_topk_workspace(int F, int64_t N, int K) {
    const size_t lists = (size_t)scan_blocks(N) * (size_t)(F > 0 ? F : 1) * (size_t)(K > 0 ? K : 1);
    return topk_score_bytes(F, N, K) + lists * sizeof(int64_t) + 256;
}

template <int KP>
static int gallery_topk_launch_kp(const float* Q, const float* G, const int64_t* view, int F, int64_t N, int K,
                                  int64_t row_offset, int64_t* out_idx, float* out_score, float* ws_score,
                                  int64_t* ws_idx, const int32_t* seg_counts, int seg_len, hipStream_t s) {
    const int nblk = scan_blocks(N);
    dim3 grid(nblk, (F + QG - 1) / QG);
    if (view) gallery_scan_topk_f32<true, KP><<<grid, 256, 0, s>>>(Q, G, view, F, N, K, ws_score, ws_idx, seg_counts, seg_len);
    else gallery_scan_topk_f32<false, KP><<<grid, 256, 0, s>>>(Q, G, nullptr, F, N, K, ws_score, ws_idx, seg_counts, seg_len);
    FR_CHECK_LAUNCH("gallery_scan_topk_f32");
    gallery_topk_reduce<KP><<<fr_cdiv(F, 4), 256, 0, s>>>(ws_score, ws_idx, nblk, F, K, row_offset, out_idx, out_score,
                                                         seg_counts, seg_len);
    FR_CHECK_LAUNCH("gallery_topk_reduce");
    return FR_OK;
}

static int gallery_topk_launch(const char* who, const float* Q, const float* G, const int64_t* view, int F, int64_t N,
                               int D, int K, int64_t row_offset, int64_t* out_idx, float* out_score, void* workspace,
                               size_t workspace_bytes, const int32_t* seg_counts, int seg_len, fr_stream_t stream) {
    FR_REQUIRE(K >= 1 && K <= FR_TOPK_MAX, "%s: K must be 1..%d (got %d)", who, FR_TOPK_MAX, K);
    FR_REQUIRE(!seg_counts || (seg_len > 0 && F % seg_len == 0), "%s: seg_len must divide F", who);
    FR_REQUIRE(D == GD, "%s: D must be %d (got %d)", who, GD, D);
    FR_REQUIRE(F >= 0 && N >= 0, "%s: negative size", who);
    if (F == 0) return FR_OK;
    FR_REQUIRE(Q && out_idx && out_score && (G || N == 0), "%s: null pointer", who);
    FR_REQUIRE(workspace && workspace_bytes >= fr_gallery_topk_workspace(F, N, K),
               "%s: workspace too small (%zu < %zu)", who, workspace_bytes, fr_gallery_topk_workspace(F, N, K));
    float* ws_score = reinterpret_cast<float*>(workspace);
    int64_t* ws_idx = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(workspace) + topk_score_bytes(F, N, K));
    hipStream_t s = fr_stream(stream);
    switch (topk_kp(K)) {
        case 2: return gallery_topk_launch_kp<2>(Q, G, view, F, N, K, row_offset, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        case 4: return gallery_topk_launch_kp<4>(Q, G, view, F, N, K, row_offset, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        case 8: return gallery_topk_launch_kp<8>(Q, G, view, F, N, K, row_offset, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        default: return gallery_topk_launch_kp<16>(Q, G, view, F, N, K, row_offset, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
    }
}

extern "C" int fr_gallery_topk_f32(const float* Q, const float* G, int F, int64_t N, int D, int K, int64_t row_offset,
                                   int64_t* out_idx, float* out_score, void* workspace, size_t workspace_bytes,
                                   const int32_t* seg_counts, int seg_len, fr_stream_t stream) {
    return gallery_topk_launch("fr_gallery_topk_f32", Q, G, nullptr, F, N, D, K, row_offset, out_idx, out_score,
                               workspace, workspace_bytes, seg_counts, seg_len, stream);
}

extern "C" int fr_gallery_topk_view_f32(const float* Q, const float* G, const int64_t* view, int F, int64_t Nview,
                                        int D, int K, int64_t* out_idx, float* out_score, void* workspace,
                                        size_t workspace_bytes, fr_stream_t stream) {
    FR_REQUIRE(view || Nview == 0, "fr_gallery_topk_view_f32: null view");
    // Nview == 0: the scan kernel sees no tiles and the reduce writes (-1, -1.0) everywhere
    return gallery_topk_launch("fr_gallery_topk_view_f32", Q, G, Nview ? view : nullptr, F, Nview, D, K, 0, out_idx,
                               out_score, workspace, workspace_bytes, nullptr, 0, stream);
}

extern "C" size_t fr_gallery_topk_grouped_workspace(int ngroups, int64_t max_view_len, int K) {
    return fr_gallery_topk_workspace((ngroups > 0 ? ngroups : 0) * QG, max_view_len, K);
}

template <int KP>
static int gallery_topk_grouped_launch_kp(const float* Q, const float* G, const int64_t* views, const int64_t* gtab,
                                          const int32_t* qmap, int F, int ngroups, int nblk, int K,
                                          int64_t* out_idx, float* out_score, float* ws_score, int64_t* ws_idx,
                                          const int32_t* seg_counts, int seg_len, hipStream_t s) {
    gallery_scan_topk_grouped_f32<KP><<<dim3(nblk, ngroups), 256, 0, s>>>(Q, G, views, gtab, qmap, F, K, ws_score,
                                                                           ws_idx, seg_counts, seg_len);
    FR_CHECK_LAUNCH("gallery_scan_topk_grouped_f32");
    gallery_topk_reduce_grouped<KP><<<fr_cdiv(ngroups * QG, 4), 256, 0, s>>>(ws_score, ws_idx, nblk, ngroups, gtab, qmap, F, K,
                                                                              out_idx, out_score, seg_counts, seg_len);
    FR_CHECK_LAUNCH("gallery_topk_reduce_grouped");
    return FR_OK;
}

// Grouped view top-K: each query through ITS OWN view (fr_gallery_match_grouped_f32's tables, match.hip).
extern "C" int fr_gallery_topk_grouped_f32(const float* Q, const float* G, const int64_t* views, const int64_t* gtab,
                                           const int32_t* qmap, int F, int ngroups, int64_t max_view_len,
                                           int64_t capacity, int D, int K, int64_t* out_idx, float* out_score,
                                           void* workspace, size_t workspace_bytes, const int32_t* seg_counts,
                                           int seg_len, fr_stream_t stream) {
    const char* who = "fr_gallery_topk_grouped_f32";
    FR_REQUIRE(K >= 1 && K <= FR_TOPK_MAX, "%s: K must be 1..%d (got %d)", who, FR_TOPK_MAX, K);
    bool empty;
    const int rc = grouped_args_check(who, Q, G, views, gtab, qmap, F, ngroups, max_view_len, capacity, D, out_idx,
                                      out_score, workspace, workspace_bytes,
                                      fr_gallery_topk_grouped_workspace(ngroups, max_view_len, K), seg_counts, seg_len,
                                      &empty);
    if (rc != FR_OK || empty) return rc;
    const int nblk = scan_blocks(max_view_len);
    float* ws_score = reinterpret_cast<float*>(workspace);
    int64_t* ws_idx = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(workspace) +
                                                 topk_score_bytes(ngroups * QG, max_view_len, K));
    hipStream_t s = fr_stream(stream);
    switch (topk_kp(K)) {
        case 2: return gallery_topk_grouped_launch_kp<2>(Q, G, views, gtab, qmap, F, ngroups, nblk, K, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        case 4: return gallery_topk_grouped_launch_kp<4>(Q, G, views, gtab, qmap, F, ngroups, nblk, K, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        case 8: return gallery_topk_grouped_launch_kp<8>(Q, G, views, gtab, qmap, F, ngroups, nblk, K, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
        default: return gallery_topk_grouped_launch_kp<16>(Q, G, views, gtab, qmap, F, ngroups, nblk, K, out_idx, out_score, ws_score, ws_idx, seg_counts, seg_len, s);
    }
}

// fr_gallery_topk_view_f32 for the queries a mask names: query f is scanned iff mask[f] > 0 (the padding rule of the
// contiguous entry with seg_len = 1), every other query costs no scan work and reports (-1, -1.0).  The exact fallback
// of the certified coarse top-K (scan_gemm.hip) runs this with the re-rank's flags as the mask.
extern "C" int fr_gallery_topk_view_masked_f32(const float* Q, const float* G, const int64_t* view, int F, int64_t Nview,
                                               int D, int K, int64_t* out_idx, float* out_score, void* workspace,
                                               size_t workspace_bytes, const int32_t* mask, fr_stream_t stream) {
    FR_REQUIRE(view || Nview == 0, "fr_gallery_topk_view_masked_f32: null view");
    return gallery_topk_launch("fr_gallery_topk_view_masked_f32", Q, G, Nview ? view : nullptr, F, Nview, D, K, 0, out_idx,
                               out_score, workspace, workspace_bytes, mask, mask ? 1 : 0, stream);
}

extern "C" int fr_match_reduce_shards_topk(const int32_t* cand, int R, int n, int K, int q0, int F, int64_t* out_idx,
                                           float* out_score, fr_stream_t stream) {
    FR_REQUIRE(K >= 1 && K <= FR_TOPK_MAX, "fr_match_reduce_shards_topk: K must be 1..%d (got %d)", FR_TOPK_MAX, K);
    FR_REQUIRE(R >= 1 && n >= 0 && q0 >= 0 && F >= 0 && q0 + F <= n,
               "fr_match_reduce_shards_topk: bad range (R %d n %d q0 %d F %d)", R, n, q0, F);
    if (F == 0) return FR_OK;
    FR_REQUIRE(cand && out_idx && out_score, "fr_match_reduce_shards_topk: null pointer");
    hipStream_t s = fr_stream(stream);
    const int blocks = fr_cdiv(F, 64);
    switch (topk_kp(K)) {
        case 2: match_reduce_shards_topk<2><<<blocks, 64, 0, s>>>(cand, R, n, K, q0, F, out_idx, out_score); break;
        case 4: match_reduce_shards_topk<4><<<blocks, 64, 0, s>>>(cand, R, n, K, q0, F, out_idx, out_score); break;
        case 8: match_reduce_shards_topk<8><<<blocks, 64, 0, s>>>(cand, R, n, K, q0, F, out_idx, out_score); break;
        default: match_reduce_shards_topk<16><<<blocks, 64, 0, s>>>(cand, R, n, K, q0, F, out_idx, out_score); break;
    }
    FR_CHECK_LAUNCH("match_reduce_shards_topk");
    return FR_OK;
}
