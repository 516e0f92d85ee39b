// Gallery audit: every pair of positions a < b of a view whose rows the duplicate check would refuse,
//     s(a, b) = row_dot_wave8(G32[view[a]], G32[view[b]])  >  thr   (inclusive: >=),
// s being the dot of gallery_first_above (match.hip) on the rows as stored - in ONE pass over the pairs instead of one
// first-hit scan per row.  The matrix cores only FILTER; the f32 VALU dot of the duplicate check alone decides.
//
//   pair_gather_f16   X16[p] = f16(G32[view[p]]) (the conversion of fr_f32_to_f16) into the workspace: the self-join's two
//                     operands, contiguous, whatever coarse slab the gallery keeps or does not keep.
//   pair_scan_f16     the coarse scan of scan_gemm.hip turned on itself: a block keeps 256 positions of X16 stationary as
//                     MFMA B fragments (read as f16, no conversion) and streams a range of X16 rows through two LDS-DMA
//                     tile buffers, one barrier per tile.  Grid = query tiles x row ranges; a block whose range ends at or
//                     before its first query has no pair b > a and returns at once (about half the grid), and a block
//                     starts at the tile that holds its first query + 1.  Per (tile, query) the common path is the max
//                     tree over the lane's 16 scores and one compare against t_lo = thr - eps; a score >= t_lo with
//                     a < b < N appends the key a << 32 | b to the candidate buffer (slot from an atomicAdd on a counter
//                     that keeps counting past the capacity, so the host learns what would have sufficed).
//                     eps = PS_EPS_C 2^-10 Gmax^2 + PS_EPS_ABS 2 Gmax + 2^-40 bounds |coarse - s| for every pair of the
//                     view (DESIGN.md 4.6b with |q| <= Gmax; 4.6f for the wave dot): no pair that passes is filtered out.
//   pair_recheck      one wave per candidate: row_dot_lane8 + wave_sum on the f32 rows through the view, the threshold
//                     test, (key, score) appended through a second counter.  A launch of its own: nothing reads within a
//                     launch what another workgroup of that launch wrote.
#include "match_scan.h"

#define PS_ROWS 64            // X16 rows per LDS tile (SG_ROWS of scan_gemm.hip)
#define PS_QB 256             // stationary positions per block: 8 waves x 32
#define PS_RB 1024            // bytes of an f16 row
#define PS_TILE_B (PS_ROWS * PS_RB)
#define PS_NPIECE 8           // LDS-DMA instructions per wave per tile
#define PS_MAX_TPR 16384      // tiles per range: the range's buffer stays below 2^31 bytes
#define PS_EPS_C 1.125f       // FR_CERT_C / FR_CERT_ABS of scan_gemm.hip: the same bound
#define PS_EPS_ABS 0x1p-20f

struct PairP {
    const half_t* X; int64_t N;
    int nqt, nranges; int64_t rows_per_range;          // rows_per_range: multiple of PS_ROWS
    float thr; const float* gmax;
    unsigned long long* keys; int64_t capacity; int* counter;
};

// thr - eps from the device Gmax: the same operations in every thread of the launch
__device__ __forceinline__ float pair_t_lo(float thr, float gm) {
    const float eps = PS_EPS_C * 0x1p-10f * gm * gm + PS_EPS_ABS * (gm + gm) + 0x1p-40f;
    return thr - eps;
}

__global__ void pair_gather_f16(const float* __restrict__ G, const int64_t* __restrict__ view, int64_t N,
                                half_t* __restrict__ X) {
    const int64_t n4 = N * (GD / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i / (GD / 4);
        const int c = (int)(i % (GD / 4)) * 4;
        const float4 v = *reinterpret_cast<const float4*>(G + (view ? view[p] : p) * GD + c);
        const half4 o = {(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
        *reinterpret_cast<half4*>(X + p * GD + c) = o;
    }
}

__global__ __launch_bounds__(512, 2) void pair_scan_f16(PairP p) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int NKC = PS_RB / 128;                   // 128-B chunks per row
    extern __shared__ __attribute__((aligned(16))) char lds[];      // [2][NKC][64 rows][128 B]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fq = lane >> 4;
    // blocks that scan the same row range for different query tiles share an XCD (scan_gemm.hip).  Speed only.
    const int b = blockIdx.x, xcd = b & 7, g = b >> 3;
    const int qt = g % p.nqt;
    const int rr = (g / p.nqt) * 8 + xcd;
    if (rr >= p.nranges) return;
    const int64_t q0b = (int64_t)qt * PS_QB;
    const int64_t r0 = (int64_t)rr * p.rows_per_range;
    const int64_t r1 = min(p.N, r0 + p.rows_per_range);
    if (r1 <= q0b + 1) return;                         // no row of the range lies above the tile's first position
    const float gm = p.gmax[0];
    if (!(gm < INFINITY)) return;                      // a row the f16 copy cannot hold (or NaN): the host refuses the view
    const float t_lo = pair_t_lo(p.thr, gm);
    const int nrows = (int)(r1 - r0);
    const int ntiles = (nrows + PS_ROWS - 1) / PS_ROWS;
    const int t0 = q0b + 1 > r0 ? (int)((q0b + 1 - r0) / PS_ROWS) : 0;      // the tile of row q0b + 1: earlier rows pair with nothing here
    const int64_t q0w = q0b + wave * 32;

    // ---- stationary B operand: this wave's 32 positions, whole K, as stored
    int4v blo[2][NKC], bhi[2][NKC];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int64_t q = q0w + n * 16 + fr;
        const bool ok = q < p.N;
        const half_t* qp = p.X + (ok ? q : 0) * GD;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            blo[n][kc] = *reinterpret_cast<const int4v*>(qp + kc * 64 + fq * 8);
            bhi[n][kc] = *reinterpret_cast<const int4v*>(qp + kc * 64 + 32 + fq * 8);
            if (!ok) { blo[n][kc] = int4v{0, 0, 0, 0}; bhi[n][kc] = int4v{0, 0, 0, 0}; }
        }
    }

    // ---- row stream: wave w fills pieces w*8 + i of a tile; piece = (kc, 8-row group); rows past the range read 0
    __amdgpu_buffer_rsrc_t grs = buffer_rsrc(reinterpret_cast<const char*>(p.X) + r0 * PS_RB, (unsigned)((int64_t)nrows * PS_RB));
    unsigned voff[PS_NPIECE], ldst[PS_NPIECE];
#pragma unroll
    for (int i = 0; i < PS_NPIECE; ++i) {
        const int pc = wave * PS_NPIECE + i, kc = pc >> 3, rg = pc & 7;
        const int row = rg * 8 + (lane >> 3);
        voff[i] = (unsigned)(row * PS_RB) + (unsigned)(kc * 128 + (((lane & 7) ^ (row & 7)) << 4));
        ldst[i] = (unsigned)((kc * PS_ROWS + rg * 8) * 128);
    }
    auto issue_tile = [&](int t) {
        char* dst = lds + (t & 1) * PS_TILE_B;
#pragma unroll
        for (int i = 0; i < PS_NPIECE; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(grs, (lds_ptr_t)(dst + ldst[i]), 16, voff[i] + (unsigned)t * PS_TILE_B, 0, 0, 0);
    };

    const int key = fr & 7;
    const unsigned a_lo = (unsigned)(fr * 128 + ((fq ^ key) << 4)), a_hi = (unsigned)(fr * 128 + (((4 + fq) ^ key) << 4));

    issue_tile(t0);
    for (int t = t0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this wave's pieces of tile t have landed
        __builtin_amdgcn_s_barrier();                               // everyone's have; buffer (t+1)&1 is free again
        if (t + 1 < ntiles) issue_tile(t + 1);
        const char* buf = lds + (t & 1) * PS_TILE_B;
        float4v acc[4][2];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = float4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            int4v alo[4], ahi[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const char* rowp = buf + (kc * PS_ROWS + m * 16) * 128;
                alo[m] = *reinterpret_cast<const int4v*>(rowp + a_lo);
                ahi[m] = *reinterpret_cast<const int4v*>(rowp + a_hi);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    acc[m][n] = mfma16(alo[m], blo[n][kc], acc[m][n]);
                    acc[m][n] = mfma16(ahi[m], bhi[n][kc], acc[m][n]);
                }
        }
        // acc[m][n][reg] = coarse score of row r0 + t*64 + m*16 + 4*fq + reg against position q0w + n*16 + fr
        const int64_t rbase = r0 + t * PS_ROWS + 4 * fq;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            float gmx[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) gmx[m] = fmaxf(fmaxf(acc[m][n][0], acc[m][n][1]), fmaxf(acc[m][n][2], acc[m][n][3]));
            const float mx = fmaxf(fmaxf(gmx[0], gmx[1]), fmaxf(gmx[2], gmx[3]));
            if (mx >= t_lo) {                                        // rare: a candidate, the diagonal, or a zero row past the end
                const int64_t a = q0w + n * 16 + fr;
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int64_t bb = rbase + m * 16 + reg;
                        if (acc[m][n][reg] >= t_lo && bb > a && bb < p.N) {
                            const int64_t slot = (int64_t)(unsigned)atomicAdd(p.counter, 1);
                            if (slot < p.capacity) p.keys[slot] = ((unsigned long long)a << 32) | (unsigned long long)bb;
                        }
                    }
            }
        }
    }
#endif
}

// out_counts: [0] candidates seen (pair_scan_f16's counter), [1] pairs (this kernel's), [2] flags, [3] row ranges used
__global__ __launch_bounds__(256) void pair_recheck(const float* __restrict__ G, const int64_t* __restrict__ view,
                                                    const unsigned long long* __restrict__ keys, int64_t capacity,
                                                    const float* __restrict__ gmax, float thr, int inclusive, int nranges,
                                                    int64_t* __restrict__ out_key, float* __restrict__ out_score,
                                                    int32_t* out_counts) {
    const int lane = threadIdx.x & 63;
    const int64_t seen = (int64_t)(unsigned)out_counts[0];          // written by the launch before this one
    const int64_t n = seen < capacity ? seen : capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_counts[2] = (seen > capacity ? FR_PAIRS_OVERFLOW : 0) | (gmax[0] < INFINITY ? 0 : FR_PAIRS_NONFINITE);
        out_counts[3] = nranges;
    }
    for (int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += (int64_t)gridDim.x * 4) {
        const unsigned long long k = keys[c];
        const int64_t a = (int64_t)(k >> 32), b = (int64_t)(k & 0xffffffffull);
        const float4* qa = reinterpret_cast<const float4*>(G + (view ? view[a] : a) * GD + lane * 8);
        const float4* gb = reinterpret_cast<const float4*>(G + (view ? view[b] : b) * GD + lane * 8);
        const float4 q0 = qa[0], q1 = qa[1];
        const float qv[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        const float s = row_dot_wave8(qv, gb[0], gb[1]);
        if (lane == 0 && (inclusive ? (s >= thr) : (s > thr))) {
            const int slot = atomicAdd(out_counts + 1, 1);           // < n <= capacity
            out_key[slot] = (int64_t)k;
            out_score[slot] = s;
        }
    }
}

// ---------------------------------------------------------------- host side
struct PairPlan { int nqt, nranges; int64_t rows_per_range; int64_t grid; };

// About 1024 working blocks (half of nqt x nranges), at most 32 tiles a block so that the blocks along the diagonal, which do
// part of a range, do not leave the others waiting; max_ranges > 0 bounds the number of ranges instead.
static PairPlan pair_plan(int64_t N, int max_ranges) {
    PairPlan pl;
    pl.nqt = (int)((N + PS_QB - 1) / PS_QB);
    if (pl.nqt < 1) pl.nqt = 1;
    int64_t tiles = (N + PS_ROWS - 1) / PS_ROWS;
    if (tiles < 1) tiles = 1;
    int64_t want = 2048 / pl.nqt;
    if (want < 8) want = 8;
    if (want > tiles) want = tiles;
    int64_t tpr = (tiles + want - 1) / want;
    if (tpr > 32) tpr = 32;
    if (max_ranges > 0 && (tiles + tpr - 1) / tpr > max_ranges) tpr = (tiles + max_ranges - 1) / max_ranges;
    if (tpr > PS_MAX_TPR) tpr = PS_MAX_TPR;            // the buffer bound outranks max_ranges
    pl.nranges = (int)((tiles + tpr - 1) / tpr);
    pl.rows_per_range = tpr * PS_ROWS;
    pl.grid = (int64_t)((pl.nranges + 7) / 8) * 8 * pl.nqt;
    return pl;
}

static size_t ps_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace: Gmax (256 bytes) | candidate keys [capacity] | X16 [N][512]
extern "C" size_t fr_gallery_pairs_workspace(int64_t N, int64_t capacity) {
    const size_t n = N > 0 ? (size_t)N : 0, c = capacity > 0 ? (size_t)capacity : 0;
    return 256 + ps_up256(c * 8) + n * PS_RB;
}

extern "C" int fr_gallery_pairs_above_f16(const float* G32, const int64_t* view, int64_t N, int D, float thr, int inclusive,
                                          int64_t capacity, int max_ranges, int64_t* out_key, float* out_score,
                                          int32_t* out_counts, void* workspace, size_t workspace_bytes, fr_stream_t stream) {
    const char* who = "fr_gallery_pairs_above_f16";
    FR_REQUIRE(D == GD, "%s: D must be %d (got %d)", who, GD, D);
    FR_REQUIRE(N >= 0 && N < (1ll << 31), "%s: N must be 0..2^31-1 (got %lld)", who, (long long)N);
    FR_REQUIRE(capacity >= 1 && capacity < (1ll << 31), "%s: capacity must be 1..2^31-1 (got %lld)", who, (long long)capacity);
    FR_REQUIRE(max_ranges >= 0, "%s: max_ranges must not be negative (got %d)", who, max_ranges);
    hipStream_t s = fr_stream(stream);
    if (N <= 1) {                                       // no pair: zero counts, no row is read
        if (out_counts && hipMemsetAsync(out_counts, 0, 4 * sizeof(int32_t), s) != hipSuccess) {
            fr_set_error("%s: memset failed", who);
            return FR_E_LAUNCH;
        }
        return FR_OK;
    }
    FR_REQUIRE(G32 && out_key && out_score && out_counts, "%s: null pointer", who);
    const size_t need = fr_gallery_pairs_workspace(N, capacity);
    FR_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", who, workspace_bytes, need);
    const PairPlan pl = pair_plan(N, max_ranges);
    FR_REQUIRE(pl.grid < (1ll << 31), "%s: grid too large", who);
    char* base = reinterpret_cast<char*>(workspace);
    float* gmax = reinterpret_cast<float*>(base);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + 256);
    half_t* X = reinterpret_cast<half_t*>(base + 256 + ps_up256((size_t)capacity * 8));
    if (hipMemsetAsync(gmax, 0, 256, s) != hipSuccess || hipMemsetAsync(out_counts, 0, 4 * sizeof(int32_t), s) != hipSuccess) {
        fr_set_error("%s: memset failed", who);
        return FR_E_LAUNCH;
    }
    const int rc = fr_gallery_gmax_update(G32, view, N, D, gmax, stream);
    if (rc != FR_OK) return rc;
    int64_t gb = (N * (GD / 4) + 255) / 256;
    if (gb > 8192) gb = 8192;
    pair_gather_f16<<<(int)gb, 256, 0, s>>>(G32, view, N, X);
    FR_CHECK_LAUNCH("pair_gather_f16");
    PairP p;
    p.X = X; p.N = N; p.nqt = pl.nqt; p.nranges = pl.nranges; p.rows_per_range = pl.rows_per_range;
    p.thr = thr; p.gmax = gmax; p.keys = keys; p.capacity = capacity; p.counter = out_counts;
    constexpr int lds = 2 * PS_TILE_B;
    static FrDevLatch latch;
    if (!fr_raise_lds(reinterpret_cast<const void*>(pair_scan_f16), lds, latch)) {
        fr_set_error("%s: cannot raise dynamic LDS", who);
        return FR_E_LAUNCH;
    }
    pair_scan_f16<<<(int)pl.grid, 512, lds, s>>>(p);
    FR_CHECK_LAUNCH("pair_scan_f16");
    int64_t rb = (capacity + 3) / 4;
    if (rb > 2048) rb = 2048;
    pair_recheck<<<(int)rb, 256, 0, s>>>(G32, view, keys, capacity, gmax, thr, inclusive, pl.nranges, out_key, out_score, out_counts);
    FR_CHECK_LAUNCH("pair_recheck");
    return FR_OK;
}
