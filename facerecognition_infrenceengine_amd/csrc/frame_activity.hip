// Activity gate: which frames of a camera batch show something that the last PROCESSED frame of the same camera did not, so the
// engine pass can skip the others (the reference sheds load blindly: /root/reference/peopleCount.py:938,962 takes every 2nd
// frame, /root/reference/infrenceServer.py:595-598,614-617 drop frames when a queue is full).
//
// Arithmetic (include/frhip.h fr_frame_activity_u8; tests/helpers/activity_ref.py is the definition), all in
// 32-bit integers:
//     L = (29 B + 150 G + 77 R + 128) >> 8          per pixel of a BGR u8 frame (the weights sum to 256: L is 0 .. 255)
//     m = (sum of L over a 16 x 16 cell + 128) >> 8  per cell, gh = H / 16 rows of gw = W / 16 cells; remainder rows and
//                                                    columns belong to no cell
// and, per frame f with slot s = slot[f] and cur = its cell means,
//     changed = -1 if geom[s] != (H, W), else the number of cells with |cur - grid[s]| > thr
//     active  = changed < 0 or changed >= min_cells or (max_idle > 0 and idle[s] >= max_idle)
//     active: grid[s] = cur, geom[s] = (H, W), idle[s] = 0;   otherwise idle[s] += 1 and nothing else moves.
//
// Two launches, no atomics, no host synchronisation:
//  1. activity_means*: memory-bound, no LDS, no barrier.  A wave owns a block of 16 rows x 4 cells: lane = 4 * row + cell, so the
//     four lanes of a row read 192 contiguous bytes as 3 x 16 bytes each and the wave's 16 rows are reduced with four xor
//     shuffles.  The four waves of a workgroup take neighbouring blocks of one 16-row band and walk the band 16 cells at a
//     time; every byte of a frame's cell area is read once.  The loads are declared with byte alignment: a row starts on 16
//     bytes only when 3 W is a multiple of 16 (and the frame does), and nothing past a cell row's 48 bytes is read.
//  2. activity_judge: one workgroup per frame.  It counts the changed cells 16 at a time (wave reduce, then LDS), and - behind
//     the barrier that ends every read of grid[s], geom[s] and idle[s] - copies cur to grid[s] when the frame is active and
//     writes the slot's state, so the verdicts do not depend on how many frames share a launch.
#include "common.h"
#include <algorithm>

namespace {

typedef int4v int4v_u __attribute__((aligned(1)));              // 16-byte access at any byte address

constexpr int AC = 16;                                          // cell side in pixels

// A frame the rule is defined for: at least one cell, its cells fit a row of the cell arrays, below 2 GiB, memory behind it.
__device__ __forceinline__ bool judged(const uint8_t* data, int H, int W, int C) {
    return data && H >= AC && W >= AC && (int64_t)H * W * 3 < (1ll << 31) && (int64_t)(H / AC) * (W / AC) <= C;
}

// sum of the luma of the 16 pixels held in 48 bytes
__device__ __forceinline__ int luma16(const int4v a, const int4v b, const int4v c) {
    const unsigned d[12] = {(unsigned)a[0], (unsigned)a[1], (unsigned)a[2], (unsigned)a[3], (unsigned)b[0], (unsigned)b[1],
                            (unsigned)b[2], (unsigned)b[3], (unsigned)c[0], (unsigned)c[1], (unsigned)c[2], (unsigned)c[3]};
    int sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {                               // 4 pixels in 3 dwords: BGRB GRBG RBGR
        const unsigned w0 = d[3 * q], w1 = d[3 * q + 1], w2 = d[3 * q + 2];
        const unsigned B[4] = {w0 & 0xffu, w0 >> 24, (w1 >> 16) & 0xffu, (w2 >> 8) & 0xffu};
        const unsigned G[4] = {(w0 >> 8) & 0xffu, w1 & 0xffu, w1 >> 24, (w2 >> 16) & 0xffu};
        const unsigned R[4] = {(w0 >> 16) & 0xffu, (w1 >> 8) & 0xffu, w2 & 0xffu, w2 >> 24};
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += (int)((29u * B[j] + 150u * G[j] + 77u * R[j] + 128u) >> 8);
    }
    return sum;
}

// Bands first, first + stride, ... of ONE judged frame: cur[cell] for their cells.  Only the frame's cell area is read.
__device__ __forceinline__ void band_means(const uint8_t* __restrict__ data, int H, int W, uint8_t* __restrict__ cur, int first,
                                           int stride) {
    const int gh = H / AC, gw = W / AC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = lane >> 2, sub = lane & 3;
    for (int band = first; band < gh; band += stride) {
        const uint8_t* __restrict__ line = data + (band * AC + row) * W * 3;      // < H W 3 < 2^31
        for (int c0 = 0; c0 < gw; c0 += 16) {                   // wave-uniform trip count: the shuffles see all 64 lanes
            const int cell = c0 + wave * 4 + sub;
            int sum = 0;
            if (cell < gw) {
                const uint8_t* p = line + cell * (AC * 3);
                sum = luma16(*reinterpret_cast<const int4v_u*>(p), *reinterpret_cast<const int4v_u*>(p + 16),
                             *reinterpret_cast<const int4v_u*>(p + 32));
            }
#pragma unroll
            for (int o = 4; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);       // over the 16 rows: lanes with one `sub`
            if (row == 0 && cell < gw) cur[band * gw + cell] = (uint8_t)((sum + 128) >> 8);
        }
    }
}

// uniform batch: workgroup (band, frame)
__global__ __launch_bounds__(256) void activity_means_u8(const uint8_t* __restrict__ frames, int H, int W, int C,
                                                         uint8_t* __restrict__ cur) {
    const int f = blockIdx.y;
    const uint8_t* data = frames + (int64_t)f * H * W * 3;
    if (!judged(data, H, W, C)) return;
    band_means(data, H, W, cur + (int64_t)f * C, blockIdx.x, gridDim.x);
}

// frame table: blockIdx.y is the frame, its gridDim.x workgroups walk its bands (the sizes live on the device)
__global__ __launch_bounds__(256) void activity_means_refs_u8(const fr_frame_ref* __restrict__ refs, int C, uint8_t* __restrict__ cur) {
    const fr_frame_ref r = refs[blockIdx.y];
    if (!judged(r.data, r.H, r.W, C)) return;
    band_means(r.data, r.H, r.W, cur + (int64_t)blockIdx.y * C, blockIdx.x, gridDim.x);
}

struct Rule { int thr, min_cells, max_idle; };

// number of bytes among 16 with |a - b| > thr
__device__ __forceinline__ int changed16(const int4v a, const int4v b, int thr) {
    int n = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned x = (unsigned)a[q], y = (unsigned)b[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = (int)((x >> (8 * j)) & 0xffu) - (int)((y >> (8 * j)) & 0xffu);
            n += (d < 0 ? -d : d) > thr ? 1 : 0;
        }
    }
    return n;
}

// One workgroup per frame.  refs == nullptr: every frame is H x W (the uniform entry; the frames' memory is not needed here).
__global__ __launch_bounds__(256) void activity_judge(const fr_frame_ref* __restrict__ refs, const uint8_t* frames, int H, int W,
                                                      const int32_t* __restrict__ slot, int S, uint8_t* grid, int32_t* geom,
                                                      int32_t* idle, int C, const uint8_t* __restrict__ cur_all,
                                                      int32_t* __restrict__ changed_out, int32_t* __restrict__ active_out, Rule k) {
    __shared__ int part[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const uint8_t* data = frames;
    if (refs) {
        const fr_frame_ref r = refs[f];
        data = r.data; H = r.H; W = r.W;
    }
    const int s = slot[f];
    if (!judged(data, H, W, C) || s < 0 || s >= S) {            // block-uniform: always active, no state is read or written
        if (tid == 0) {
            changed_out[f] = -1;
            active_out[f] = 1;
        }
        return;
    }
    const int cells = (H / AC) * (W / AC), full = cells >> 4;
    const uint8_t* __restrict__ cur = cur_all + (int64_t)f * C;
    uint8_t* g = grid + (int64_t)s * C;
    const bool same = geom[2 * s] == H && geom[2 * s + 1] == W;
    const int was_idle = idle[s];
    int n = 0;
    if (same) {
        for (int i = tid; i < full; i += 256)
            n += changed16(*reinterpret_cast<const int4v_u*>(cur + 16 * i), *reinterpret_cast<const int4v_u*>(g + 16 * i), k.thr);
        for (int i = 16 * full + tid; i < cells; i += 256) {
            const int d = (int)cur[i] - (int)g[i];
            n += (d < 0 ? -d : d) > k.thr ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = n;
    __syncthreads();                                            // every read of grid[s], geom[s] and idle[s] lies before this
    const int changed = same ? part[0] + part[1] + part[2] + part[3] : -1;
    const bool active = changed < 0 || changed >= k.min_cells || (k.max_idle > 0 && was_idle >= k.max_idle);
    if (active) {
        for (int i = tid; i < full; i += 256)
            *reinterpret_cast<int4v_u*>(g + 16 * i) = *reinterpret_cast<const int4v_u*>(cur + 16 * i);
        for (int i = 16 * full + tid; i < cells; i += 256) g[i] = cur[i];
    }
    if (tid == 0) {
        changed_out[f] = changed;
        active_out[f] = active ? 1 : 0;
        if (active) {
            geom[2 * s] = H;
            geom[2 * s + 1] = W;
            idle[s] = 0;
        } else {
            idle[s] = was_idle + 1;
        }
    }
}

// the checks both entries share
int activity_check(const char* who, int n, int S, int C, int thr, int min_cells, int max_idle) {
    FR_REQUIRE(n >= 0 && n <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(S > 0 && C > 0, "%s: bad state size (S slots and C cells per slot, both positive)", who);
    FR_REQUIRE(thr >= 0 && thr <= 255, "%s: thr %d outside 0 .. 255", who, thr);
    FR_REQUIRE(min_cells >= 1, "%s: min_cells %d below 1", who, min_cells);
    FR_REQUIRE(max_idle >= 0, "%s: max_idle %d below 0 (0 switches the refresh off)", who, max_idle);
    return FR_OK;
}

}  // namespace

extern "C" int fr_frame_activity_u8(const uint8_t* frames, int N, int H, int W, const int32_t* slot, int S, uint8_t* grid,
                                    int32_t* geom, int32_t* idle, int C, uint8_t* cur, int32_t* changed, int32_t* active, int thr,
                                    int min_cells, int max_idle, fr_stream_t stream) {
    if (const int rc = activity_check("fr_frame_activity_u8", N, S, C, thr, min_cells, max_idle)) return rc;
    FR_REQUIRE(H > 0 && W > 0, "fr_frame_activity_u8: bad frame size %d x %d (H and W positive)", H, W);
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "fr_frame_activity_u8: a %d x %d frame is beyond 2 GiB", H, W);
    if (N == 0) return FR_OK;
    FR_REQUIRE(frames && slot && grid && geom && idle && cur && changed && active, "fr_frame_activity_u8: null pointer");
    const int gh = H / AC;
    if (gh > 0 && W >= AC) {                                    // a frame without a cell: the judge alone (always active)
        activity_means_u8<<<dim3((unsigned)gh, (unsigned)N), 256, 0, fr_stream(stream)>>>(frames, H, W, C, cur);
        FR_CHECK_LAUNCH("activity_means_u8");
    }
    activity_judge<<<(unsigned)N, 256, 0, fr_stream(stream)>>>(nullptr, frames, H, W, slot, S, grid, geom, idle, C, cur, changed,
                                                               active, Rule{thr, min_cells, max_idle});
    FR_CHECK_LAUNCH("activity_judge");
    return FR_OK;
}

extern "C" int fr_frame_activity_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* slot, int S, uint8_t* grid,
                                         int32_t* geom, int32_t* idle, int C, uint8_t* cur, int32_t* changed, int32_t* active,
                                         int thr, int min_cells, int max_idle, fr_stream_t stream) {
    if (const int rc = activity_check("fr_frame_activity_refs_u8", nframes, S, C, thr, min_cells, max_idle)) return rc;
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(refs && slot && grid && geom && idle && cur && changed && active, "fr_frame_activity_refs_u8: null pointer");
    // about 8192 workgroups in all, 8 .. 256 per frame (a workgroup past the frame's last band ends at once): a 1080p frame has
    // 67 bands, so 64 of them get a workgroup per band
    const int per = std::min(256, std::max(8, (8192 + nframes - 1) / nframes));
    activity_means_refs_u8<<<dim3((unsigned)per, (unsigned)nframes), 256, 0, fr_stream(stream)>>>(refs, C, cur);
    FR_CHECK_LAUNCH("activity_means_refs_u8");
    activity_judge<<<(unsigned)nframes, 256, 0, fr_stream(stream)>>>(refs, nullptr, 0, 0, slot, S, grid, geom, idle, C, cur, changed,
                                                                     active, Rule{thr, min_cells, max_idle});
    FR_CHECK_LAUNCH("activity_judge");
    return FR_OK;
}
