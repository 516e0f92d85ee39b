// Face redaction of the live path: the regions of a frame's faces are pixelated (or filled) IN PLACE in the BGR frames where they
// already are - on the device, behind the engine pass, in front of the HUD draw and the JPEG encoder - so that no unmasked
// picture of a masked face ever leaves the device.
//
// The picture is DEFINED by tests/helpers/redact_ref.py (include/frhip.h fr_redact_u8), integers only:
//     cells    block x block, anchored at the picture's origin: pixel (x, y) lies in cell (x / block, y / block); the cells of the
//              last column and row are cut at W and H, so a cell has n = cw ch <= block^2 pixels
//     held     a pixel is held when at least one of the frame's regions (inclusive rectangles x1 y1 x2 y2) contains it
//     mode 0   a held pixel takes, per channel, (S + n / 2) / n with S the sum of the ORIGINAL bytes of its whole cell - the
//              cell's pixels outside every region included
//     mode 1   a held pixel takes the colour
// A pixel that is not held is never written.  The grid does not depend on the regions: regions that overlap, a region listed
// twice and any order of the list give the bytes of the union.
//
// Work is cut by CELL, never by region.  A tile is one strip of whole cells: `block` rows x TW = block * (64 / block) pixels
// (at most 192 bytes of a row); blockIdx.y is the frame and the gridDim.x blocks of a frame walk its tiles, as hud_draw.hip
// does.  A block loads its frame's regions into LDS once; a tile that no region meets is skipped without touching memory (the
// test reads LDS only and is block-uniform).
//
// IN PLACE, and why that is safe: the tiles of a frame are disjoint and each is made of whole cells, so a cell's mean needs no
// byte outside its tile.  A tile is owned by exactly one workgroup; that workgroup reads bytes of its own tile only - no
// workgroup reads a pixel that another may write.  Inside the workgroup every load of the tile has landed in a register sum and
// gone to LDS before the first __syncthreads() of the tile, the means are finished behind the third, and the stores of the tile
// come after it: the whole tile is read before any of it is stored, so a mean never sees a byte this launch wrote.  The stores
// write no byte the definition leaves alone, so the neighbouring tiles' owners read original bytes whenever they run.
//
// Mapping: a wave takes the rows w, w + 4, ... of the tile, and its lanes the bytes lane, lane + 64, lane + 128 of a row -
// consecutive lanes, consecutive bytes - summing their byte column over the wave's rows in registers.  The four waves' column
// sums meet in LDS, and one thread per (cell, channel) - channel = byte index mod 3 - adds the cell's cw columns and divides:
// one division per cell and channel, 32-bit integers throughout (S <= 4096 * 255).  For the stores a lane keeps, per byte
// column, the set of regions whose x range holds it (one 64-bit mask per column and tile); a row's set of regions whose y range
// holds it is wave-uniform, and a pixel is held when the two sets meet - one AND per byte, no rectangle test per pixel.
#include "common.h"
#include <algorithm>

namespace {

constexpr int RD_CAP = FR_REDACT_MAX_CAP;             // regions of a frame
constexpr int RD_LIMIT = 1 << 20;                     // coordinates are clamped to +-2^20
constexpr int RD_ROWB = 192;                          // bytes of a tile's row at most: 64 pixels
constexpr int RD_COLS = RD_ROWB / 64;                 // byte columns of a lane

struct RedactArgs {
    const int32_t* counts;
    const int32_t* regions;
    int cap, block, mode;
    uint32_t bgr;
};

// a value every lane holds alike, moved to scalar registers
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Tiles first, first + stride, ... of ONE frame of H x W at `data` (H, W positive, H*W*3 < 2^31: the callers see to it);
// f: its row of counts / regions.  Nothing outside [data, data + H*W*3) is touched.
__device__ __forceinline__ void redact_frame(uint8_t* __restrict__ data, int H, int W, int f, const RedactArgs a, int first, int stride) {
    __shared__ int R[RD_CAP * 4];
    __shared__ unsigned part[4][RD_ROWB];             // a wave's column sums
    __shared__ unsigned col[RD_ROWB];                 // the tile's column sums
    __shared__ unsigned mean[RD_ROWB];                // per (cell, channel) of the tile: at most 32 cells
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = a.block;
    const int n = min(max(a.counts[f], 0), a.cap);              // slots j >= counts[f] are never read
    if (n == 0) return;                                         // block-uniform
    if (tid < n * 4) R[tid] = min(max(a.regions[(int64_t)f * a.cap * 4 + tid], -RD_LIMIT), RD_LIMIT);
    __syncthreads();
    const int TW = B * (64 / B);
    const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + B - 1) / B);
    int px[RD_COLS], chn[RD_COLS], cell[RD_COLS];               // a lane's byte columns: pixel, channel and cell within the tile
#pragma unroll
    for (int k = 0; k < RD_COLS; ++k) {
        const int b = lane + 64 * k;
        px[k] = b / 3;
        chn[k] = b - 3 * px[k];
        cell[k] = px[k] / B;
    }
    unsigned fill[RD_COLS];                                     // mode 1: the colour's byte for each byte column
#pragma unroll
    for (int k = 0; k < RD_COLS; ++k) fill[k] = (a.bgr >> (8 * chn[k])) & 255u;
    for (int t = first; t < tiles; t += stride) {               // first and stride are block-uniform, so is everything up to `lane`
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x0 = tx * TW, y0 = ty * B;
        const int tw = min(TW, W - x0), th = min(B, H - y0);
        unsigned long long reach = 0;                           // the regions that meet the tile
        for (int j = 0; j < n; ++j) {
            const int* r = R + 4 * j;
            if (r[0] <= x0 + tw - 1 && r[2] >= x0 && r[1] <= y0 + th - 1 && r[3] >= y0) reach |= 1ull << j;
        }
        reach = uniform64(reach);
        if (!reach) continue;
        const int rowb = 3 * tw;
        uint8_t* base = data + (y0 * W + x0) * 3;
        if (a.mode == 0) {
            unsigned acc[RD_COLS] = {0, 0, 0};
            for (int r = wave; r < th; r += 4) {
                const uint8_t* q = base + r * W * 3;
#pragma unroll
                for (int k = 0; k < RD_COLS; ++k)
                    if (lane + 64 * k < rowb) acc[k] += q[lane + 64 * k];
            }
#pragma unroll
            for (int k = 0; k < RD_COLS; ++k) part[wave][lane + 64 * k] = acc[k];
            __syncthreads();                                    // every byte of the tile has been read
            if (tid < RD_ROWB) col[tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            __syncthreads();
            const int cells = (tw + B - 1) / B;
            if (tid < cells * 3) {
                const int c = tid / 3, k = tid - 3 * c, cw = min(B, tw - c * B);
                unsigned s = 0;
                for (int i = 0; i < cw; ++i) s += col[(c * B + i) * 3 + k];
                const unsigned cnt = (unsigned)(cw * th);
                mean[tid] = (s + cnt / 2) / cnt;
            }
            __syncthreads();                                    // the means stand: from here the tile is stored
        }
        unsigned long long xin[RD_COLS] = {0, 0, 0};            // per byte column: the regions whose x range holds it
        for (unsigned long long m = reach; m; m &= m - 1) {
            const int j = __builtin_ctzll(m);
#pragma unroll
            for (int k = 0; k < RD_COLS; ++k)
                if (x0 + px[k] >= R[4 * j] && x0 + px[k] <= R[4 * j + 2]) xin[k] |= 1ull << j;
        }
        for (int r = wave; r < th; r += 4) {
            const int y = y0 + r;
            unsigned long long yin = 0;                         // the regions whose y range holds the row: wave-uniform
            for (unsigned long long m = reach; m; m &= m - 1) {
                const int j = __builtin_ctzll(m);
                if (y >= R[4 * j + 1] && y <= R[4 * j + 3]) yin |= 1ull << j;
            }
            yin = uniform64(yin);
            if (!yin) continue;
            uint8_t* q = base + r * W * 3;
#pragma unroll
            for (int k = 0; k < RD_COLS; ++k)
                if (lane + 64 * k < rowb && (xin[k] & yin))
                    q[lane + 64 * k] = (uint8_t)(a.mode ? fill[k] : mean[cell[k] * 3 + chn[k]]);
        }
    }
}

// uniform batch u8 [N,H,W,3]: blockIdx.y is the frame
__global__ __launch_bounds__(256) void redact_u8(uint8_t* __restrict__ frames, int H, int W, RedactArgs a) {
    redact_frame(frames + (int64_t)blockIdx.y * H * W * 3, H, W, (int)blockIdx.y, a, (int)blockIdx.x, (int)gridDim.x);
}

// frame table: the sizes live on the device; an entry no picture is defined for is skipped as a whole
__global__ __launch_bounds__(256) void redact_refs_u8(const fr_frame_ref* __restrict__ refs, RedactArgs a) {
    const fr_frame_ref r = refs[blockIdx.y];
    if (r.H <= 0 || r.W <= 0 || (int64_t)r.H * r.W * 3 >= (1ll << 31) || !r.data) return;
    redact_frame(const_cast<uint8_t*>(r.data), r.H, r.W, (int)blockIdx.y, a, (int)blockIdx.x, (int)gridDim.x);
}

// the checks both entries share
int redact_check(const char* who, int n, int cap, int block, int mode) {
    FR_REQUIRE(n >= 0 && n <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(cap >= 1 && cap <= RD_CAP, "%s: cap %d out of range (1 .. %d)", who, cap, RD_CAP);
    FR_REQUIRE(block >= 2 && block <= 64, "%s: block %d out of range (2 .. 64)", who, block);
    FR_REQUIRE(mode == 0 || mode == 1, "%s: mode %d is neither 0 (pixelate) nor 1 (fill)", who, mode);
    return FR_OK;
}

// blocks of a frame: about 8192 in all, at least 16 and at most 1024 per frame (and no more than the frame has tiles)
unsigned redact_blocks(int n, int64_t tiles) {
    return (unsigned)std::min<int64_t>(tiles, std::min(1024, std::max(16, (8192 + n - 1) / n)));
}

}  // namespace

extern "C" int fr_redact_u8(uint8_t* frames, int N, int H, int W, const int32_t* counts, int cap, const int32_t* regions,
                            int block, int mode, uint32_t bgr, fr_stream_t stream) {
    if (const int rc = redact_check("fr_redact_u8", N, cap, block, mode)) return rc;
    FR_REQUIRE(H > 0 && W > 0, "fr_redact_u8: bad size (H and W positive)");
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "fr_redact_u8: a %d x %d frame is beyond 2 GiB", H, W);
    if (N == 0) return FR_OK;
    FR_REQUIRE(frames && counts && regions, "fr_redact_u8: null pointer");
    const int TW = block * (64 / block);
    const int64_t tiles = (int64_t)((H + block - 1) / block) * ((W + TW - 1) / TW);
    const RedactArgs a{counts, regions, cap, block, mode, bgr};
    redact_u8<<<dim3(redact_blocks(N, tiles), (unsigned)N), 256, 0, fr_stream(stream)>>>(frames, H, W, a);
    FR_CHECK_LAUNCH("redact_u8");
    return FR_OK;
}

extern "C" int fr_redact_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* counts, int cap, const int32_t* regions,
                                 int block, int mode, uint32_t bgr, fr_stream_t stream) {
    if (const int rc = redact_check("fr_redact_refs_u8", nframes, cap, block, mode)) return rc;
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(refs && counts && regions, "fr_redact_refs_u8: null pointer");
    const RedactArgs a{counts, regions, cap, block, mode, bgr};
    redact_refs_u8<<<dim3(redact_blocks(nframes, 1 << 30), (unsigned)nframes), 256, 0, fr_stream(stream)>>>(refs, a);
    FR_CHECK_LAUNCH("redact_refs_u8");
    return FR_OK;
}
