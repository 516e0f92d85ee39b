// YUV 4:2:0 -> packed BGR u8 on the device: what a video decoder hands out (NV12 / I420, 1.5 bytes per pixel) becomes the
// [H,W,3] BGR frame every other kernel of the library reads, so the frames cross PCIe at half the bytes and the host never
// converts (the reference's capture path decodes H.264 and converts on the CPU inside cv2.VideoCapture:
// /root/reference/infrenceServer.py:573-601).
//
// Arithmetic (include/frhip.h fr_yuv420_to_bgr_u8): nearest chroma - a 2x2 pixel block shares its (U, V) pair -
// and per pixel, in 32-bit integers,
//     y = max(0, Y - y_off) * CY + (1 << 19);  u = U - 128;  v = V - 128
//     B = sat8((y + CUB u) >> 20)   G = sat8((y + CUG u + CVG v) >> 20)   R = sat8((y + CVR v) >> 20)      (arithmetic shift)
// with the six constants passed in by the host (colour.py holds the one table).  The entry points refuse constants with which
// an intermediate could leave int32, so the kernel's wrap-around arithmetic never wraps.
//
// Memory-bound, no LDS: a lane owns a strip of 2 rows x 16 pixels, so every chroma sample is loaded once.  A strip that lies
// wholly inside the rows is two 16-byte Y loads, 16 bytes of chroma (one load of interleaved UV, or 8 + 8 bytes of the U and V
// planes) and 2 x 3 stores of 16 bytes; consecutive lanes take consecutive strips of a row pair, so a wave reads 1 KiB runs and
// writes a 3 KiB run per row.  The vector types are declared with byte alignment: the accesses are correct at any address (an
// odd frame stride, an I420 V plane at an odd offset, a row pitch 3 W that is no multiple of 4) and are aligned 16-byte
// accesses whenever W % 16 == 0 and the frames start on 16 bytes - every common video size from a FrameIngest / RaggedIngest
// arena.  The last strip of a row whose width is no multiple of 16 goes pixel pair by pixel pair, in bytes.
#include "common.h"
#include <algorithm>

namespace {

typedef int4v int4v_u __attribute__((aligned(1)));              // 16-byte access at any byte address

struct YuvK { int y_off, cy, cub, cug, cvg, cvr; };

constexpr int YB_PX = 16;                                       // pixels of a row a lane converts

// sat8(v >> 20) for the 20 fractional bits of the sums: the clamp comes BEFORE the shift (the same value: the shift is
// monotonic).  Written the other way round - clamp(v >> 20, 0, 255) for two neighbouring bytes - hipcc (ROCm 7) forms gfx950's
// v_ashr_pk_u8_i32 and takes the upper half of its result for zero, which it is not on the MI355X: the two bytes packed above
// it came out wrong in about 8 % of the pixels there (docs/KERNEL_NOTES.md; tests/test_yuv_abi.py looks for the instruction).
__device__ __forceinline__ unsigned sat8s(int v) { return (unsigned)min(max(v, 0), (256 << 20) - 1) >> 20; }

// one row of a full strip: 16 Y bytes + the strip's 8 chroma terms -> 48 BGR bytes
__device__ __forceinline__ void row16(const int4v yq, const int (&cb)[8], const int (&cg)[8], const int (&cr)[8], const YuvK k,
                                      uint8_t* __restrict__ out) {
    unsigned d[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                               // 4 pixels -> 3 dwords
        const unsigned yw = (unsigned)yq[q];
        unsigned b[4], g[4], r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int yt = max((int)((yw >> (8 * j)) & 0xffu) - k.y_off, 0) * k.cy + (1 << 19);
            const int c = 2 * q + (j >> 1);
            b[j] = sat8s(yt + cb[c]);
            g[j] = sat8s(yt + cg[c]);
            r[j] = sat8s(yt + cr[c]);
        }
        d[3 * q + 0] = b[0] | g[0] << 8 | r[0] << 16 | b[1] << 24;
        d[3 * q + 1] = g[1] | r[1] << 8 | b[2] << 16 | g[2] << 24;
        d[3 * q + 2] = r[2] | b[3] << 8 | g[3] << 16 | r[3] << 24;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s)
        *reinterpret_cast<int4v_u*>(out + 16 * s) = int4v{(int)d[4 * s], (int)d[4 * s + 1], (int)d[4 * s + 2], (int)d[4 * s + 3]};
}

// Strips first, first + stride, ... of ONE frame.  src: the H*W*3/2 bytes of the YUV frame, dst: its H*W*3 BGR bytes; nothing
// outside either range is touched.  H, W even and positive, H*W*3 < 2^31 (the callers see to it).
__device__ __forceinline__ void convert_strips(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W, int layout,
                                               const YuvK k, int first, int stride) {
    const int chunks = (W + YB_PX - 1) / YB_PX, items = (H >> 1) * chunks;
    const int cw = W >> 1;                                      // chroma samples per row
    const uint8_t* __restrict__ chroma = src + H * W;
    const uint8_t* __restrict__ vplane = chroma + (H >> 1) * cw;                  // I420 only
    for (int i = first; i < items; i += stride) {
        const int ry = i / chunks, x0 = (i - ry * chunks) * YB_PX;
        const int yoff = 2 * ry * W + x0;
        uint8_t* __restrict__ o0 = dst + yoff * 3;
        if (x0 + YB_PX <= W) {
            const int4v ya = *reinterpret_cast<const int4v_u*>(src + yoff);
            const int4v yb = *reinterpret_cast<const int4v_u*>(src + yoff + W);
            unsigned long long uq, vq;                          // 8 U bytes, 8 V bytes
            if (layout == FR_YUV_NV12) {
                const int4v uv = *reinterpret_cast<const int4v_u*>(chroma + ry * W + x0);
                uq = vq = 0;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const unsigned w = (unsigned)uv[c >> 1] >> (16 * (c & 1));
                    uq |= (unsigned long long)(w & 0xffu) << (8 * c);
                    vq |= (unsigned long long)((w >> 8) & 0xffu) << (8 * c);
                }
            } else {
                uq = *reinterpret_cast<const u64_unaligned*>(chroma + ry * cw + (x0 >> 1));
                vq = *reinterpret_cast<const u64_unaligned*>(vplane + ry * cw + (x0 >> 1));
            }
            int cb[8], cg[8], cr[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int u = (int)((uq >> (8 * c)) & 0xffu) - 128, v = (int)((vq >> (8 * c)) & 0xffu) - 128;
                cb[c] = k.cub * u;
                cg[c] = k.cug * u + k.cvg * v;
                cr[c] = k.cvr * v;
            }
            row16(ya, cb, cg, cr, k, o0);
            row16(yb, cb, cg, cr, k, o0 + 3 * W);
        } else {                                                // the row's last, partial strip: a pixel pair at a time
            for (int x = x0; x < W; x += 2) {
                int u, v;
                if (layout == FR_YUV_NV12) {
                    u = chroma[ry * W + x];
                    v = chroma[ry * W + x + 1];
                } else {
                    u = chroma[ry * cw + (x >> 1)];
                    v = vplane[ry * cw + (x >> 1)];
                }
                u -= 128;
                v -= 128;
                const int cb = k.cub * u, cg = k.cug * u + k.cvg * v, cr = k.cvr * v;
#pragma unroll
                for (int p = 0; p < 4; ++p) {                   // (row, column) of the 2x2 block
                    const int at = 2 * ry * W + x + (p >> 1) * W + (p & 1);
                    const int yt = max((int)src[at] - k.y_off, 0) * k.cy + (1 << 19);
                    dst[at * 3 + 0] = (uint8_t)sat8s(yt + cb);
                    dst[at * 3 + 1] = (uint8_t)sat8s(yt + cg);
                    dst[at * 3 + 2] = (uint8_t)sat8s(yt + cr);
                }
            }
        }
    }
}

// uniform batch: block b converts strips of frame b / bpf (bpf blocks cover a frame's strips once)
__global__ __launch_bounds__(256) void yuv420_to_bgr_u8(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                        int layout, YuvK k, int bpf) {
    const int f = blockIdx.x / bpf, b = blockIdx.x - f * bpf;
    const int64_t px = (int64_t)H * W;
    convert_strips(src + f * (px + px / 2), dst + f * px * 3, H, W, layout, k, b * 256 + threadIdx.x, bpf * 256);
}

// frame table: blockIdx.y is the frame, the gridDim.x blocks of a frame walk its strips (the sizes live on the device)
__global__ __launch_bounds__(256) void yuv420_to_bgr_refs_u8(const fr_frame_ref* __restrict__ refs, const uint8_t* const* __restrict__ srcs,
                                                             int layout, YuvK k) {
    const fr_frame_ref r = refs[blockIdx.y];
    const uint8_t* src = srcs[blockIdx.y];
    // an entry no conversion is defined for (odd or empty sides, beyond 2 GiB, no memory) is skipped as a whole: the host checks
    if (r.H <= 0 || r.W <= 0 || ((r.H | r.W) & 1) || (int64_t)r.H * r.W * 3 >= (1ll << 31) || !r.data || !src) return;
    convert_strips(src, const_cast<uint8_t*>(r.data), r.H, r.W, layout, k, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// the checks both entries share; fills k
int yuv_check(const char* who, int layout, int y_off, int cy, int cub, int cug, int cvg, int cvr, YuvK* k) {
    FR_REQUIRE(layout == FR_YUV_NV12 || layout == FR_YUV_I420, "%s: unknown layout %d (FR_YUV_NV12 = 0, FR_YUV_I420 = 1)", who, layout);
    const auto mag = [](int v) { return v < 0 ? -(int64_t)v : (int64_t)v; };
    const int64_t c = std::max(std::max(mag(cub), mag(cvr)), mag(cug) + mag(cvg));
    FR_REQUIRE(y_off >= 0 && y_off <= 255 && cy >= 0 && 255ll * cy + (1 << 19) + 128 * c < (1ll << 31),
               "%s: bad constants (y_off 0 .. 255, CY >= 0, 255 CY + 2^19 + 128 max|chroma term| below 2^31: int32 arithmetic)", who);
    *k = YuvK{y_off, cy, cub, cug, cvg, cvr};
    return FR_OK;
}

}  // namespace

extern "C" int fr_yuv420_to_bgr_u8(const uint8_t* src, uint8_t* dst, int N, int H, int W, int layout, int y_off, int cy, int cub,
                                   int cug, int cvg, int cvr, fr_stream_t stream) {
    YuvK k;
    if (const int rc = yuv_check("fr_yuv420_to_bgr_u8", layout, y_off, cy, cub, cug, cvg, cvr, &k)) return rc;
    FR_REQUIRE(N >= 0 && H > 0 && W > 0, "fr_yuv420_to_bgr_u8: bad size (N >= 0, H and W positive)");
    FR_REQUIRE(!(H & 1) && !(W & 1), "fr_yuv420_to_bgr_u8: odd size %d x %d (4:2:0 needs H and W even)", H, W);
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "fr_yuv420_to_bgr_u8: a %d x %d frame is beyond 2 GiB", H, W);
    if (N == 0) return FR_OK;
    FR_REQUIRE(src && dst, "fr_yuv420_to_bgr_u8: null pointer");
    const int64_t items = (int64_t)(H / 2) * ((W + YB_PX - 1) / YB_PX), bpf = (items + 255) / 256;
    FR_REQUIRE(bpf * N < (1ll << 31), "fr_yuv420_to_bgr_u8: too many frames (%d of %d x %d)", N, H, W);
    yuv420_to_bgr_u8<<<(unsigned)(bpf * N), 256, 0, fr_stream(stream)>>>(src, dst, H, W, layout, k, (int)bpf);
    FR_CHECK_LAUNCH("yuv420_to_bgr_u8");
    return FR_OK;
}

extern "C" int fr_yuv420_to_bgr_refs_u8(const fr_frame_ref* dst_refs, const uint8_t* const* src_ptrs, int nframes, int layout,
                                        int y_off, int cy, int cub, int cug, int cvg, int cvr, fr_stream_t stream) {
    YuvK k;
    if (const int rc = yuv_check("fr_yuv420_to_bgr_refs_u8", layout, y_off, cy, cub, cug, cvg, cvr, &k)) return rc;
    FR_REQUIRE(nframes >= 0 && nframes <= 65535, "fr_yuv420_to_bgr_refs_u8: bad size (0 .. 65535 frames)");
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(dst_refs && src_ptrs, "fr_yuv420_to_bgr_refs_u8: null pointer");
    // about 4096 blocks in all (16 waves per SIMD of 256 CUs), at least 8 per frame: a 1080p frame is 254 blocks' worth of strips
    const int per = std::min(1024, std::max(8, (4096 + nframes - 1) / nframes));
    yuv420_to_bgr_refs_u8<<<dim3((unsigned)per, (unsigned)nframes), 256, 0, fr_stream(stream)>>>(dst_refs, src_ptrs, layout, k);
    FR_CHECK_LAUNCH("yuv420_to_bgr_refs_u8");
    return FR_OK;
}
