// det_size: the detection canvas of insightface's FaceAnalysis.prepare(det_size=(dw, dh)) - the frame resized to fit, placed
// top-left, zero padded (the reference's prepare(ctx_id=0) means 640 x 640: /root/reference/infrenceServer.py:416, SURVEY a-1) -
// and the way back: detections of the canvas divided by the frame's scale.
//
// fr_letterbox_u8 makes the canvases of a RAGGED batch (frames of differing sizes: include/frhip.h fr_frame_ref) in one
// launch.  The resize is the pyramid's (detect_math.h lerp_coord / bilerp: f32, half-pixel centres, edge clamp) applied to
// the BGR bytes, rounded floor(v + 0.5) in f64 and clamped as the alignment warp rounds (align.hip); the library is built with
// -fno-fast-math -ffp-contract=off, so the bytes are those of oracle/detect.py resize_bilinear + that rounding.
//
// Memory-bound: a 1080p frame on a 640 x 360 image reads two source rows per canvas row and writes 1.2 MB.
// A block makes a tile of LB_TH rows x LB_TW canvas pixels of ONE frame (block-uniform: blockIdx.y).  Its lerp tables (source
// row offsets + wy per tile row, source column offset + wx per tile column) are computed once by LB_TH + LB_TW threads, as
// pnet_conv1.hip builds them.  A wave owns 64 adjacent canvas pixels of a row: their source pixels are one run of the source
// row, read as ONE unaligned 8-byte load per source row and pixel (both corners are 6 adjacent bytes: BGR BGR) - pulled back
// at the end of every frame, each being an allocation of its own.  The tile's bytes are collected in LDS and leave as 16-byte
// stores; tiles that lie in the padding store zeros and read nothing.
#include "detect_math.h"

namespace {

constexpr int LB_TH = 16, LB_TW = 64, LB_ROWB = LB_TW * 3;        // tile: 16 rows x 64 pixels = 16 x 192 bytes

template <bool VEC16>
__global__ __launch_bounds__(256) void letterbox_u8(const fr_frame_ref* __restrict__ refs, uint8_t* __restrict__ canvas,
                                                    int dh, int dw) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[LB_TH * LB_ROWB];
    __shared__ int4v tab[LB_TH + LB_TW];       // rows {i0 * W * 3, i1 * W * 3, wy, -}   columns {x0 * 3, wx, x1 != x0, -}
    const int tid = threadIdx.x;
    const int tiles_x = (dw + LB_TW - 1) / LB_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * LB_TH, x0 = tx * LB_TW;
    const fr_frame_ref r = refs[blockIdx.y];
    const int H = r.H, W = r.W, nh = min(r.nh, dh), nw = min(r.nw, dw);
    uint8_t* out = canvas + (int64_t)blockIdx.y * dh * dw * 3;
    const bool image = y0 < nh && x0 < nw && H > 0 && W > 0;          // block-uniform: the tile holds pixels of the image

    if (image) {
        if (tid < LB_TH + LB_TW) {
            int4v e;
            if (tid < LB_TH) {
                const Lerp l = lerp_coord(y0 + tid, (float)H / (float)nh, H);
                e = int4v{l.i0 * W * 3, l.i1 * W * 3, __float_as_int(l.w), 0};
            } else {
                const Lerp l = lerp_coord(x0 + tid - LB_TH, (float)W / (float)nw, W);
                e = int4v{l.i0 * 3, __float_as_int(l.w), l.i1 != l.i0 ? 1 : 0, 0};
            }
            tab[tid] = e;
        }
        __syncthreads();
        const int px = tid & 63, x = x0 + px;
        const int4v ce = tab[LB_TH + px];
        const float wx = __int_as_float(ce[1]);
        const bool two = ce[2] != 0;
        const int lim = H * W * 3 - 8;          // the last offset an 8-byte load of THIS frame may start at (< 0: a frame below 8 bytes)
        unsigned long long q[LB_TH / 4][2];
        // all loads first: eight independent 8-byte loads per thread in flight
#pragma unroll
        for (int u = 0; u < LB_TH / 4; ++u) {
            const int4v re = tab[(tid >> 6) + 4 * u];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int off = re[a] + ce[0];
                if (lim >= 0) {
                    const int c8 = min(off, lim);
                    q[u][a] = *reinterpret_cast<const u64_unaligned*>(r.data + c8) >> ((off - c8) * 8);
                } else {                        // one or two pixels in all: bytes
                    unsigned long long v = 0;
                    for (int b = 0; b < 6; ++b)
                        if (off + b < H * W * 3) v |= (unsigned long long)r.data[off + b] << (8 * b);
                    q[u][a] = v;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < LB_TH / 4; ++u) {
            const int row = (tid >> 6) + 4 * u;
            const float wy = __int_as_float(tab[row][2]);
            const bool inside = y0 + row < nh && x < nw;
            unsigned char* t = tile + row * LB_ROWB + px * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float p00 = (float)(unsigned)((q[u][0] >> (8 * c)) & 0xff), p01 = (float)(unsigned)((q[u][0] >> (24 + 8 * c)) & 0xff);
                const float p10 = (float)(unsigned)((q[u][1] >> (8 * c)) & 0xff), p11 = (float)(unsigned)((q[u][1] >> (24 + 8 * c)) & 0xff);
                const float v = bilerp(p00, two ? p01 : p00, p10, two ? p11 : p10, wx, wy);
                double d = floor((double)v + 0.5);
                d = d < 0 ? 0 : (d > 255 ? 255 : d);
                t[c] = inside ? (unsigned char)d : (unsigned char)0;
            }
        }
        __syncthreads();
    }
    // ---- the tile leaves: 16 rows x 12 pieces of 16 bytes (dw % 16 == 0: a piece is inside the canvas row or outside it as a whole)
    if constexpr (VEC16) {
        if (tid < LB_TH * (LB_ROWB / 16)) {
            const int row = tid / (LB_ROWB / 16), piece = tid - row * (LB_ROWB / 16);
            const int y = y0 + row, xb = x0 * 3 + piece * 16;
            if (y < dh && xb < dw * 3) {
                const int4v v = image ? *reinterpret_cast<const int4v*>(tile + row * LB_ROWB + piece * 16) : int4v{0, 0, 0, 0};
                *reinterpret_cast<int4v*>(out + ((int64_t)y * dw * 3 + xb)) = v;
            }
        }
    } else {
        for (int e = tid; e < LB_TH * LB_ROWB; e += 256) {
            const int row = e / LB_ROWB, b = e - row * LB_ROWB;
            const int y = y0 + row, xb = x0 * 3 + b;
            if (y < dh && xb < dw * 3) out[(int64_t)y * dw * 3 + xb] = image ? tile[e] : (unsigned char)0;
        }
    }
}

__global__ __launch_bounds__(256) void detections_unscale(float* __restrict__ boxes, float* __restrict__ kps,
                                                          const int32_t* __restrict__ counts, const float* __restrict__ det_scale,
                                                          int nframes, int cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // (slot, coordinate 0..13): 4 of the box, 10 of the landmarks
    if (i >= nframes * cap * 14) return;
    const int slot = i / 14, c = i - slot * 14, f = slot / cap;
    if (slot - f * cap >= counts[f]) return;
    float* p = c < 4 ? boxes + (int64_t)slot * 4 + c : kps + (int64_t)slot * 10 + (c - 4);
    *p = *p / det_scale[f];
}

}  // namespace

extern "C" int fr_letterbox_u8(const fr_frame_ref* refs, int nframes, uint8_t* canvas, int dh, int dw, fr_stream_t stream) {
    FR_REQUIRE(refs && canvas, "fr_letterbox_u8: null pointer");
    FR_REQUIRE(nframes > 0 && nframes <= 65535 && dh > 0 && dw > 0 && (int64_t)dh * dw * 3 < (1ll << 31),
               "fr_letterbox_u8: bad size (1 .. 65535 frames, canvas below 2 GiB)");
    const dim3 grid((unsigned)(((dh + LB_TH - 1) / LB_TH) * ((dw + LB_TW - 1) / LB_TW)), (unsigned)nframes);
    if (dw % 16 == 0 && (reinterpret_cast<uintptr_t>(canvas) & 15) == 0)
        letterbox_u8<true><<<grid, 256, 0, fr_stream(stream)>>>(refs, canvas, dh, dw);
    else
        letterbox_u8<false><<<grid, 256, 0, fr_stream(stream)>>>(refs, canvas, dh, dw);
    FR_CHECK_LAUNCH("letterbox_u8");
    return FR_OK;
}

extern "C" int fr_detections_unscale(float* boxes, float* kps, const int32_t* counts, const float* det_scale, int nframes,
                                     int cap, fr_stream_t stream) {
    FR_REQUIRE(boxes && kps && counts && det_scale, "fr_detections_unscale: null pointer");
    FR_REQUIRE(nframes > 0 && cap > 0 && (int64_t)nframes * cap * 14 < (1ll << 31), "fr_detections_unscale: bad size");
    detections_unscale<<<fr_cdiv((int64_t)nframes * cap * 14, 256), 256, 0, fr_stream(stream)>>>(boxes, kps, counts, det_scale, nframes, cap);
    FR_CHECK_LAUNCH("detections_unscale");
    return FR_OK;
}
