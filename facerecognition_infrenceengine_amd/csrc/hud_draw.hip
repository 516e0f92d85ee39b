// The HUD of the live path (the reference's recognize_faces returns the frame with one drawn on every face:
// infrenceServer.py:418-513), drawn into the BGR frames where they already are: on the device, behind the
// engine pass, so that only what a viewer needs crosses the link.
//
// The picture is DEFINED by tests/helpers/hud_ref.py (include/frhip.h fr_hud_draw_u8): per pixel a fold over the
// frame's faces in order and, within a face, over its layers - box blend, corner ticks, two bars with their fills and letters,
// panel background, border and text.  Every layer is a predicate on the pixel's own (x, y) and a colour rule, no layer reads a
// neighbouring pixel, and all of it is 32-bit integer arithmetic: the bytes are those of the NumPy definition.  With s = scale:
//     box    [x1,x2] x [y1,y2] minus [x1+2s,x2-2s] x [y1+2s,y2-2s]                 p = (102 c + 154 p + 128) >> 8
//     ticks  L = 15 s, h = s, per corner (cx, cy), u = x - cx, v = y - cy:          p = c
//            [cx,cx+L] x [cy-h,cy+h], [cx-h,cx+h] x [cy,cy+L], 0 <= u,v <= L and |u + v - L| <= h
//     bars   bx = x2 + 10 s (detection) and bx + 12 s (recognition): outline [b,b+6s] x [y1,y2], s thick, (100,100,100);
//            fill [b,b+6s] x [y2-height,y2] in (255,140,0) / c; letter 'D' / 'R' at (b - 2 s, y1 - 12 s), glyph scale s, white
//     panel  g = 2 s, pw = maxlen 6 g + 20 s, ph = nlines 18 s + 10 s, px = max(0, min(x1, W - pw)), py = max(0, y2 + 10 s),
//            py = max(0, y1 - ph - 10 s) if py + ph > H; background p = (205 * 30 + 51 p + 128) >> 8, border s thick in c,
//            line i in white at (px + 10 s, py + s + 18 s i)
//
// A GATHER over output pixels: a scatter per face could not keep the fold's order where two faces' HUDs overlap.  The frame is
// cut into tiles of HD_TH rows x HD_TW pixels as letterbox_u8 cuts its canvas; blockIdx.y is the frame and the gridDim.x blocks
// of a frame walk its tiles (a frame table's sizes live on the device, so the grid cannot follow them).  A block loads its
// frame's records into LDS once, one thread per face normalises a record and computes the face's panel and its EXTENT - the
// bounding rectangle of all its layers.  A tile no extent meets is skipped without touching memory (block-uniform: the test
// reads LDS only); the text and the font are fetched into LDS when the first tile is met.  In a tile that is met a lane owns a
// pixel column and four rows, reads a pixel's three bytes, folds the faces whose extent holds the pixel, in order, and writes
// the bytes back only where a layer hit: untouched pixels are never written, frames may start at any byte address.
// Coordinates may be negative: only values known to be non-negative are divided.
#include "common.h"
#include <algorithm>

namespace {

constexpr int HD_TH = 16, HD_TW = 64;                 // tile: 16 rows x 64 pixels (192 bytes of a row per wave)
constexpr int HD_K = FR_HUD_K;                        // ints of a record in global memory
constexpr int HD_F = 24;                              // ints of a face in LDS: the record, then px py pw ph, then the extent
constexpr int HD_CAP = FR_HUD_MAX_CAP, HD_CHARS = FR_HUD_MAX_CHARS, HD_LINES = 4, HD_GLYPHS = 95;
constexpr int HD_LIMIT = 1 << 20;                     // coordinates are clamped to +-2^20: no sum below leaves int32

struct HudArgs {
    const int32_t* counts;
    const int32_t* faces;
    const uint8_t* text;
    const uint8_t* font;
    int cap, max_chars, s;
};

__device__ __forceinline__ bool in_rect(int x, int y, int xa, int ya, int xb, int yb) {
    return x >= xa && x <= xb && y >= ya && y <= yb;
}

// lit pixel of one character cell?  u, v >= 0: offsets from the cell's top-left corner, u < 6 g, v < 7 g
__device__ __forceinline__ bool glyph_lit(const uint8_t* fnt, unsigned ch, unsigned u, unsigned v, unsigned g) {
    const unsigned cu = u / g;
    if (cu >= 5) return false;
    unsigned k = ch - 0x20u;
    if (k >= (unsigned)HD_GLYPHS) k = 0x3Fu - 0x20u;             // a byte outside 0x20 .. 0x7E is drawn as '?'
    return (fnt[k * 7 + v / g] >> (4 - cu)) & 1u;
}

// one face folded into one pixel; F: the face's HD_F ints, txt: its 4 x max_chars bytes
__device__ __forceinline__ void fold_face(const int* __restrict__ F, const uint8_t* __restrict__ txt, const uint8_t* __restrict__ fnt,
                                          int max_chars, int s, int x, int y, int (&p)[3], bool& hit) {
    const int x1 = F[0], y1 = F[1], x2 = F[2], y2 = F[3];
    const int c[3] = {F[4], F[5], F[6]};
    // 1. box
    if (in_rect(x, y, x1, y1, x2, y2) && !in_rect(x, y, x1 + 2 * s, y1 + 2 * s, x2 - 2 * s, y2 - 2 * s)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) p[k] = (102 * c[k] + 154 * p[k] + 128) >> 8;
        hit = true;
    }
    // 2. corner ticks: a corner's three strokes lie in [cx - h, cx + L] x [cy - h, cy + L], so most pixels of an extent are
    //    turned away by the four range tests in front
    const int L = 15 * s, h = s;
    if (((x >= x1 - h && x <= x1 + L) || (x >= x2 - h && x <= x2 + L)) && ((y >= y1 - h && y <= y1 + L) || (y >= y2 - h && y <= y2 + L))) {
        bool t = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int u = x - ((k & 1) ? x2 : x1), v = y - ((k & 2) ? y2 : y1);
            t |= (u >= 0 && u <= L && v >= -h && v <= h) || (u >= -h && u <= h && v >= 0 && v <= L) ||
                 (u >= 0 && v >= 0 && u <= L && v <= L && abs(u + v - L) <= h);
        }
        if (t) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = c[k];
            hit = true;
        }
    }
    // 3. bars: outline, fill, letter - detection first
    {
        const int bx = x2 + 10 * s;
        if (x >= bx - 2 * s && x <= bx + 18 * s) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int b0 = bx + 12 * s * k, height = k ? F[8] : F[7];
                if (in_rect(x, y, b0, y1, b0 + 6 * s, y2) && !in_rect(x, y, b0 + s, y1 + s, b0 + 5 * s, y2 - s)) {
                    p[0] = p[1] = p[2] = 100;
                    hit = true;
                }
                if (in_rect(x, y, b0, y2 - height, b0 + 6 * s, y2)) {
                    p[0] = k ? c[0] : 255;
                    p[1] = k ? c[1] : 140;
                    p[2] = k ? c[2] : 0;
                    hit = true;
                }
                const int u = x - (b0 - 2 * s), v = y - (y1 - 12 * s);
                if (u >= 0 && v >= 0 && u < 6 * s && v < 7 * s &&
                    glyph_lit(fnt, k ? 'R' : 'D', (unsigned)u, (unsigned)v, (unsigned)s)) {
                    p[0] = p[1] = p[2] = 255;
                    hit = true;
                }
            }
        }
    }
    // 4. panel: background, border, text
    {
        const int px = F[14], py = F[15], pw = F[16], ph = F[17];
        if (in_rect(x, y, px, py, px + pw, py + ph)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[k] = (205 * 30 + 51 * p[k] + 128) >> 8;
            hit = true;
            if (!in_rect(x, y, px + s, py + s, px + pw - s, py + ph - s)) {
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = c[k];
            }
            const int u = x - (px + 10 * s), vt = y - (py + s);
            if (u >= 0 && vt >= 0) {
                const unsigned g = 2u * s, line = (unsigned)vt / (18u * s), v = (unsigned)vt - line * 18u * s;
                if (line < (unsigned)F[9] && v < 7 * g) {
                    const unsigned ci = (unsigned)u / (6 * g);
                    if (ci < (unsigned)F[10 + line] &&
                        glyph_lit(fnt, txt[line * max_chars + ci], (unsigned)u - ci * 6 * g, v, g))
                        p[0] = p[1] = p[2] = 255;
                }
            }
        }
    }
}

// Tiles first, first + stride, ... of ONE frame of H x W at `data` (H, W positive, H*W*3 < 2^31: the callers see to it);
// f: its row of counts / faces / text.  Nothing outside [data, data + H*W*3) is touched.
__device__ __forceinline__ void hud_frame(uint8_t* __restrict__ data, int H, int W, int f, const HudArgs a, int first, int stride) {
    __shared__ int F[HD_CAP * HD_F];
    __shared__ __attribute__((aligned(4))) uint8_t txt[HD_CAP * HD_LINES * HD_CHARS];
    __shared__ uint8_t fnt[HD_GLYPHS * 7 + 3];
    const int tid = threadIdx.x, s = a.s;
    const int n = min(max(a.counts[f], 0), a.cap);              // slots j >= counts[f] are never read
    if (n == 0) return;                                         // block-uniform
    if (tid < n) {
        const int32_t* __restrict__ rec = a.faces + ((int64_t)f * a.cap + tid) * HD_K;
        int* o = F + tid * HD_F;
        const int x1 = min(max(rec[0], -HD_LIMIT), HD_LIMIT), y1 = min(max(rec[1], -HD_LIMIT), HD_LIMIT);
        const int x2 = min(max(rec[2], -HD_LIMIT), HD_LIMIT), y2 = min(max(rec[3], -HD_LIMIT), HD_LIMIT);
        const int span = max(y2 - y1, 0);
        const int nlines = min(max(rec[9], 0), HD_LINES);
        o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2;
        o[4] = rec[4] & 255; o[5] = rec[5] & 255; o[6] = rec[6] & 255;
        o[7] = max(0, min(rec[7], span));
        o[8] = max(0, min(rec[8], span));
        o[9] = nlines;
        int maxlen = 0;
#pragma unroll
        for (int i = 0; i < HD_LINES; ++i) {
            const int len = i < nlines ? min(max(rec[10 + i], 0), a.max_chars) : 0;
            o[10 + i] = len;
            maxlen = max(maxlen, len);
        }
        const int pw = maxlen * 12 * s + 20 * s, ph = nlines * 18 * s + 10 * s;
        const int px = max(0, min(x1, W - pw));
        int py = max(0, y2 + 10 * s);
        if (py + ph > H) py = max(0, y1 - ph - 10 * s);
        o[14] = px; o[15] = py; o[16] = pw; o[17] = ph;
        // the extent: box, ticks (x1 - s .. x2 + 15 s, y1 - s .. y2 + 15 s), bars and letters (.. x2 + 28 s, y1 - 12 s ..), panel
        o[18] = min(min(x1, x2) - s, px);
        o[19] = min(min(y1, y2) - 12 * s, py);
        o[20] = max(max(x1, x2) + 28 * s, px + pw);
        o[21] = max(max(y1, y2) + 15 * s, py + ph);
        o[22] = o[23] = 0;
    }
    __syncthreads();
    const int tiles_x = (W + HD_TW - 1) / HD_TW, tiles = tiles_x * ((H + HD_TH - 1) / HD_TH);
    bool staged = false;
    for (int t = first; t < tiles; t += stride) {               // first and stride are block-uniform, so is everything up to `lane`
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int x0 = tx * HD_TW, y0 = ty * HD_TH;
        const int xe = min(x0 + HD_TW, W) - 1, ye = min(y0 + HD_TH, H) - 1;
        unsigned long long reach = 0;                           // the faces whose extent meets the tile
        for (int j = 0; j < n; ++j) {
            const int* e = F + j * HD_F + 18;
            if (e[0] <= xe && e[2] >= x0 && e[1] <= ye && e[3] >= y0) reach |= 1ull << j;
        }
        if (!reach) continue;
        if (!staged) {                                          // the first tile that is met: text and font into LDS
            for (int i = tid; i < n * HD_LINES * a.max_chars; i += 256) {
                const int j = i / (HD_LINES * a.max_chars);
                txt[i] = a.text[((int64_t)f * a.cap + j) * HD_LINES * a.max_chars + (i - j * HD_LINES * a.max_chars)];
            }
            for (int i = tid; i < HD_GLYPHS * 7; i += 256) fnt[i] = a.font[i];
            __syncthreads();
            staged = true;
        }
        const int x = x0 + (tid & 63);
        if (x >= W) continue;
        for (int r = 0; r < HD_TH / 4; ++r) {
            const int y = y0 + (tid >> 6) + 4 * r;
            if (y >= H) break;
            uint8_t* __restrict__ q = data + (y * W + x) * 3;
            bool hit = false, loaded = false;
            int p[3] = {0, 0, 0};
            unsigned long long m = reach;
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const int* Fj = F + j * HD_F;
                if (!in_rect(x, y, Fj[18], Fj[19], Fj[20], Fj[21])) continue;
                if (!loaded) {
                    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
                    loaded = true;
                }
                fold_face(Fj, txt + j * HD_LINES * a.max_chars, fnt, a.max_chars, s, x, y, p, hit);
            }
            if (hit) {
                q[0] = (uint8_t)p[0]; q[1] = (uint8_t)p[1]; q[2] = (uint8_t)p[2];
            }
        }
    }
}

// uniform batch u8 [N,H,W,3]: blockIdx.y is the frame
__global__ __launch_bounds__(256) void hud_draw_u8(uint8_t* __restrict__ frames, int H, int W, HudArgs a) {
    hud_frame(frames + (int64_t)blockIdx.y * H * W * 3, H, W, (int)blockIdx.y, a, (int)blockIdx.x, (int)gridDim.x);
}

// frame table: the sizes live on the device; an entry no drawing is defined for is skipped as a whole
__global__ __launch_bounds__(256) void hud_draw_refs_u8(const fr_frame_ref* __restrict__ refs, HudArgs a) {
    const fr_frame_ref r = refs[blockIdx.y];
    if (r.H <= 0 || r.W <= 0 || (int64_t)r.H * r.W * 3 >= (1ll << 31) || !r.data) return;
    hud_frame(const_cast<uint8_t*>(r.data), r.H, r.W, (int)blockIdx.y, a, (int)blockIdx.x, (int)gridDim.x);
}

// the checks both entries share
int hud_check(const char* who, int n, int cap, int max_chars, int scale) {
    FR_REQUIRE(n >= 0 && n <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(cap >= 1 && cap <= HD_CAP, "%s: cap %d out of range (1 .. %d)", who, cap, HD_CAP);
    FR_REQUIRE(max_chars >= 1 && max_chars <= HD_CHARS, "%s: max_chars %d out of range (1 .. %d)", who, max_chars, HD_CHARS);
    FR_REQUIRE(scale >= 1 && scale <= 8, "%s: scale %d out of range (1 .. 8)", who, scale);
    return FR_OK;
}

// blocks of a frame: about 8192 in all, at least 16 and at most 1024 per frame (and no more than the frame has tiles)
unsigned hud_blocks(int n, int64_t tiles) {
    return (unsigned)std::min<int64_t>(tiles, std::min(1024, std::max(16, (8192 + n - 1) / n)));
}

}  // namespace

extern "C" int fr_hud_draw_u8(uint8_t* frames, int N, int H, int W, const int32_t* counts, int cap, const int32_t* faces,
                              const uint8_t* text, int max_chars, const uint8_t* font, int scale, fr_stream_t stream) {
    if (const int rc = hud_check("fr_hud_draw_u8", N, cap, max_chars, scale)) return rc;
    FR_REQUIRE(H > 0 && W > 0, "fr_hud_draw_u8: bad size (H and W positive)");
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "fr_hud_draw_u8: a %d x %d frame is beyond 2 GiB", H, W);
    if (N == 0) return FR_OK;
    FR_REQUIRE(frames && counts && faces && text && font, "fr_hud_draw_u8: null pointer");
    const int64_t tiles = (int64_t)((H + HD_TH - 1) / HD_TH) * ((W + HD_TW - 1) / HD_TW);
    const HudArgs a{counts, faces, text, font, cap, max_chars, scale};
    hud_draw_u8<<<dim3(hud_blocks(N, tiles), (unsigned)N), 256, 0, fr_stream(stream)>>>(frames, H, W, a);
    FR_CHECK_LAUNCH("hud_draw_u8");
    return FR_OK;
}

extern "C" int fr_hud_draw_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* counts, int cap, const int32_t* faces,
                                   const uint8_t* text, int max_chars, const uint8_t* font, int scale, fr_stream_t stream) {
    if (const int rc = hud_check("fr_hud_draw_refs_u8", nframes, cap, max_chars, scale)) return rc;
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(refs && counts && faces && text && font, "fr_hud_draw_refs_u8: null pointer");
    const HudArgs a{counts, faces, text, font, cap, max_chars, scale};
    hud_draw_refs_u8<<<dim3(hud_blocks(nframes, 1 << 30), (unsigned)nframes), 256, 0, fr_stream(stream)>>>(refs, a);
    FR_CHECK_LAUNCH("hud_draw_refs_u8");
    return FR_OK;
}
