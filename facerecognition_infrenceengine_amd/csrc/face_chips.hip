// Face chips: a square around each face is cut out of the full-size BGR frames where they already are - on the device, behind
// the engine pass and in front of the redactor and the HUD draw - and resampled to S x S bytes, so that the face itself can be
// handed back (unknown-person events, recognition logs, watch-list dashboards) without the host ever holding the frame.
//
// The picture is DEFINED by tests/helpers/chip_ref.py (include/frhip.h fr_face_chips_u8), integers only.  A
// record (frame, x0, y0, side) names the square [x0, x0 + L) x [y0, y0 + L), L = side, anywhere; a pixel outside the frame reads
// as the fill colour.  Per axis, output j weighs source position p (relative to the square's origin):
//     box      L >= S: w = min((j + 1) L, (p + 1) S) - max(j L, p S) where positive (a source pixel is S units long, an output
//              pixel L); the weights of an output sum to T = L
//     bilinear L <  S: n = (2 j + 1) L - S, p = floor(n / 2 S) (-1 at the leading edge), t = n - 2 S p; taps p (2 S - t) and
//              p + 1 (t), not clamped to the square; T = 2 S
// and a byte is (sum_y sum_x w_y w_x pix + T^2 / 2) / T^2: round half up, the identity at L == S.  The largest sum is
// 255 * 4096^2 + 4096^2 / 2 < 2^32: UNSIGNED 32-bit accumulators throughout (a signed one does not hold it).
//
// Work: blockIdx.x is the chip, blockIdx.y a band of BR = ceil(S / 16) output rows; 256 threads.
// Box regime: the band's source rows are walked ONCE, top to bottom.  The segment of the frame row the square covers (at most
// 4096 pixels, 12 KiB) is staged in LDS - aligned dwords, consecutive lanes consecutive dwords, the ragged head and tail bytes
// on their own, nothing outside the frame's bytes read - into one of two buffers, so that one barrier per row is enough.  An
// output column is owned by G = 2^k <= 256 / S adjacent lanes: each sums every G-th pixel of the column's span, weighted, from
// LDS, and a butterfly of shuffles leaves the row sum (<= 255 L) in all of them.  Source pixel length S <= output length L, so
// a source row feeds at most two output rows: the walk adds w h to the row it is in, and where the source row ends the output
// row, divides, stores, and starts the next with the remainder - (i, p) are block-uniform, no thread diverges on them.
// Bilinear regime: the source is smaller than the output, so a thread (one output column) gathers its four taps per output
// byte straight from memory; there is nothing to stage.
// A record no picture is defined for - frame index outside the batch, side outside 1 .. 4096, a coordinate beyond +-2^20, a
// table entry that is null, non-positive or of 2 GiB or more - is checked HERE (records are device data) and gives pure fill.
#include "common.h"

namespace {

constexpr int CH_LIMIT = 1 << 20;                     // |x0|, |y0|
constexpr int CH_MAX_F = 1 << 20;                     // chips of a call
constexpr int CH_ROW_DW = FR_CHIP_MAX_SIDE * 3 / 4 + 2;   // dwords of a staged row segment: 12 KiB and the alignment slack

struct ChipArgs {
    const int32_t* chips;
    int size;
    uint32_t bgr;
    uint8_t* out;
};

// floor(a / b) for b > 0 and a >= -b
__device__ __forceinline__ int floor_div_near(int a, int b) { return (a + b) / b - 1; }

// Band blockIdx.y of chip blockIdx.x.  data: the frame (H x W, H*W*3 < 2^31), or null: no picture, the chip is fill.
__device__ __forceinline__ void chip_band(const uint8_t* __restrict__ data, int H, int W, int x0, int y0, int L, const ChipArgs a) {
    __shared__ uint32_t stage[2][CH_ROW_DW];
    const int tid = threadIdx.x, S = a.size;
    const int BR = (S + 15) >> 4;
    const int i0 = (int)blockIdx.y * BR, i1 = min(i0 + BR, S);
    if (i0 >= i1) return;                                               // block-uniform
    const unsigned fill[3] = {a.bgr & 255u, (a.bgr >> 8) & 255u, (a.bgr >> 16) & 255u};
    uint8_t* __restrict__ out = a.out + (int64_t)blockIdx.x * S * S * 3;
    if (!data) {
        for (int k = tid; k < (i1 - i0) * S * 3; k += 256) out[i0 * S * 3 + k] = (uint8_t)fill[k % 3];
        return;
    }
    if (L < S) {                                                        // ---- bilinear: two taps per axis, gathered
        const int j = tid;
        if (j >= S) return;
        const int nx = (2 * j + 1) * L - S, px = floor_div_near(nx, 2 * S), tx = nx - 2 * S * px;
        const int xa = x0 + px, xb = xa + 1;
        const bool ina = xa >= 0 && xa < W, inb = xb >= 0 && xb < W;
        const unsigned wxa = (unsigned)(2 * S - tx), wxb = (unsigned)tx, half = 2u * S * S, den = 4u * S * S;
        for (int i = i0; i < i1; ++i) {
            const int ny = (2 * i + 1) * L - S, py = floor_div_near(ny, 2 * S), ty = ny - 2 * S * py;
            unsigned acc[3] = {0, 0, 0};
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int y = y0 + py + r;
                const unsigned wy = r ? (unsigned)ty : (unsigned)(2 * S - ty);
                const bool iny = y >= 0 && y < H;
                const uint8_t* q = data + ((iny ? y : 0) * W) * 3;      // read only where the pixel exists
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned va = (iny && ina) ? q[xa * 3 + c] : fill[c];
                    const unsigned vb = (iny && inb) ? q[xb * 3 + c] : fill[c];
                    acc[c] += wy * (wxa * va + wxb * vb);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(i * S + j) * 3 + c] = (uint8_t)((acc[c] + half) / den);
        }
        return;
    }
    // ---- box: the exact area average
    int G = 1;
    while (G < 16 && 2 * G * S <= 256) G *= 2;                          // lanes of a column: 16, 4, 2, 1 at S = 16, 48, 112, 256
    const int j = tid / G, g = tid & (G - 1);
    const int ra = max(-x0, 0), rb = min(L, W - x0);                    // the square's columns [ra, rb) exist in the frame
    // the column's span of source positions, cut to the columns that exist; empty for the lanes past the last column
    const int jl = j * L, jh = jl + L;
    const int lo = j < S ? max(jl / S, ra) : 0, hi = j < S ? min((jh - 1) / S, rb - 1) : -1;
    const unsigned LL = (unsigned)L * (unsigned)L;
    const int pend = (i1 * L + S - 1) / S;
    int i = i0;
    unsigned acc[3] = {0, 0, 0};
    for (int p = i0 * L / S; p < pend; ++p) {
        const int y = y0 + p;
        unsigned h[3];
        if (y >= 0 && y < H && ra < rb) {                               // block-uniform
            uint32_t* buf = stage[p & 1];
            const uint8_t* src = data + (y * W + x0 + ra) * 3;          // the first byte of the segment
            const int nbytes = (rb - ra) * 3;
            const int off = (int)((uintptr_t)src & 3);                  // the segment lies at buf bytes [off, off + nbytes)
            const int head = min((4 - off) & 3, nbytes);                // bytes in front of the first aligned dword
            const int ndw = (nbytes - head) >> 2, tail = nbytes - head - 4 * ndw;
            uint8_t* bufb = reinterpret_cast<uint8_t*>(buf);
            const uint32_t* src4 = reinterpret_cast<const uint32_t*>(src + head);
            const int dw0 = (off + head) >> 2;
            for (int k = tid; k < ndw; k += 256) buf[dw0 + k] = src4[k];
            if (tid < head) bufb[off + tid] = src[tid];
            if (tid >= 64 && tid < 64 + tail) bufb[off + head + 4 * ndw + tid - 64] = src[head + 4 * ndw + tid - 64];
            // two buffers, one barrier: whoever writes row p + 2 into this buffer has passed row p + 1's barrier, behind
            // every thread's reads of row p (the rows that exist are consecutive, so no staged row is skipped in between)
            __syncthreads();
            unsigned hs[3] = {0, 0, 0}, ws = 0;
            for (int q = lo + g; q <= hi; q += G) {
                const unsigned w = (unsigned)(min(jh, (q + 1) * S) - max(jl, q * S));
                const uint8_t* b = bufb + off + (q - ra) * 3;
                hs[0] += w * b[0];
                hs[1] += w * b[1];
                hs[2] += w * b[2];
                ws += w;
            }
            for (int o = 1; o < G; o <<= 1) {                           // every lane of the wave takes part
                hs[0] += __shfl_xor(hs[0], o, 64);
                hs[1] += __shfl_xor(hs[1], o, 64);
                hs[2] += __shfl_xor(hs[2], o, 64);
                ws += __shfl_xor(ws, o, 64);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] = hs[c] + ((unsigned)L - ws) * fill[c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) h[c] = (unsigned)L * fill[c];
        }
        const unsigned w = (unsigned)(min((i + 1) * L, (p + 1) * S) - max(i * L, p * S));
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += w * h[c];
        if ((p + 1) * S >= (i + 1) * L) {                               // the source row ends output row i
            if (j < S && g == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) out[(i * S + j) * 3 + c] = (uint8_t)((acc[c] + LL / 2) / LL);
            }
            ++i;
            const unsigned rem = (unsigned)((p + 1) * S - i * L);       // what of the row reaches into the next: < S <= L
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = rem * h[c];
        }
    }
}

__device__ __forceinline__ bool chip_record_ok(int f, int n, int x0, int y0, int L) {
    return f >= 0 && f < n && L >= 1 && L <= FR_CHIP_MAX_SIDE && x0 >= -CH_LIMIT && x0 <= CH_LIMIT && y0 >= -CH_LIMIT && y0 <= CH_LIMIT;
}

// uniform batch u8 [N,H,W,3]
__global__ __launch_bounds__(256) void face_chips_u8(const uint8_t* __restrict__ frames, int N, int H, int W, ChipArgs a) {
    const int32_t* r = a.chips + (int64_t)blockIdx.x * 4;
    const int f = r[0], x0 = r[1], y0 = r[2], L = r[3];
    const bool ok = chip_record_ok(f, N, x0, y0, L);
    chip_band(ok ? frames + (int64_t)f * H * W * 3 : nullptr, H, W, x0, y0, L, a);
}

// frame table: the sizes live on the device
__global__ __launch_bounds__(256) void face_chips_refs_u8(const fr_frame_ref* __restrict__ refs, int n, ChipArgs a) {
    const int32_t* r = a.chips + (int64_t)blockIdx.x * 4;
    const int f = r[0], x0 = r[1], y0 = r[2], L = r[3];
    const uint8_t* data = nullptr;
    int H = 0, W = 0;
    if (chip_record_ok(f, n, x0, y0, L)) {
        const fr_frame_ref e = refs[f];
        if (e.data && e.H > 0 && e.W > 0 && (int64_t)e.H * e.W * 3 < (1ll << 31)) data = e.data, H = e.H, W = e.W;
    }
    chip_band(data, H, W, x0, y0, L, a);
}

// the checks both entries share
int chips_check(const char* who, int n, int F, int size) {
    FR_REQUIRE(n >= 0 && n <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(F >= 0 && F <= CH_MAX_F, "%s: bad size (0 .. %d chips)", who, CH_MAX_F);
    FR_REQUIRE(size >= 16 && size <= 256, "%s: size %d out of range (16 .. 256)", who, size);
    return FR_OK;
}

dim3 chips_grid(int F, int size) {
    const int BR = (size + 15) >> 4;
    return dim3((unsigned)F, (unsigned)((size + BR - 1) / BR));
}

}  // namespace

extern "C" int fr_face_chips_u8(const uint8_t* frames, int N, int H, int W, const int32_t* chips, int F, int size,
                                uint32_t bgr_fill, uint8_t* out, fr_stream_t stream) {
    if (const int rc = chips_check("fr_face_chips_u8", N, F, size)) return rc;
    FR_REQUIRE(H > 0 && W > 0, "fr_face_chips_u8: bad size (H and W positive)");
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "fr_face_chips_u8: a %d x %d frame is beyond 2 GiB", H, W);
    if (F == 0) return FR_OK;
    FR_REQUIRE(chips && out && (frames || N == 0), "fr_face_chips_u8: null pointer");
    const ChipArgs a{chips, size, bgr_fill, out};
    face_chips_u8<<<chips_grid(F, size), 256, 0, fr_stream(stream)>>>(frames, N, H, W, a);
    FR_CHECK_LAUNCH("face_chips_u8");
    return FR_OK;
}

extern "C" int fr_face_chips_refs_u8(const fr_frame_ref* refs, int nframes, const int32_t* chips, int F, int size,
                                     uint32_t bgr_fill, uint8_t* out, fr_stream_t stream) {
    if (const int rc = chips_check("fr_face_chips_refs_u8", nframes, F, size)) return rc;
    if (F == 0) return FR_OK;
    FR_REQUIRE(chips && out && (refs || nframes == 0), "fr_face_chips_refs_u8: null pointer");
    const ChipArgs a{chips, size, bgr_fill, out};
    face_chips_refs_u8<<<chips_grid(F, size), 256, 0, fr_stream(stream)>>>(refs, nframes, a);
    FR_CHECK_LAUNCH("face_chips_refs_u8");
    return FR_OK;
}
