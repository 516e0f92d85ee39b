// Baseline JPEG encoder for the BGR frames of the live path, behind the HUD draw (hud_draw.hip): what crosses the link is then
// a JPEG file per frame, a few hundred KB at 1080p instead of 6.2 MB.  (The reference shows raw frames with cv2.imshow, one
// process per camera: infrenceServer.py:648-667.)
//
// The bytes are DEFINED by tests/helpers/jpeg_ref.py (include/frhip.h fr_jpeg_encode_u8) and reproduced byte for
// byte, all of it in 32-bit integers: JFIF full-range YCbCr in libjpeg's 16-bit fixed point, edges replicated to multiples of
// 16, 4:2:0 chroma (a + b + c + d + 2) >> 2, MCUs of 16 x 16 (Y00 Y01 Y10 Y11 Cb Cr), libjpeg's "islow" forward DCT of
// samples - 128, the quantiser sign(c) ((|c| + (qv >> 1)) / qv), the Huffman coding of T.81 F.1.2 with the Annex K tables and ONE
// restart interval per MCU row - which is what makes the rows independent: the DC predictions start at 0 and the bits at a
// byte boundary in every row.
//
// jpeg_rows: one workgroup of 256 per (frame, MCU row) walks the row's MCUs in order and carries the bit position.  Per MCU:
//   1. a lane per pixel: load (coordinates clamped to the frame: the replicated edge), convert, Y - 128 into its block in LDS;
//      the 2 x 2 chroma sums are two __shfl_xor (lanes ^ 1 and ^ 16 are the pixel's neighbours inside one wave)
//   2. 48 lanes: the row pass of the six blocks, then 48 lanes: the column pass, quantised and stored at the zigzag position
//   3. a wave per block, lane = zigzag index: the __ballot of non-zero lanes gives each lane its zero run (distance to the set
//      bit below it) and the lane behind the highest set bit emits EOB; a lane's bits - up to 3 ZRL + an AC code + 10 magnitude
//      bits, 59 at most - sit in one 64-bit value; a wave prefix sum of the lengths places them, LDS atomic OR writes them into
//      the bit buffer (big-endian 32-bit words).  DC differences chain through the quantised DC values, not the bit stream.
//   4. when the buffer could not take another MCU (or the row ends, padded with 1-bits): whole bytes are flushed to the row's
//      segment in the workspace, a 0x00 behind every 0xFF, at positions from a block prefix count of 0xFF bytes; every store
//      is bounded by the segment's budget.  The bits of the last partial byte move to the front of the cleared buffer.
// jpeg_assemble: per frame the total of its rows, a prefix sum across the frames, the header with H / W / DRI patched, the rows
// back to back with RSTm between them, EOI.  A frame with a row past its budget, or one that would end past the capacity of
// `out`, has length 0 and a flag.  No global atomics, plain vector loads and stores, byte offsets in int64.
#include "common.h"
#include <algorithm>

namespace {

constexpr int JP_BUF_WORDS = 1024, JP_BUF_BITS = JP_BUF_WORDS * 32;
constexpr int JP_MCU_BITS = 6 * (20 + 63 * 26);       // no MCU codes to more: a DC code + 11 bits, 63 x (a 16-bit code + 10 bits)
constexpr int JP_FLUSH_AT = JP_BUF_BITS - JP_MCU_BITS - 128;
constexpr int JP_HDR = FR_JPEG_HEADER_BYTES, JP_ROW = FR_JPEG_CODE_ROW;
constexpr int JP_MAX_ROWS = 4096;                     // MCU rows of a frame 65535 high
constexpr int JP_COPY_BLOCKS = 32;                    // blocks that share the copy of one frame's rows

struct JpegArgs {
    const uint32_t* codes;
    const int32_t* qt;
    uint8_t* seg;            // [N][rows][row_budget]
    int32_t* row_len;        // [N][rows]: bytes of the row, -1 when it did not fit
    int rows, row_budget;    // rows: MCU rows per frame slot (those of the largest frame)
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of libjpeg's jfdctint over d[0..7]
template <bool FIRST>
__device__ __forceinline__ void fdct_pass(int (&d)[8]) {
    constexpr int N = FIRST ? 11 : 15;                // CONST_BITS -+ PASS1_BITS
    int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) << 2;
        d[4] = (tmp10 - tmp11) << 2;
    } else {
        d[0] = descale(tmp10 + tmp11, 2);
        d[4] = descale(tmp10 - tmp11, 2);
    }
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, N);
    d[6] = descale(z1 - tmp12 * 15137, N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    tmp4 *= 2446; tmp5 *= 16819; tmp6 *= 25172; tmp7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7] = descale(tmp4 + z1 + z3, N);
    d[5] = descale(tmp5 + z2 + z4, N);
    d[3] = descale(tmp6 + z2 + z3, N);
    d[1] = descale(tmp7 + z1 + z4, N);
}

// magnitude category and the bits behind the code (one's complement for negatives), T.81 F.1.2.1
__device__ __forceinline__ void magnitude(int v, int& size, uint32_t& bits) {
    size = 32 - __clz(abs(v));
    bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);
}

// the bits one lane contributes to its block: lane = zigzag index, v its quantised coefficient, pred the DC prediction
__device__ __forceinline__ void lane_code(const uint32_t* __restrict__ ct, int lane, int v, int pred, unsigned long long& val, int& len) {
    const unsigned long long ac = __ballot(v != 0) & ~1ull;
    val = 0;
    len = 0;
    if (lane == 0) {
        int size;
        uint32_t bits;
        magnitude(v - pred, size, bits);
        const uint32_t e = ct[256 + min(size, 15)];
        val = ((unsigned long long)(e >> 8) << size) | bits;
        len = (int)(e & 255u) + size;
    } else if (v != 0) {
        const unsigned long long below = (ac | 1ull) & ((1ull << lane) - 1ull);
        const int run = lane - 1 - (63 - __clzll(below));
        int size;
        uint32_t bits;
        magnitude(v, size, bits);
        const uint32_t zrl = ct[0xF0], e = ct[((run & 15) << 4) | min(size, 15)];
        for (int i = 0; i < (run >> 4); ++i) {
            val = (val << (zrl & 255u)) | (zrl >> 8);
            len += (int)(zrl & 255u);
        }
        val = (((val << (e & 255u)) | (e >> 8)) << size) | bits;
        len += (int)(e & 255u) + size;
    } else {
        const int last = ac ? 63 - __clzll(ac) : 0;
        if (lane == last + 1) {                                  // the block ends in zeros: EOB
            val = ct[0] >> 8;
            len = (int)(ct[0] & 255u);
        }
    }
}

// ORs the len (1 .. 59) low bits of val into the bit buffer at bit position p (bit 0 = the MSB of byte 0)
__device__ __forceinline__ void put_bits(uint32_t* buf, int p, unsigned long long val, int len) {
    const int w = p >> 5, t = 64 - (p & 31) - len;               // t in -26 .. 63
    const unsigned long long x = t >= 0 ? val << t : val >> (-t);
    const uint32_t w0 = (uint32_t)(x >> 32), w1 = (uint32_t)x, w2 = t < 0 ? (uint32_t)(val << (32 + t)) : 0u;
    if (w0 && w < JP_BUF_WORDS) atomicOr(buf + w, w0);
    if (w1 && w + 1 < JP_BUF_WORDS) atomicOr(buf + w + 1, w1);
    if (w2 && w + 2 < JP_BUF_WORDS) atomicOr(buf + w + 2, w2);
}

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// MCU row `my` of ONE frame of H x W at `data` (H, W in 1 .. 65535, H*W*3 < 2^31: the callers see to it) into segment `slot`
__device__ __forceinline__ void jpeg_row(const uint8_t* __restrict__ data, int H, int W, int64_t slot, int my, const JpegArgs a) {
    __shared__ int blk[6 * 64];                      // samples - 128, then the row pass's output
    __shared__ int q[6 * 64];                        // quantised, zigzag order
    __shared__ uint32_t codes[2 * JP_ROW];
    __shared__ int qt[3 * 64];
    __shared__ uint32_t bitbuf[JP_BUF_WORDS];
    __shared__ int blk_bits[6];
    __shared__ int wave_ff[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 2 * JP_ROW; i += 256) codes[i] = a.codes[i];
    if (tid < 3 * 64) qt[tid] = a.qt[tid];
    for (int i = tid; i < JP_BUF_WORDS; i += 256) bitbuf[i] = 0u;
    __syncthreads();
    uint8_t* __restrict__ seg = a.seg + slot * a.row_budget;
    const int budget = a.row_budget;
    const int mw = (W + 15) >> 4;
    const int ly = tid >> 4, lx = tid & 15;
    const int py = min(my * 16 + ly, H - 1);
    int nbits = 0;                                   // bits in the buffer
    int64_t outpos = 0;                              // bytes of the row so far, stuffing included (may pass the budget)
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    for (int mx = 0; mx < mw; ++mx) {
        {   // 1. pixels -> Y / Cb / Cr
            const int px = min(mx * 16 + lx, W - 1);
            const uint8_t* __restrict__ p = data + ((int64_t)py * W + px) * 3;
            const int B = p[0], G = p[1], R = p[2];
            const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            int cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            int cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            blk[((ly >> 3) * 2 + (lx >> 3)) * 64 + (ly & 7) * 8 + (lx & 7)] = Y - 128;
            cb += __shfl_xor(cb, 1, 64);
            cr += __shfl_xor(cr, 1, 64);
            cb += __shfl_xor(cb, 16, 64);
            cr += __shfl_xor(cr, 16, 64);
            if (!((lx | ly) & 1)) {
                blk[4 * 64 + (ly >> 1) * 8 + (lx >> 1)] = ((cb + 2) >> 2) - 128;
                blk[5 * 64 + (ly >> 1) * 8 + (lx >> 1)] = ((cr + 2) >> 2) - 128;
            }
        }
        __syncthreads();
        if (tid < 48) {                              // 2. rows
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = blk[tid * 8 + k];
            fdct_pass<true>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) blk[tid * 8 + k] = d[k];
        }
        __syncthreads();
        if (tid < 48) {                              // columns, quantiser
            const int b = tid >> 3, c = tid & 7;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = blk[b * 64 + k * 8 + c];
            fdct_pass<false>(d);
            const int* __restrict__ t = qt + (b < 4 ? 0 : 64);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int n = k * 8 + c;
                const unsigned qv = (unsigned)t[n] << 3;
                const int mag = (int)(((unsigned)abs(d[k]) + (qv >> 1)) / qv);
                q[b * 64 + qt[128 + n]] = d[k] < 0 ? -mag : mag;
            }
        }
        __syncthreads();
        // 3. a wave per block: waves 0 .. 3 the Y blocks, then waves 0 and 1 Cb and Cr
        unsigned long long val0, val1 = 0;
        int len0, len1 = 0, at0, at1 = 0;
        {
            const int pred = wave == 0 ? pred_y : q[(wave - 1) * 64];
            lane_code(codes, lane, q[wave * 64 + lane], pred, val0, len0);
            const int s = wave_scan_incl(len0, lane);
            at0 = s - len0;
            if (lane == 63) blk_bits[wave] = s;
        }
        if (wave < 2) {                              // wave-uniform
            lane_code(codes + JP_ROW, lane, q[(4 + wave) * 64 + lane], wave == 0 ? pred_cb : pred_cr, val1, len1);
            const int s = wave_scan_incl(len1, lane);
            at1 = s - len1;
            if (lane == 63) blk_bits[4 + wave] = s;
        }
        __syncthreads();
        {
            int base = nbits;
            for (int b = 0; b < wave; ++b) base += blk_bits[b];
            if (len0) put_bits(bitbuf, base + at0, val0, len0);
            int all = 0;
#pragma unroll
            for (int b = 0; b < 6; ++b) all += blk_bits[b];
            if (wave < 2 && len1) {
                int base1 = nbits;
                for (int b = 0; b < 4 + wave; ++b) base1 += blk_bits[b];
                put_bits(bitbuf, base1 + at1, val1, len1);
            }
            nbits += all;
        }
        pred_y = q[3 * 64];
        pred_cb = q[4 * 64];
        pred_cr = q[5 * 64];
        const bool last = mx == mw - 1;
        if (last && (nbits & 7)) {                   // the row's last byte is padded with 1-bits
            const int pad = 8 - (nbits & 7);
            if (tid == 0) put_bits(bitbuf, nbits, (1ull << pad) - 1ull, pad);
            nbits += pad;
        }
        if (!last && nbits <= JP_FLUSH_AT) continue;             // block-uniform
        __syncthreads();
        // 4. flush the whole bytes: a contiguous run per lane, a 0x00 behind every 0xFF
        const int nbytes = min(nbits >> 3, JP_BUF_WORDS * 4 - 1), per = (nbytes + 255) >> 8;      // the bound is never met
        const int first = min(tid * per, nbytes), end = min(first + per, nbytes);
        int ff = 0;
        for (int i = first; i < end; ++i) ff += ((bitbuf[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
        const int incl = wave_scan_incl(ff, lane);
        if (lane == 63) wave_ff[wave] = incl;
        const uint32_t partial = (nbits & 7) ? (bitbuf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u : 0u;
        __syncthreads();
        int before = incl - ff, total_ff = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_ff[w];
            total_ff += wave_ff[w];
        }
        int64_t pos = outpos + first + before;
        for (int i = first; i < end; ++i) {
            const uint32_t byte = (bitbuf[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
            if (pos < budget) seg[pos] = (uint8_t)byte;
            ++pos;
            if (byte == 255u) {
                if (pos < budget) seg[pos] = 0;
                ++pos;
            }
        }
        outpos += nbytes + total_ff;
        nbits &= 7;
        __syncthreads();
        for (int i = tid; i < JP_BUF_WORDS; i += 256) bitbuf[i] = i == 0 ? partial << 24 : 0u;
        __syncthreads();
    }
    if (tid == 0) a.row_len[slot] = outpos <= budget ? (int32_t)outpos : -1;
}

// may frame (data, H, W) be encoded into a slot made for max_H x max_W?
__device__ __forceinline__ bool frame_ok(const uint8_t* data, int H, int W, int max_H, int max_W) {
    return data && H > 0 && W > 0 && H <= max_H && W <= max_W && (int64_t)H * W * 3 < (1ll << 31);
}

// uniform batch u8 [N,H,W,3]: blockIdx.x the MCU row, blockIdx.y the frame
__global__ __launch_bounds__(256) void jpeg_rows_u8(const uint8_t* __restrict__ frames, int H, int W, JpegArgs a) {
    jpeg_row(frames + (int64_t)blockIdx.y * H * W * 3, H, W, (int64_t)blockIdx.y * a.rows + blockIdx.x, (int)blockIdx.x, a);
}

// frame table: the sizes live on the device, the grid has the rows of the largest frame
__global__ __launch_bounds__(256) void jpeg_rows_refs_u8(const fr_frame_ref* __restrict__ refs, int max_H, int max_W, JpegArgs a) {
    const fr_frame_ref r = refs[blockIdx.y];
    if (!frame_ok(r.data, r.H, r.W, max_H, max_W) || (int)blockIdx.x >= (r.H + 15) >> 4) return;      // block-uniform
    jpeg_row(r.data, r.H, r.W, (int64_t)blockIdx.y * a.rows + blockIdx.x, (int)blockIdx.x, a);
}

// bytes of frame g's file (0: it has none) and its status
template <bool REFS>
__device__ __forceinline__ int64_t frame_bytes(const fr_frame_ref* __restrict__ refs, int H, int W, int g, const JpegArgs a, int& status) {
    int h = H;
    if (REFS) {
        const fr_frame_ref r = refs[g];
        if (!frame_ok(r.data, r.H, r.W, H, W)) {
            status = FR_JPEG_SKIPPED;
            return 0;
        }
        h = r.H;
    }
    const int mh = (h + 15) >> 4;
    const int32_t* __restrict__ rl = a.row_len + (int64_t)g * a.rows;
    int64_t sum = 0;
    bool fits = true;
    for (int r = 0; r < mh; ++r) {
        const int l = rl[r];
        fits &= l >= 0;
        sum += l;
    }
    status = fits ? FR_JPEG_OK : FR_JPEG_OVERFLOW;
    return fits ? JP_HDR + sum + 2 * (mh - 1) + 2 : 0;
}

// blockIdx.y the frame; the gridDim.x blocks of a frame share the copy of its rows.  Every block sums the frames up to its own.
template <bool REFS>
__global__ __launch_bounds__(256) void jpeg_assemble(const fr_frame_ref* __restrict__ refs, int N, int H, int W,
                                                     const uint8_t* __restrict__ header, uint8_t* __restrict__ out, int64_t capacity,
                                                     int64_t* __restrict__ offsets, int32_t* __restrict__ status, JpegArgs a) {
    __shared__ int64_t scan[256];
    __shared__ int64_t mine[2];                      // start and length of this block's frame
    __shared__ unsigned long long fit_end;           // end of the last frame that ends inside the capacity
    __shared__ int my_status;
    __shared__ int rl[JP_MAX_ROWS];
    const int tid = threadIdx.x, f = blockIdx.y;
    if (tid == 0) fit_end = 0ull;
    __syncthreads();
    int64_t carry = 0;
    for (int g0 = 0; g0 <= f; g0 += 256) {           // block-uniform
        const int g = g0 + tid;
        int st = FR_JPEG_OK;
        const int64_t len = g <= f ? frame_bytes<REFS>(refs, H, W, g, a, st) : 0;
        scan[tid] = len;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int64_t t = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += t;
            __syncthreads();
        }
        const int64_t incl = carry + scan[tid];
        if (g <= f && incl <= capacity) atomicMax(&fit_end, (unsigned long long)incl);
        if (g == f) {
            mine[0] = incl - len;
            mine[1] = len;
            my_status = st;
        }
        carry += scan[255];
        __syncthreads();
    }
    const int64_t start = mine[0], len = mine[1];
    const bool fits = start + len <= capacity;
    if (blockIdx.x == 0 && tid == 0) {
        offsets[f] = fits ? start : (int64_t)fit_end;
        if (f == N - 1) offsets[N] = fits ? start + len : (int64_t)fit_end;
        status[f] = fits ? my_status : (my_status == FR_JPEG_SKIPPED ? FR_JPEG_SKIPPED : FR_JPEG_OVERFLOW);
    }
    if (!fits || len == 0) return;                   // block-uniform
    int h = H, w = W;
    if (REFS) {
        h = refs[f].H;
        w = refs[f].W;
    }
    const int mh = (h + 15) >> 4, mw = (w + 15) >> 4;
    for (int r = tid; r < mh; r += 256) rl[r] = a.row_len[(int64_t)f * a.rows + r];
    __syncthreads();
    uint8_t* __restrict__ dst = out + start;
    if (blockIdx.x == 0) {
        for (int i = tid; i < JP_HDR; i += 256) {
            int b = header[i];
            if (i == FR_JPEG_AT_H) b = h >> 8;
            if (i == FR_JPEG_AT_H + 1) b = h & 255;
            if (i == FR_JPEG_AT_W) b = w >> 8;
            if (i == FR_JPEG_AT_W + 1) b = w & 255;
            if (i == FR_JPEG_AT_DRI) b = mw >> 8;
            if (i == FR_JPEG_AT_DRI + 1) b = mw & 255;
            dst[i] = (uint8_t)b;
        }
        if (tid == 0) {
            dst[len - 2] = 0xFF;
            dst[len - 1] = 0xD9;
        }
    }
    int64_t pos = JP_HDR;
    for (int r = 0; r < mh; ++r) {
        const int l = rl[r];
        if (r % (int)gridDim.x == (int)blockIdx.x) {
            const uint8_t* __restrict__ src = a.seg + ((int64_t)f * a.rows + r) * a.row_budget;
            for (int i = tid; i < l; i += 256) dst[pos + i] = src[i];
            if (tid == 0 && r + 1 < mh) {
                dst[pos + l] = 0xFF;
                dst[pos + l + 1] = (uint8_t)(0xD0 + (r & 7));
            }
        }
        pos += l + 2;
    }
}

size_t ws_rows_bytes(int64_t slots) { return (size_t)((slots * 4 + 15) / 16 * 16); }

// the checks both entries share; H x W: the frames' size, or the largest a table's frame may have
int jpeg_check(const char* who, int n, int H, int W, int header_len, int row_budget, int64_t capacity, size_t ws_bytes) {
    FR_REQUIRE(n >= 0 && n <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(H >= 1 && H <= 65535 && W >= 1 && W <= 65535, "%s: bad size (H and W 1 .. 65535)", who);
    FR_REQUIRE((int64_t)H * W * 3 < (1ll << 31), "%s: a %d x %d frame is beyond 2 GiB", who, H, W);
    FR_REQUIRE(row_budget >= 1, "%s: row_budget %d out of range (at least 1)", who, row_budget);
    FR_REQUIRE(header_len == JP_HDR, "%s: header of %d bytes (it has %d)", who, header_len, JP_HDR);
    FR_REQUIRE(capacity >= 0, "%s: negative out_capacity", who);
    FR_REQUIRE(n == 0 || ws_bytes >= fr_jpeg_workspace(n, H, W, row_budget), "%s: workspace too small (%zu bytes, %zu needed)", who,
               ws_bytes, fr_jpeg_workspace(n, H, W, row_budget));
    return FR_OK;
}

}  // namespace

extern "C" size_t fr_jpeg_workspace(int N, int H, int W, int row_budget) {
    if (N < 0 || N > 65535 || H < 1 || H > 65535 || W < 1 || W > 65535 || row_budget < 1) return 0;
    const int64_t slots = (int64_t)N * ((H + 15) >> 4);
    return ws_rows_bytes(slots) + (size_t)slots * (size_t)row_budget;
}

extern "C" int fr_jpeg_encode_u8(const uint8_t* frames, int N, int H, int W, const uint8_t* header, int header_len,
                                 const uint32_t* codes, const int32_t* qtables, int row_budget, uint8_t* out, int64_t out_capacity,
                                 int64_t* offsets, int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream) {
    if (const int rc = jpeg_check("fr_jpeg_encode_u8", N, H, W, header_len, row_budget, out_capacity, workspace_bytes)) return rc;
    if (N == 0) return FR_OK;
    FR_REQUIRE(frames && header && codes && qtables && out && offsets && status && workspace, "fr_jpeg_encode_u8: null pointer");
    const int mh = (H + 15) >> 4;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const JpegArgs a{codes, qtables, ws + ws_rows_bytes((int64_t)N * mh), reinterpret_cast<int32_t*>(ws), mh, row_budget};
    jpeg_rows_u8<<<dim3((unsigned)mh, (unsigned)N), 256, 0, fr_stream(stream)>>>(frames, H, W, a);
    FR_CHECK_LAUNCH("jpeg_rows_u8");
    jpeg_assemble<false><<<dim3((unsigned)std::min(mh, JP_COPY_BLOCKS), (unsigned)N), 256, 0, fr_stream(stream)>>>(
        nullptr, N, H, W, header, out, out_capacity, offsets, status, a);
    FR_CHECK_LAUNCH("jpeg_assemble");
    return FR_OK;
}

extern "C" int fr_jpeg_encode_refs_u8(const fr_frame_ref* refs, int nframes, int max_H, int max_W, const uint8_t* header,
                                      int header_len, const uint32_t* codes, const int32_t* qtables, int row_budget, uint8_t* out,
                                      int64_t out_capacity, int64_t* offsets, int32_t* status, void* workspace,
                                      size_t workspace_bytes, fr_stream_t stream) {
    if (const int rc = jpeg_check("fr_jpeg_encode_refs_u8", nframes, max_H, max_W, header_len, row_budget, out_capacity, workspace_bytes))
        return rc;
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(refs && header && codes && qtables && out && offsets && status && workspace, "fr_jpeg_encode_refs_u8: null pointer");
    const int mh = (max_H + 15) >> 4;
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    const JpegArgs a{codes, qtables, ws + ws_rows_bytes((int64_t)nframes * mh), reinterpret_cast<int32_t*>(ws), mh, row_budget};
    jpeg_rows_refs_u8<<<dim3((unsigned)mh, (unsigned)nframes), 256, 0, fr_stream(stream)>>>(refs, max_H, max_W, a);
    FR_CHECK_LAUNCH("jpeg_rows_refs_u8");
    jpeg_assemble<true><<<dim3((unsigned)std::min(mh, JP_COPY_BLOCKS), (unsigned)nframes), 256, 0, fr_stream(stream)>>>(
        refs, nframes, max_H, max_W, header, out, out_capacity, offsets, status, a);
    FR_CHECK_LAUNCH("jpeg_assemble");
    return FR_OK;
}
