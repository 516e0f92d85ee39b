// Baseline JPEG decoder: the files of an MJPEG camera or of an enrolment upload cross the link as they arrived and become the
// [H,W,3] BGR frames every other kernel of the library reads, behind the copy (the reference decodes on the CPU inside
// cv2.VideoCapture / cv2.imdecode: infrenceServer.py:573-601, trainingServer.py:219-221).
//
// The pixels are DEFINED by tests/helpers/jpeg_decode_ref.py (include/frhip.h fr_jpeg_decode_refs_u8) and
// reproduced byte for byte, all of it in 32-bit integers; the definition equals libjpeg's decode: T.81 F.2.2 with the file's own
// Huffman tables, coef * q, the "islow" inverse DCT, the "fancy" chroma upsampling, the 16-bit fixed-point colour transform.
// The host parses SOI .. SOS only (jpeg_decode.py) and passes one fr_jpeg_frame per file; four launches do the rest:
//
// jpegd_segments: a workgroup per frame walks the scan bytes once and finds the RSTm markers (0xFF followed by 0xD0 .. 0xD7) and
//   the scan's end (0xFF followed by anything but 0x00 and RSTm); a prefix count places each restart interval's byte range in
//   the workspace.  It also judges the descriptor: a frame the later launches must not touch gets FR_JPEGD_SKIPPED here.
// jpegd_entropy: a workgroup per (restart interval, frame).  Cameras rarely send DRI, and then the whole frame is one interval:
//   the interval is walked in chunks of 256 subsequences of JD_S raw bytes with the self-synchronising scheme of Weissenberger
//   and Schmidt.  Round 0: every lane decodes its subsequence from a guessed state (block 0 of an MCU, coefficient
//   0) and records the state it ends in: bit position, block of the MCU, zigzag index, and the blocks it completed.  Further
//   rounds: a lane takes the end state of the lane before it and decodes again if that changed what it started from; lane 0
//   has the chunk's exact entry state, so lane r is exact after round r at the latest and the loop is bounded by the lanes.  A
//   speculative walk must go on from a wrong state until it falls into step: bits that are no code are skipped one at a time,
//   an index past 63 ends the block.  Write pass: a prefix sum of the block counts gives every lane its first block, and the
//   walk, now strict - a code no table has, a DC category past 11, an index past 63 or a block past the interval's count flag
//   the FRAME - stores the coefficients int16 at [block][natural index], DC as differences.  The chunk's last end state is the
//   next chunk's entry.  Behind the last chunk the same workgroup turns the DC differences into values: a prefix sum per
//   component over the interval's MCUs.  No workgroup waits on another; every loop is bounded by sizes the host passed.
// jpegd_idct: 8 lanes per 8 x 8 block: a lane dequantises and transforms a column, the block turns in LDS, a lane transforms a
//   row and stores its 8 samples into the component's plane in the workspace.
// jpegd_colour: a lane per output pixel reads the planes (chroma through the triangle filter on the component cropped to its
//   real size, or replicated when the component is at most 2 samples wide, as libjpeg does) and writes BGR through the frame
//   table - the destination form fr_yuv420_to_bgr_refs_u8 writes.
// jpegd_colour_oriented: the last launch of fr_jpeg_decode_oriented_refs_u8 in its place: the same pixels, written where each
//   frame's EXIF orientation (1 .. 8, a device word per frame) puts them; 5 .. 8 turn a tile in LDS so that the stores run along
//   destination rows.
// Plain vector loads and stores, LDS atomics only, byte offsets in int64, nothing allocated, nothing synchronised.
#include "common.h"
#include <algorithm>

namespace {

constexpr int JD_S = 32, JD_LANES = 256;                  // bytes of a subsequence (tests/helpers/jpeg_decode_ref.py S, LANES)
constexpr int JD_CHUNK = JD_S * JD_LANES;
constexpr int JD_SLACK = 16;                              // staged behind a chunk: a symbol is at most 27 bits, 5 data bytes
constexpr int JD_HUFF = FR_JPEGD_HUFF_ROW;
constexpr int JD_SCAN_PER_LANE = 16;
constexpr int JD_MAX_SCAN = 1 << 28;                      // bit positions stay in int32

struct Geometry {
    int bpm;            // blocks of an MCU
    int hs, vs;         // luma sampling factors
    int mx, my;         // MCUs across and down
    int mcus, blocks;
};

__device__ __host__ inline Geometry geometry(int H, int W, int sampling) {
    Geometry g;
    g.hs = (sampling == FR_JPEGD_422 || sampling == FR_JPEGD_420) ? 2 : 1;
    g.vs = sampling == FR_JPEGD_420 ? 2 : 1;
    g.bpm = sampling == FR_JPEGD_GRAY ? 1 : 2 + g.hs * g.vs;
    g.mx = (W + 8 * g.hs - 1) / (8 * g.hs);
    g.my = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.mcus = g.mx * g.my;
    g.blocks = g.mcus * g.bpm;
    return g;
}

// component of block j of an MCU
__device__ __forceinline__ int block_comp(const Geometry& g, int j) { return j < g.bpm - 2 || g.bpm == 1 ? 0 : j - (g.bpm - 3); }

__device__ __host__ inline int64_t max_blocks(int H, int W) {
    const int64_t a = 3ll * ((W + 7) / 8) * ((H + 7) / 8), b = 4ll * ((W + 15) / 16) * ((H + 7) / 8),
                  c = 6ll * ((W + 15) / 16) * ((H + 15) / 16);
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// one frame's slot of the workspace: the interval table, the coefficients, the planes
struct Slot {
    int64_t seg_bytes, coef_bytes, plane_bytes;
    __device__ __host__ int64_t total() const { return seg_bytes + coef_bytes + plane_bytes; }
};

__device__ __host__ inline Slot slot_of(int max_H, int max_W, int max_segments) {
    Slot s;
    s.seg_bytes = (12ll * max_segments + 15) / 16 * 16;     // two bounds an interval, then a round count an interval
    s.coef_bytes = max_blocks(max_H, max_W) * 128;
    const int64_t ph = (max_H + 15) / 16 * 16, pw = (max_W + 15) / 16 * 16;
    s.plane_bytes = 3 * ph * pw;
    return s;
}

struct DecodeArgs {
    const uint8_t* stream;
    int64_t stream_bytes;
    const fr_jpeg_frame* frames;
    const int32_t* qtables;
    const int32_t* htables;
    const fr_frame_ref* refs;
    const int32_t* orient;      // EXIF orientation per frame, 1 .. 8; null: all 1
    int32_t* status;
    uint8_t* ws;
    int nq, nh, max_H, max_W, max_segments;
};

__device__ __forceinline__ int32_t* slot_segments(const DecodeArgs& a, int f) {
    return reinterpret_cast<int32_t*>(a.ws + f * slot_of(a.max_H, a.max_W, a.max_segments).total());
}
__device__ __forceinline__ int16_t* slot_coef(const DecodeArgs& a, int f) {
    const Slot s = slot_of(a.max_H, a.max_W, a.max_segments);
    return reinterpret_cast<int16_t*>(a.ws + f * s.total() + s.seg_bytes);
}
__device__ __forceinline__ uint8_t* slot_planes(const DecodeArgs& a, int f) {
    const Slot s = slot_of(a.max_H, a.max_W, a.max_segments);
    return a.ws + f * s.total() + s.seg_bytes + s.coef_bytes;
}

__device__ __forceinline__ int orientation_of(const DecodeArgs& a, int f) { return a.orient ? a.orient[f] : 1; }

__device__ __forceinline__ int intervals_of(const fr_jpeg_frame& d, const Geometry& g) {
    return d.restart > 0 ? (g.mcus + d.restart - 1) / d.restart : 1;
}

// is the entry one the launches may follow?  Every index and range the kernels use is judged here, once.
__device__ bool frame_usable(const DecodeArgs& a, const fr_jpeg_frame& d, const fr_frame_ref& r, int o) {
    if (o < 1 || o > 8) return false;
    if (d.H < 1 || d.W < 1 || d.H > a.max_H || d.W > a.max_W) return false;
    if (d.sampling < FR_JPEGD_444 || d.sampling > FR_JPEGD_GRAY) return false;
    if (d.restart < 0 || d.restart > 65535) return false;
    if (d.scan_off < 0 || d.scan_len < 0 || d.scan_len >= JD_MAX_SCAN || d.scan_off > a.stream_bytes ||
        d.scan_len > a.stream_bytes - d.scan_off)
        return false;
    if (!r.data || r.H != (o > 4 ? d.W : d.H) || r.W != (o > 4 ? d.H : d.W)) return false;   // 5 .. 8 turn the picture: W x H
    const int nc = d.sampling == FR_JPEGD_GRAY ? 1 : 3;
    for (int c = 0; c < nc; ++c)
        if (d.qsel[c] < 0 || d.qsel[c] >= a.nq || d.dcsel[c] < 0 || d.dcsel[c] >= a.nh || d.acsel[c] < 0 || d.acsel[c] >= a.nh)
            return false;
    return intervals_of(d, geometry(d.H, d.W, d.sampling)) <= a.max_segments;
}

// inclusive prefix sum of one int per lane of a 256-lane workgroup; every lane calls it
__device__ __forceinline__ int block_scan(int v, int* scan, int tid) {
    scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < JD_LANES; d <<= 1) {
        const int t = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += t;
        __syncthreads();
    }
    const int out = scan[tid];
    __syncthreads();
    return out;
}

// ---------------------------------------------------------------- segments
__global__ __launch_bounds__(JD_LANES) void jpegd_segments(DecodeArgs a) {
    __shared__ int scan[JD_LANES];
    __shared__ int term, bad;
    const int f = blockIdx.x, tid = threadIdx.x;
    const fr_jpeg_frame d = a.frames[f];
    if (!frame_usable(a, d, a.refs[f], orientation_of(a, f))) {                 // block-uniform
        if (tid == 0) a.status[f] = FR_JPEGD_SKIPPED;
        return;
    }
    const Geometry g = geometry(d.H, d.W, d.sampling);
    const int nseg = intervals_of(d, g), len = d.scan_len;
    const uint8_t* __restrict__ src = a.stream + d.scan_off;
    int32_t* __restrict__ seg = slot_segments(a, f);      // [2 k]: first byte of interval k, [2 k + 1]: the byte behind it
    if (tid == 0) {
        term = len;
        bad = 0;
    }
    __syncthreads();
    int carry = 0;
    constexpr int SPAN = JD_LANES * JD_SCAN_PER_LANE;
    for (int base = 0; base < len; base += SPAN) {        // bounded by scan_len
        const int lo = base + tid * JD_SCAN_PER_LANE, hi = min(lo + JD_SCAN_PER_LANE, len);
        unsigned rst = 0;                                 // bit i: byte lo + i begins an RSTm
        int first_other = len;
        int prev = 0;
        for (int i = lo; i < hi; ++i) {
            const int b = i == lo ? src[i] : prev;
            const int nx = i + 1 < len ? src[i + 1] : 0;  // a trailing 0xFF is data as far as the segments go
            prev = nx;
            if (b != 0xFF || nx == 0) continue;
            if (nx >= 0xD0 && nx <= 0xD7) rst |= 1u << (i - lo);
            else first_other = min(first_other, i);
        }
        if (first_other < len) atomicMin(&term, first_other);
        __syncthreads();
        const int end = term;
        int mine = 0;
        for (int i = 0; i < JD_SCAN_PER_LANE; ++i)
            if ((rst >> i & 1) && lo + i < end) ++mine;
        const int incl = block_scan(mine, scan, tid);
        int k = carry + incl - mine;                      // index of this lane's first marker
        for (int i = 0; i < JD_SCAN_PER_LANE; ++i) {
            if (!(rst >> i & 1) || lo + i >= end) continue;
            if (k + 1 < nseg && src[lo + i + 1] == 0xD0 + (k & 7)) {
                seg[2 * k + 1] = lo + i;
                seg[2 * k + 2] = lo + i + 2;
            } else {
                bad = 1;                                  // one marker too many, or out of order
            }
            ++k;
        }
        carry += scan[JD_LANES - 1];
        __syncthreads();
        if (end < len) break;                             // block-uniform: the scan ended inside this span
    }
    __syncthreads();
    if (tid == 0) {
        seg[0] = 0;
        seg[2 * nseg - 1] = term;
        a.status[f] = (bad || carry != nseg - 1) ? FR_JPEGD_BAD_STREAM : FR_JPEGD_OK;
    }
}

// ---------------------------------------------------------------- entropy
struct Huff {                                             // the six tables of a frame in LDS: component * 2 + (AC)
    uint16_t look[6][512];
    int maxcode[6][18];
    int valoff[6][18];
    uint8_t vals[6][256];
};

struct State {
    int p;              // bit position in the interval's raw bytes (never inside a stuffed 0x00)
    int bz;             // block of the MCU << 8 | zigzag index
};

// The chunk's raw bytes in LDS: stage[1 + i] is byte `base + i` of the interval, stage[0] the byte before `base`; bytes outside
// the interval read 0.
struct Stage {
    const uint8_t* bytes;
    int base, len;      // first staged byte, bytes of the interval
    __device__ __forceinline__ int at(int k) const { return bytes[1 + k - base]; }
    __device__ __forceinline__ bool stuffed(int k) const { return k > 0 && k < len && at(k) == 0 && at(k - 1) == 0xFF; }
    __device__ __forceinline__ int next(int k) const { return stuffed(k + 1) ? k + 2 : k + 1; }
};

// Decodes the symbols that START before bit `limit` (at most `max_symbols` of them) from state `s`; returns the end state and
// adds the blocks completed to `n`.  STORE: the strict write pass; `coef` is the interval's first block, `blk` this lane's
// first, `count` the interval's blocks; a violation sets `*err`.  Mirrors jpeg_decode_ref._walk.
template <bool STORE>
__device__ State walk(const Stage& st, const Huff& hf, const Geometry& g, State s, int limit, int& n, int16_t* __restrict__ coef,
                      int blk, int count, const int* __restrict__ natural, int* err) {
    int k = s.p >> 3, o = s.p & 7, b = s.bz >> 8, z = s.bz & 255;
    n = 0;
    for (int it = 0; it < JD_S * 8 + 64 && k * 8 + o < limit; ++it) {
        // the next 40 data bits from byte k on, and how many of them are real
        unsigned long long acc = 0;
        int avail = 0, j = k;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            acc <<= 8;
            if (j < st.len) {
                acc |= (unsigned)st.at(j);
                avail += 8;
                j = st.next(j);
            }
        }
        avail -= o;
        const unsigned win = (unsigned)(acc >> (24 - o)) & 0xFFFFu;
        const int t = block_comp(g, b) * 2 + (z ? 1 : 0);
        int length = 0, sym = 0;
        const unsigned e = hf.look[t][win >> 7];
        if (e) {
            length = e >> 8;
            sym = e & 255;
        } else {
            for (int l = 10; l <= 16; ++l) {
                const int code = (int)(win >> (16 - l));
                if (code <= hf.maxcode[t][l]) {
                    length = l;
                    sym = hf.vals[t][(hf.valoff[t][l] + code) & 255];
                    break;
                }
            }
        }
        if (length == 0) {
            if (avail < 16) {                             // the padding of the last byte, or a stream that broke off
                k = st.len;
                o = 0;
                break;
            }
            if (STORE) {
                *err = 1;
                break;
            }
            if (++o == 8) {
                o = 0;
                k = st.next(k);
            }
            continue;
        }
        const int run = z ? sym >> 4 : 0;
        int size = z ? sym & 15 : sym;
        if (size > 11 && z == 0) {
            if (STORE) {
                *err = 1;
                break;
            }
            size &= 15;
        }
        const int used = length + size;
        if (used > avail) {
            k = st.len;
            o = 0;
            break;
        }
        int v = 0;
        if (size) {
            v = (int)(acc >> (40 - o - used)) & ((1 << size) - 1);
            if (v < 1 << (size - 1)) v -= (1 << size) - 1;
        }
        o += used;
        while (o >= 8) {                                  // at most 4 bytes
            o -= 8;
            k = st.next(k);
        }
        const bool fits = blk + n < count;
        if (z == 0) {
            if (STORE) {
                if (fits) coef[(int64_t)(blk + n) * 64] = (int16_t)v;
                else *err = 1;
            }
            z = 1;
        } else if (size == 0) {
            if (run == 15) {
                z += 16;
                if (z > 64) {
                    if (STORE) *err = 1;
                    z = 64;
                }
            } else {
                z = 64;
            }
        } else {
            z += run;
            if (z > 63) {
                if (STORE) *err = 1;
                z = 63;
            }
            if (STORE && fits) coef[(int64_t)(blk + n) * 64 + natural[z]] = (int16_t)v;
            ++z;
        }
        if (z == 64) {
            z = 0;
            b = b + 1 == g.bpm ? 0 : b + 1;
            ++n;
        }
        if (STORE && *err) break;
    }
    return State{k * 8 + o, b << 8 | z};
}

__global__ __launch_bounds__(JD_LANES) void jpegd_entropy(DecodeArgs a, const int32_t* __restrict__ natural_g) {
    __shared__ Huff hf;
    __shared__ __attribute__((aligned(16))) uint8_t stage[16 + JD_CHUNK + JD_SLACK];
    __shared__ int end_p[JD_LANES], end_bz[JD_LANES], cnt[JD_LANES], scan[JD_LANES];
    __shared__ int natural[64];
    __shared__ int err;
    const int f = blockIdx.y, sidx = blockIdx.x, tid = threadIdx.x;
    // Another interval's workgroup may flag the frame while this one starts: lane 0 reads the word once for all, so that the
    // whole workgroup takes one way
    __shared__ int frame_status;
    if (tid == 0) frame_status = a.status[f];
    __syncthreads();
    if (frame_status != FR_JPEGD_OK) return;
    const fr_jpeg_frame d = a.frames[f];
    const Geometry g = geometry(d.H, d.W, d.sampling);
    const int nseg = intervals_of(d, g);
    if (sidx >= nseg) return;
    const int32_t* seg = slot_segments(a, f);
    // the interval's bytes, clamped into the scan whatever the table holds
    const int from = min(max(seg[2 * sidx], 0), d.scan_len), to = min(max(seg[2 * sidx + 1], from), d.scan_len);
    const int len = to - from;
    const uint8_t* __restrict__ src = a.stream + d.scan_off + from;
    const int per = d.restart > 0 ? d.restart : g.mcus;
    const int mcus = min(per, g.mcus - sidx * per);       // >= 1: sidx < nseg
    const int count = mcus * g.bpm;
    int16_t* __restrict__ coef = slot_coef(a, f) + (int64_t)sidx * per * g.bpm * 64;

    // tables into LDS, the interval's coefficients to zero
    const int nc = d.sampling == FR_JPEGD_GRAY ? 1 : 3;
    for (int t = 0; t < 2 * nc; ++t) {
        const int32_t* __restrict__ tab = a.htables + (int64_t)((t & 1) ? d.acsel[t >> 1] : d.dcsel[t >> 1]) * JD_HUFF;
        for (int i = tid; i < 512; i += JD_LANES) hf.look[t][i] = (uint16_t)tab[i];
        if (tid < 18) {
            hf.maxcode[t][tid] = tab[512 + tid];
            hf.valoff[t][tid] = tab[530 + tid];
        }
        hf.vals[t][tid] = (uint8_t)tab[548 + tid];
    }
    if (tid < 64) natural[tid] = natural_g[tid] & 63;
    if (tid == 0) err = 0;
    {
        int4v* __restrict__ c4 = reinterpret_cast<int4v*>(coef);                  // 128 bytes a block, the base on 16
        for (int i = tid; i < count * 8; i += JD_LANES) c4[i] = int4v{0, 0, 0, 0};
    }
    __syncthreads();

    const int subs = max((len + JD_S - 1) / JD_S, 1);
    State entry{0, 0};
    int done = 0;                                         // blocks completed by the chunks so far
    bool failed = false;
    int most_rounds = 0;
    for (int c0 = 0; c0 < subs; c0 += JD_LANES) {         // bounded by the interval's length
        const int base = c0 * JD_S;
        for (int i = tid; i < 1 + JD_CHUNK + JD_SLACK; i += JD_LANES) {
            const int k = base - 1 + i;
            stage[i] = (k >= 0 && k < len) ? src[k] : 0;
        }
        __syncthreads();
        const Stage st{stage, base, len};
        const int lanes = min(JD_LANES, subs - c0);       // the subsequences that begin inside the interval
        const bool active = tid < lanes;
        const int limit = min((base + (tid + 1) * JD_S) * 8, len * 8);
        int k0 = base + tid * JD_S;
        if (st.stuffed(k0)) ++k0;
        entry.p = max(entry.p, base * 8);               // it is: every chunk's last lane walks up to its limit
        State start = tid == 0 ? entry : State{k0 * 8, 0};
        int n = 0;
        if (active) {
            const State e = walk<false>(st, hf, g, start, limit, n, nullptr, 0, 0, natural, nullptr);
            end_p[tid] = e.p;
            end_bz[tid] = e.bz;
            cnt[tid] = n;
        } else {
            cnt[tid] = 0;
        }
        int r = 0;
        for (; r < JD_LANES; ++r) {                       // lane r is exact after round r at the latest
            __syncthreads();
            int changed = 0;
            if (active && tid > 0) {
                const State want{end_p[tid - 1], end_bz[tid - 1]};
                if (want.p != start.p || want.bz != start.bz) {
                    start = want;
                    changed = 1;
                }
            }
            if (!__syncthreads_or(changed)) break;
            if (changed) {
                const State e = walk<false>(st, hf, g, start, limit, n, nullptr, 0, 0, natural, nullptr);
                end_p[tid] = e.p;
                end_bz[tid] = e.bz;
                cnt[tid] = n;
            }
        }
        most_rounds = max(most_rounds, r);                // rounds behind round 0 in which a lane decoded again: block-uniform
        __syncthreads();
        // the write pass, from exact states
        const int incl = block_scan(cnt[tid], scan, tid);
        if (active) {
            int n2 = 0;
            walk<true>(st, hf, g, start, limit, n2, coef, done + incl - cnt[tid], count, natural, &err);
        }
        __syncthreads();
        entry = State{end_p[lanes - 1], end_bz[lanes - 1]};
        done += scan[JD_LANES - 1];
        failed = err != 0;
        __syncthreads();
        if (failed) break;                                // block-uniform
    }
    // what the walk needed, for whoever measures it (tools/jpeg_decode_time.py): the most rounds any chunk of this interval took
    if (tid == 0) slot_segments(a, f)[2 * a.max_segments + sidx] = most_rounds;
    if (failed || entry.bz != 0 || done != count) {
        if (tid == 0) a.status[f] = FR_JPEGD_BAD_STREAM;  // every workgroup that stores here stores the same word
        return;
    }
    // DC differences -> values: a prefix sum per component over the interval's MCUs (the stores above are this workgroup's own)
    int carry[3] = {0, 0, 0};
    const int luma = g.bpm == 1 ? 1 : g.bpm - 2;
    for (int m0 = 0; m0 < mcus; m0 += JD_LANES) {
        const int m = m0 + tid;
        int16_t* __restrict__ mc = coef + (int64_t)m * g.bpm * 64;
        int sum[3] = {0, 0, 0};
        if (m < mcus) {
            for (int j = 0; j < luma; ++j) sum[0] += mc[j * 64];
            if (g.bpm > 1) {
                sum[1] = mc[luma * 64];
                sum[2] = mc[(luma + 1) * 64];
            }
        }
        for (int c = 0; c < nc; ++c) {
            const int incl = block_scan(sum[c], scan, tid);
            int run = carry[c] + incl - sum[c];
            if (m < mcus) {
                if (c == 0) {
                    for (int j = 0; j < luma; ++j) {
                        run += mc[j * 64];
                        mc[j * 64] = (int16_t)run;
                    }
                } else {
                    mc[(luma + c - 1) * 64] = (int16_t)(run + sum[c]);
                }
            }
            carry[c] += scan[JD_LANES - 1];
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- IDCT
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of libjpeg's jidctint over d[0..7], descaled by N
template <int N>
__device__ __forceinline__ void idct_pass(int (&d)[8]) {
    int z1 = (d[2] + d[6]) * 4433;
    int tmp2 = z1 - d[6] * 15137, tmp3 = z1 + d[2] * 6270;
    int tmp0 = (d[0] + d[4]) << 13, tmp1 = (d[0] - d[4]) << 13;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
    z1 = tmp0 + tmp3;
    int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    d[0] = descale(tmp10 + tmp3, N);
    d[7] = descale(tmp10 - tmp3, N);
    d[1] = descale(tmp11 + tmp2, N);
    d[6] = descale(tmp11 - tmp2, N);
    d[2] = descale(tmp12 + tmp1, N);
    d[5] = descale(tmp12 - tmp1, N);
    d[3] = descale(tmp13 + tmp0, N);
    d[4] = descale(tmp13 - tmp0, N);
}

// where the planes of a frame lie in its slot: luma, then the two chroma planes; pitches are multiples of 8
struct Planes {
    int pitch[3];
    int64_t off[3];
};
__device__ __forceinline__ Planes planes_of(const Geometry& g) {
    Planes p;
    p.pitch[0] = g.mx * g.hs * 8;
    p.pitch[1] = p.pitch[2] = g.mx * 8;
    p.off[0] = 0;
    p.off[1] = (int64_t)p.pitch[0] * g.my * g.vs * 8;
    p.off[2] = p.off[1] + (int64_t)p.pitch[1] * g.my * 8;
    return p;
}

__global__ __launch_bounds__(JD_LANES) void jpegd_idct(DecodeArgs a) {
    __shared__ int turn[32][8][9];
    const int f = blockIdx.y, tid = threadIdx.x;
    if (a.status[f] != FR_JPEGD_OK) return;               // block-uniform
    const fr_jpeg_frame d = a.frames[f];
    const Geometry g = geometry(d.H, d.W, d.sampling);
    const int local = tid >> 3, line = tid & 7;
    const int blk = blockIdx.x * 32 + local;
    const bool real = blk < g.blocks;
    const int m = real ? blk / g.bpm : 0, j = real ? blk - m * g.bpm : 0;
    const int comp = block_comp(g, j);
    int v[8];
    if (real) {
        const int16_t* __restrict__ c = slot_coef(a, f) + (int64_t)blk * 64;
        const int32_t* __restrict__ q = a.qtables + (int64_t)a.frames[f].qsel[comp] * 64;
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = (int)c[r * 8 + line] * q[r * 8 + line];
        idct_pass<11>(v);
#pragma unroll
        for (int r = 0; r < 8; ++r) turn[local][r][line] = v[r];
    }
    __syncthreads();
    if (!real) return;
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = turn[local][line][c];
    idct_pass<18>(v);
    unsigned w[2] = {0, 0};
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c >> 2] |= (unsigned)min(max(v[c] + 128, 0), 255) << (8 * (c & 3));
    const Planes p = planes_of(g);
    const int mxi = m % g.mx, myi = m / g.mx;
    int bx = mxi, by = myi;
    if (comp == 0) {
        bx = mxi * g.hs + (j % g.hs);
        by = myi * g.vs + (j / g.hs);
    }
    uint8_t* __restrict__ out = slot_planes(a, f) + p.off[comp] + (int64_t)(by * 8 + line) * p.pitch[comp] + bx * 8;
    *reinterpret_cast<int2v*>(out) = int2v{(int)w[0], (int)w[1]};
}

// ---------------------------------------------------------------- upsample + colour
// pixel (y, x) of a frame from its planes `pl`: B | G << 8 | R << 16
__device__ __forceinline__ unsigned pixel_bgr(const fr_jpeg_frame& d, const Geometry& g, const Planes& p, const uint8_t* __restrict__ pl,
                                              int y, int x) {
    const int Y = pl[p.off[0] + (int64_t)y * p.pitch[0] + x];
    if (d.sampling == FR_JPEGD_GRAY) return (unsigned)Y * 0x010101u;
    int ch[2];
    const int cw = (d.W + g.hs - 1) / g.hs, chh = (d.H + g.vs - 1) / g.vs;       // the chroma component's real size
    const int cx = x / g.hs, cy = y / g.vs;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint8_t* __restrict__ q = pl + p.off[1 + c];
        const int pitch = p.pitch[1 + c];
        if (g.hs == 1 || cw <= 2) {                       // 4:4:4, or libjpeg's plain replication for a narrow component
            ch[c] = q[(int64_t)cy * pitch + cx];
        } else {
            const int nx = (x & 1) ? min(cx + 1, cw - 1) : max(cx - 1, 0);
            const uint8_t* __restrict__ near = q + (int64_t)cy * pitch;
            if (g.vs == 1) {
                ch[c] = (3 * near[cx] + near[nx] + ((x & 1) ? 2 : 1)) >> 2;
            } else {
                const int fy = (y & 1) ? min(cy + 1, chh - 1) : max(cy - 1, 0);
                const uint8_t* __restrict__ far = q + (int64_t)fy * pitch;
                const int s0 = 3 * near[cx] + far[cx], s1 = 3 * near[nx] + far[nx];
                ch[c] = (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
            }
        }
    }
    const int cb = ch[0] - 128, cr = ch[1] - 128;
    const int r = Y + ((91881 * cr + 32768) >> 16);
    const int gg = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    const int b = Y + ((116130 * cb + 32768) >> 16);
    return (unsigned)min(max(b, 0), 255) | (unsigned)min(max(gg, 0), 255) << 8 | (unsigned)min(max(r, 0), 255) << 16;
}

__device__ __forceinline__ void store_bgr(uint8_t* __restrict__ out, unsigned v) {
    out[0] = (uint8_t)v;
    out[1] = (uint8_t)(v >> 8);
    out[2] = (uint8_t)(v >> 16);
}

__global__ __launch_bounds__(JD_LANES) void jpegd_colour(DecodeArgs a) {
    const int f = blockIdx.y;
    if (a.status[f] != FR_JPEGD_OK) return;
    const fr_jpeg_frame d = a.frames[f];
    const int64_t idx = (int64_t)blockIdx.x * JD_LANES + threadIdx.x;
    if (idx >= (int64_t)d.H * d.W) return;
    const int y = (int)(idx / d.W), x = (int)(idx - (int64_t)y * d.W);
    const Geometry g = geometry(d.H, d.W, d.sampling);
    store_bgr(const_cast<uint8_t*>(a.refs[f].data) + idx * 3, pixel_bgr(d, g, planes_of(g), slot_planes(a, f), y, x));
}

// The same pixels written where the EXIF orientation puts them (tests/helpers/orient_ref.py): 2 .. 4 mirror, 5 .. 8 also swap
// rows and columns, and the destination is W x H.  A workgroup takes a JD_TILE x JD_TILE tile of the SOURCE and reads the planes
// along source rows.  For 1 .. 4 a source row is a destination row and the lanes store at once.  For 5 .. 8 the tile's pixels
// wait in LDS, one word each, and are read back turned, so that consecutive lanes store along a DESTINATION row: a run of up to
// 3 JD_TILE bytes, where a lane per source pixel would scatter 3-byte stores a destination row apart.  The pitch of JD_TILE + 1
// words keeps both the row-wise ds_write_b32 and the column-wise ds_read_b32 of a 32-lane group on 32 different banks.
constexpr int JD_TILE = 32;

__global__ __launch_bounds__(JD_LANES) void jpegd_colour_oriented(DecodeArgs a) {
    __shared__ unsigned tile[JD_TILE * (JD_TILE + 1)];
    const int f = blockIdx.y;
    if (a.status[f] != FR_JPEGD_OK) return;               // block-uniform, as is every branch on `o` below
    const fr_jpeg_frame d = a.frames[f];
    const int tiles_x = (d.W + JD_TILE - 1) / JD_TILE, tiles_y = (d.H + JD_TILE - 1) / JD_TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    if (ty >= tiles_y) return;
    const int o = orientation_of(a, f);                   // 1 .. 8: the segments launch judged it
    const bool turn = o > 4, flip_x = o == 2 || o == 3 || o == 7 || o == 8, flip_y = o == 3 || o == 4 || o == 6 || o == 7;
    const Geometry g = geometry(d.H, d.W, d.sampling);
    const Planes p = planes_of(g);
    const uint8_t* __restrict__ pl = slot_planes(a, f);
    uint8_t* __restrict__ out = const_cast<uint8_t*>(a.refs[f].data);
    const int x0 = tx * JD_TILE, y0 = ty * JD_TILE;
    const int lx = threadIdx.x % JD_TILE, ly = threadIdx.x / JD_TILE;
#pragma unroll
    for (int r = ly; r < JD_TILE; r += JD_LANES / JD_TILE) {
        const int y = y0 + r, x = x0 + lx;
        if (y >= d.H || x >= d.W) continue;
        const unsigned v = pixel_bgr(d, g, p, pl, y, x);
        if (turn) tile[r * (JD_TILE + 1) + lx] = v;
        else store_bgr(out + ((int64_t)(flip_y ? d.H - 1 - y : y) * d.W + (flip_x ? d.W - 1 - x : x)) * 3, v);
    }
    if (!turn) return;
    __syncthreads();
    // destination row <- source column x0 + c, destination column <- source row y0 + lx
#pragma unroll
    for (int c = ly; c < JD_TILE; c += JD_LANES / JD_TILE) {
        const int y = y0 + lx, x = x0 + c;
        if (y >= d.H || x >= d.W) continue;
        store_bgr(out + ((int64_t)(flip_x ? d.W - 1 - x : x) * d.H + (flip_y ? d.H - 1 - y : y)) * 3, tile[lx * (JD_TILE + 1) + c]);
    }
}

typedef int4v int4v_any __attribute__((aligned(1)));               // 16-byte store at any byte address

// A frame the decoder flagged keeps what its destination held - in a ring, the picture of some turns ago.  This zeroes the
// destination of every frame whose status is FR_JPEGD_BAD_STREAM: a black frame, a frame without faces.
__global__ __launch_bounds__(JD_LANES) void jpegd_blank(const fr_frame_ref* __restrict__ refs, const int32_t* __restrict__ status) {
    const int f = blockIdx.y;
    if (status[f] != FR_JPEGD_BAD_STREAM) return;
    const fr_frame_ref r = refs[f];
    if (!r.data || r.H < 1 || r.W < 1 || (int64_t)r.H * r.W * 3 >= (1ll << 31)) return;
    uint8_t* __restrict__ out = const_cast<uint8_t*>(r.data);
    const int bytes = r.H * r.W * 3, whole = bytes / 16;
    for (int i = blockIdx.x * JD_LANES + threadIdx.x; i < whole; i += gridDim.x * JD_LANES)
        *reinterpret_cast<int4v_any*>(out + (int64_t)i * 16) = int4v{0, 0, 0, 0};
    if (blockIdx.x == 0 && (int)threadIdx.x < bytes - whole * 16) out[whole * 16 + threadIdx.x] = 0;
}

bool sizes_ok(int n, int max_H, int max_W, int max_segments) {
    return n >= 0 && n <= 65535 && max_H >= 1 && max_H <= 65535 && max_W >= 1 && max_W <= 65535 && max_segments >= 1 &&
           max_segments <= (1 << 24) && (int64_t)max_H * max_W * 3 < (1ll << 31);
}

}  // namespace

extern "C" size_t fr_jpeg_decode_workspace(int N, int max_H, int max_W, int max_segments) {
    if (!sizes_ok(N, max_H, max_W, max_segments)) return 0;
    return (size_t)N * (size_t)slot_of(max_H, max_W, max_segments).total();
}

namespace {

int decode_refs(const char* who, const uint8_t* data, int64_t data_bytes, const fr_jpeg_frame* frames, int nframes, int max_H,
                int max_W, int max_segments, const int32_t* qtables, int nq, const int32_t* htables, int nh, const int32_t* natural,
                const fr_frame_ref* refs, const int32_t* orient, int32_t* status, void* workspace, size_t workspace_bytes,
                fr_stream_t stream) {
    FR_REQUIRE(nframes >= 0 && nframes <= 65535, "%s: bad size (0 .. 65535 frames)", who);
    FR_REQUIRE(max_H >= 1 && max_H <= 65535 && max_W >= 1 && max_W <= 65535, "%s: bad size (max_H and max_W 1 .. 65535)", who);
    FR_REQUIRE((int64_t)max_H * max_W * 3 < (1ll << 31), "%s: a %d x %d frame is beyond 2 GiB", who, max_H, max_W);
    FR_REQUIRE(max_segments >= 1 && max_segments <= (1 << 24), "%s: max_segments %d out of range (1 .. 2^24)", who, max_segments);
    FR_REQUIRE(data_bytes >= 0, "%s: negative data_bytes", who);
    FR_REQUIRE(nq >= 1 && nq <= 65535 && nh >= 1 && nh <= 65535, "%s: bad table count (nq and nh 1 .. 65535)", who);
    if (nframes == 0) return FR_OK;
    const size_t need = fr_jpeg_decode_workspace(nframes, max_H, max_W, max_segments);
    FR_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu bytes, %zu needed)", who, workspace_bytes, need);
    FR_REQUIRE(data && frames && qtables && htables && natural && refs && status && workspace, "%s: null pointer", who);
    FR_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: workspace not on a 16-byte boundary", who);
    const DecodeArgs a{data, data_bytes, frames, qtables, htables, refs, orient, status, static_cast<uint8_t*>(workspace),
                       nq,   nh,         max_H,  max_W,   max_segments};
    hipStream_t s = fr_stream(stream);
    jpegd_segments<<<(unsigned)nframes, JD_LANES, 0, s>>>(a);
    FR_CHECK_LAUNCH("jpegd_segments");
    jpegd_entropy<<<dim3((unsigned)max_segments, (unsigned)nframes), JD_LANES, 0, s>>>(a, natural);
    FR_CHECK_LAUNCH("jpegd_entropy");
    const int64_t blocks = max_blocks(max_H, max_W);
    jpegd_idct<<<dim3((unsigned)((blocks + 31) / 32), (unsigned)nframes), JD_LANES, 0, s>>>(a);
    FR_CHECK_LAUNCH("jpegd_idct");
    if (orient) {                                         // tiles of the coded geometry
        const int64_t tiles = (int64_t)((max_H + JD_TILE - 1) / JD_TILE) * ((max_W + JD_TILE - 1) / JD_TILE);
        jpegd_colour_oriented<<<dim3((unsigned)tiles, (unsigned)nframes), JD_LANES, 0, s>>>(a);
        FR_CHECK_LAUNCH("jpegd_colour_oriented");
    } else {
        const int64_t px = (int64_t)max_H * max_W;
        jpegd_colour<<<dim3((unsigned)((px + JD_LANES - 1) / JD_LANES), (unsigned)nframes), JD_LANES, 0, s>>>(a);
        FR_CHECK_LAUNCH("jpegd_colour");
    }
    return FR_OK;
}

}  // namespace

extern "C" int fr_jpeg_decode_refs_u8(const uint8_t* data, int64_t data_bytes, const fr_jpeg_frame* frames, int nframes,
                                      int max_H, int max_W, int max_segments, const int32_t* qtables, int nq, const int32_t* htables,
                                      int nh, const int32_t* natural, const fr_frame_ref* refs, int32_t* status, void* workspace,
                                      size_t workspace_bytes, fr_stream_t stream) {
    return decode_refs("fr_jpeg_decode_refs_u8", data, data_bytes, frames, nframes, max_H, max_W, max_segments, qtables, nq, htables,
                       nh, natural, refs, nullptr, status, workspace, workspace_bytes, stream);
}

extern "C" int fr_jpeg_decode_oriented_refs_u8(const uint8_t* data, int64_t data_bytes, const fr_jpeg_frame* frames, int nframes,
                                               int max_H, int max_W, int max_segments, const int32_t* qtables, int nq,
                                               const int32_t* htables, int nh, const int32_t* natural, const fr_frame_ref* refs,
                                               const int32_t* orient, int32_t* status, void* workspace, size_t workspace_bytes,
                                               fr_stream_t stream) {
    return decode_refs("fr_jpeg_decode_oriented_refs_u8", data, data_bytes, frames, nframes, max_H, max_W, max_segments, qtables, nq,
                       htables, nh, natural, refs, orient, status, workspace, workspace_bytes, stream);
}

extern "C" int fr_jpeg_blank_bad_refs_u8(const fr_frame_ref* refs, const int32_t* status, int nframes, fr_stream_t stream) {
    FR_REQUIRE(nframes >= 0 && nframes <= 65535, "fr_jpeg_blank_bad_refs_u8: bad size (0 .. 65535 frames)");
    if (nframes == 0) return FR_OK;
    FR_REQUIRE(refs && status, "fr_jpeg_blank_bad_refs_u8: null pointer");
    jpegd_blank<<<dim3(64, (unsigned)nframes), JD_LANES, 0, fr_stream(stream)>>>(refs, status);
    FR_CHECK_LAUNCH("jpegd_blank");
    return FR_OK;
}
