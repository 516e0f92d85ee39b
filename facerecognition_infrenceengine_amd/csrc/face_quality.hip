// Face quality: is an aligned face worth the embed net?  (The reference embeds every detected face, infrenceServer.py:528-532;
// its only guard is the silent [0.35, 0.45) drop band of the counting path.)  The crops are the f16 [S,112,112,8] faces that
// warp_affine_5pt writes in fixed geometry, so sharpness, exposure and contrast measured on them compare between a 30-pixel
// and a 600-pixel face; pose and resolution follow from the five landmarks the detector returns.
//
// The definition is include/frhip.h fr_face_quality_f16 (tests/helpers/quality_ref.py is the NumPy form): the
// luma byte L of every pixel of the window (rows 20..99, columns 16..95) and of the one-pixel ring round it, five integer
// metrics over the window, four float32 landmark terms, and a verdict mask against scalar thresholds.
//
// One launch, one workgroup of 256 threads per slot, no atomics:
//  1. stage: thread i takes pixels i, i + 256, ... of the 82 x 82 block; a pixel is ONE 16-byte load (8 halves, 3 used), a row of
//     the block is 1312 contiguous bytes.  Each pixel becomes its luma byte in LDS (6724 bytes).
//  2. behind one barrier thread i takes window pixels i, i + 256, ... (25 each): its sums are 32-bit, the wave reduces them with xor
//     shuffles - a wave holds 1600 pixels, so even its sum of D^2 (at most 1600 * 1020^2 = 1.66e9) fits 32 bits - and thread 0 adds
//     the four waves' partials in 64 bits.  Integer sums in any order give the same bits: the result does not depend on the shape.
//  3. thread 0 finishes: the 64-bit variances, the landmark terms in the stated operation order (the library is built with
//     -ffp-contract=off: no fused multiply-add), the verdict.
// A slot without a face returns before any read of its crop or landmarks.
#include "common.h"

namespace {

constexpr int QS = 112;                                         // crop side
constexpr int QY0 = 20, QX0 = 16, QW = 80;                      // the window: rows 20..99, columns 16..95
constexpr int QB = QW + 2;                                      // window plus ring: 82 x 82
constexpr int QN = QW * QW;                                     // 6400 pixels

struct Limits {
    float min_eye2;
    int mean_lo, mean_hi, contrast_min, sharp_min, clip_max;
    float yaw_max, pitch_lo, pitch_hi;
};

// the byte the warp rounded to: two singly rounded f32 operations, round to nearest even, clamped
__device__ __forceinline__ int crop_byte(half_t h) {
    const float v = (float)h * 127.5f + 127.5f;
    return (int)fminf(fmaxf(__builtin_rintf(v), 0.f), 255.f);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float cross2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }

__global__ __launch_bounds__(256) void face_quality_f16(const half_t* __restrict__ crops, const float* __restrict__ kps,
                                                        const int32_t* __restrict__ slot_counts, int cap, int32_t* __restrict__ qi,
                                                        float* __restrict__ qf, int32_t* __restrict__ verdict, Limits k) {
    __shared__ uint8_t lum[QB * QB];
    __shared__ int part[4][6];
    const int s = blockIdx.x, tid = threadIdx.x;
    if (slot_counts && !slot_valid(slot_counts, cap, s)) {      // block-uniform: neither the crop nor the landmarks are read
        if (tid < 8) qi[(int64_t)s * 8 + tid] = 0;
        if (tid < 4) qf[(int64_t)s * 4 + tid] = 0.f;
        if (tid == 0) verdict[s] = -1;
        return;
    }
    const half_t* __restrict__ crop = crops + (int64_t)s * (QS * QS * 8);
    for (int i = tid; i < QB * QB; i += 256) {
        const int y = i / QB, x = i - y * QB;
        const half8 p = *reinterpret_cast<const half8*>(crop + ((QY0 - 1 + y) * QS + (QX0 - 1 + x)) * 8);
        const int R = crop_byte(p[0]), G = crop_byte(p[1]), B = crop_byte(p[2]);
        lum[i] = (uint8_t)((77 * R + 150 * G + 29 * B + 128) >> 8);
    }
    __syncthreads();
    int sL = 0, sD = 0, dark = 0, bright = 0;
    unsigned sL2 = 0, sD2 = 0;                                  // per wave: at most 1600 * 255^2 and 1600 * 1020^2, below 2^32
    for (int i = tid; i < QN; i += 256) {
        const int y = i / QW, x = i - y * QW;
        const uint8_t* c = lum + (y + 1) * QB + (x + 1);
        const int L = c[0];
        const int D = 4 * L - (int)c[-QB] - (int)c[QB] - (int)c[-1] - (int)c[1];
        sL += L;
        sL2 += (unsigned)(L * L);
        sD += D;
        sD2 += (unsigned)(D * D);
        dark += L <= 15 ? 1 : 0;
        bright += L >= 240 ? 1 : 0;
    }
    sL = wave_sum_i(sL);
    sD = wave_sum_i(sD);
    dark = wave_sum_i(dark);
    bright = wave_sum_i(bright);
    sL2 = (unsigned)wave_sum_i((int)sL2);                       // two's complement: the sum modulo 2^32 is the unsigned sum
    sD2 = (unsigned)wave_sum_i((int)sD2);
    if ((tid & 63) == 0) {
        int* w = part[tid >> 6];
        w[0] = sL; w[1] = sD; w[2] = dark; w[3] = bright; w[4] = (int)sL2; w[5] = (int)sD2;
    }
    __syncthreads();
    if (tid != 0) return;
    int64_t tL = 0, tD = 0, tL2 = 0, tD2 = 0;
    int tdark = 0, tbright = 0;
    for (int w = 0; w < 4; ++w) {
        tL += part[w][0];
        tD += part[w][1];
        tdark += part[w][2];
        tbright += part[w][3];
        tL2 += (int64_t)(unsigned)part[w][4];
        tD2 += (int64_t)(unsigned)part[w][5];                   // up to 6 658 560 000 in all: 64 bits from here on
    }
    const int64_t n = QN;
    const int mean = (int)((tL + n / 2) / n);
    const int contrast = (int)((n * tL2 - tL * tL) / (n * n));  // both numerators are n^2 times a variance: never negative
    const int sharp = (int)((n * tD2 - tD * tD) / (n * n));

    const float* p = kps + (int64_t)s * 10;
    const float lex = p[0], ley = p[1], rex = p[2], rey = p[3], nx = p[4], ny = p[5], lmx = p[6], lmy = p[7], rmx = p[8], rmy = p[9];
    const float ex = rex - lex, ey = rey - ley;
    const float d2 = ex * ex + ey * ey;
    const float ax = nx - lex, ay = ny - ley;
    const float t = ax * ex + ay * ey;
    const float mx = (lmx + rmx) * 0.5f, my = (lmy + rmy) * 0.5f;
    const float c = cross2(ex, ey, ax, ay);
    const float m = cross2(ex, ey, mx - lex, my - ley);

    int v = 0;
    if (d2 < k.min_eye2) v |= 1;
    if (mean < k.mean_lo) v |= 2;
    if (mean > k.mean_hi) v |= 4;
    if (contrast < k.contrast_min) v |= 8;
    if (sharp < k.sharp_min) v |= 16;
    if (tdark + tbright > k.clip_max) v |= 32;
    if (fabsf((t + t) - d2) > k.yaw_max * d2) v |= 64;
    if (!(m > 0.f) || c < k.pitch_lo * m || c > k.pitch_hi * m) v |= 128;

    int32_t* oi = qi + (int64_t)s * 8;
    oi[0] = mean; oi[1] = contrast; oi[2] = sharp; oi[3] = tdark; oi[4] = tbright; oi[5] = 0; oi[6] = 0; oi[7] = 0;
    float* of = qf + (int64_t)s * 4;
    of[0] = d2; of[1] = t; of[2] = c; of[3] = m;
    verdict[s] = v;
}

}  // namespace

extern "C" int fr_face_quality_f16(const void* crops, const float* kps, const int32_t* slot_counts, int cap, int S, int32_t* qi,
                                   float* qf, int32_t* verdict, float min_eye2, int mean_lo, int mean_hi, int contrast_min,
                                   int sharp_min, int clip_max, float yaw_max, float pitch_lo, float pitch_hi, fr_stream_t stream) {
    FR_REQUIRE(S >= 0 && S <= 65535 * 64, "fr_face_quality_f16: bad size (0 .. 65535 * 64 slots)");
    FR_REQUIRE(!slot_counts || cap >= 1, "fr_face_quality_f16: cap %d below 1 with slot counts given", cap);
    FR_REQUIRE(min_eye2 >= 0.f && min_eye2 <= 3.0e38f, "fr_face_quality_f16: min_eye2 must be finite and not negative");
    FR_REQUIRE(mean_lo >= 0 && mean_lo <= 255 && mean_hi >= 0 && mean_hi <= 255, "fr_face_quality_f16: mean_lo %d / mean_hi %d outside 0 .. 255",
               mean_lo, mean_hi);
    FR_REQUIRE(contrast_min >= 0 && sharp_min >= 0, "fr_face_quality_f16: contrast_min %d / sharp_min %d below 0", contrast_min, sharp_min);
    FR_REQUIRE(clip_max >= 0 && clip_max <= QN, "fr_face_quality_f16: clip_max %d outside 0 .. %d", clip_max, QN);
    FR_REQUIRE(yaw_max >= 0.f, "fr_face_quality_f16: yaw_max below 0 (or NaN)");
    FR_REQUIRE(pitch_lo <= pitch_hi, "fr_face_quality_f16: pitch_lo above pitch_hi (or a NaN)");
    if (S == 0) return FR_OK;
    FR_REQUIRE(crops && kps && qi && qf && verdict, "fr_face_quality_f16: null pointer");
    FR_REQUIRE((reinterpret_cast<uintptr_t>(crops) & 15) == 0, "fr_face_quality_f16: crops must start on 16 bytes");
    face_quality_f16<<<(unsigned)S, 256, 0, fr_stream(stream)>>>(reinterpret_cast<const half_t*>(crops), kps, slot_counts, cap, qi, qf,
                                                                 verdict, Limits{min_eye2, mean_lo, mean_hi, contrast_min, sharp_min, clip_max,
                                                                                 yaw_max, pitch_lo, pitch_hi});
    FR_CHECK_LAUNCH("face_quality_f16");
    return FR_OK;
}
