// The detector's numeric conventions, shared by the f32 kernels (detect_ops.hip, dconv_mfma.hip) and the fused /
// split-precision kernels of the batch path (pnet_conv1.hip, pnet_fused.hip, ro_conv1.hip, ro_conv2.hip, ro_gemm.hip).
//
// The batch path may only change how a value is computed, never a keep / reject decision:
// its margins (refine_margin, ro_margin) send every cell or crop near a stage threshold back through the f32 kernels.
// That is sound only when both paths start from the same pixels.  So every kernel that resizes on the fly uses this
// one resize, and the fused crop + conv1 equals fr_crop_resize_norm followed by the f32 layer bit for bit
// (tests/test_gpu_detect.py).  The margins are derived from the error of the split format below.
#pragma once
#include "common.h"

// ------------------------------------------------------------------ bilinear resize (half-pixel centres, clamped)
struct Lerp { int i0, i1; float w; };

__device__ __forceinline__ Lerp lerp_coord(int d, float ratio, int n) {
    float f = ((float)d + 0.5f) * ratio - 0.5f;
    float fl = floorf(f);
    Lerp r;
    r.w = f - fl;
    int i = (int)fl;
    r.i0 = min(max(i, 0), n - 1);
    r.i1 = min(max(i + 1, 0), n - 1);
    return r;
}

__device__ __forceinline__ float bilerp(float p00, float p01, float p10, float p11, float wx, float wy) {
    float top = (1.0f - wx) * p00 + wx * p01;
    float bot = (1.0f - wx) * p10 + wx * p11;
    return (1.0f - wy) * top + wy * bot;
}

// ------------------------------------------------------------------ max of raw MFMA sums (pools done in registers)
// max(x, y) as v_med3_f32(x, y, +inf) with the +inf in a register the compiler cannot see through: ONE instruction - fmaxf (and
// med3 with a literal +inf, which hipcc folds to it) puts a canonicalising self-max in front of every operand of unknown origin
// (MFMA results; never NaN here).  NOT an inline-asm v_max_f32: the hazard recogniser does not see an asm statement's operands,
// and an asm max placed right behind the MFMA that produces its operand read the register before the matrix pipe had written it
// (round 4: the first of four maxima wrong, in interior tiles only - elsewhere a select sat in between).
__device__ __forceinline__ float opaque_inf() {
    float r;
    asm("v_mov_b32 %0, 0x7f800000" : "=v"(r));
    return r;
}
__device__ __forceinline__ float vmax(float x, float y, float pinf) { return __builtin_amdgcn_fmed3f(x, y, pinf); }

// ------------------------------------------------------------------ split-precision operands: x = hi + lo in f16
// Element e of hi and lo gets the split of x (hi and lo are f16 vectors or arrays).
template <class V>
__device__ __forceinline__ void split_f16(float x, V& hi, V& lo, int e) {
    const half_t h = (half_t)x;
    hi[e] = h; lo[e] = (half_t)(x - (float)h);
}

// A split-precision logit difference that is not finite (an operand beyond the f16 range, or inf - inf) says nothing about
// the f32 one.  Every decision site sends such a cell or crop to the exact pass, like one inside the margin band.
__device__ __forceinline__ bool split_nonfinite(float d) { return !__builtin_isfinite(d); }

// Plane p of the split of x: p = 0 gives hi, p = 1 gives lo (the weight packers write one plane at a time).
__device__ __forceinline__ half_t split_f16_plane(float x, int p) {
    half_t hi[1], lo[1];
    split_f16(x, hi, lo, 0);
    return p ? lo[0] : hi[0];
}
