// SCRFD head maps -> per-frame, per-level candidate lists for fr_sort_nms.
// One workgroup per frame walks one level's anchors in raster / anchor order in chunks of 1024 and keeps those with
// logit >= logit_thr, the first `cap` of them, in that order (an ordered compaction: ballots + wave counts, no atomics on
// the order).  Every product, sum and quotient is ONE IEEE f32 operation (no contraction), so NumPy float32 gives the same
// bits: cx = x * stride, box = (cx - d0 s, cy - d1 s, cx + d2 s, cy + d3 s) / det_scale, keypoint i = (cx + k[2i] s,
// cy + k[2i+1] s) / det_scale, score = 1 / (1 + expf(-logit)).
#include "common.h"

namespace {

__global__ __launch_bounds__(1024) void scrfd_decode(const float* __restrict__ score, const float* __restrict__ bbox,
                                                     const float* __restrict__ kps, int Hl, int Wl, int A, int stride, int level,
                                                     float logit_thr, const float* __restrict__ det_scale, int cap,
                                                     float* __restrict__ boxes, float* __restrict__ scores, float* __restrict__ aux,
                                                     int32_t* __restrict__ counts) {
    __shared__ int wave_cnt[16];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = Hl * Wl * A;
    const float* sc = score + (int64_t)f * na;
    const float* bb = bbox + (int64_t)f * na * 4;
    const float* kp = kps + (int64_t)f * na * 10;
    const int64_t seg = (int64_t)f * 3 + level;
    const float ds = det_scale[f], s = (float)stride;
    int kept = 0;
    for (int a0 = 0; a0 < na && kept < cap; a0 += 1024) {
        const int a = a0 + tid;
        float lg = 0.f;
        bool on = false;
        if (a < na) { lg = sc[a]; on = lg >= logit_thr; }
        const unsigned long long bal = __ballot(on);
        if (lane == 0) wave_cnt[wave] = __popcll(bal);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const int c = wave_cnt[w]; if (w < wave) base += c; total += c; }
        const int slot = kept + base + __popcll(bal & ((1ull << lane) - 1ull));
        if (on && slot < cap) {
            const int cell = a / A;
            const int y = cell / Wl, x = cell - y * Wl;
            const float cx = (float)(x * stride), cy = (float)(y * stride);
            const float4 d = *reinterpret_cast<const float4*>(bb + (int64_t)a * 4);
            const int64_t o = seg * cap + slot;
            float4 b;
            b.x = __fdiv_rn(__fsub_rn(cx, __fmul_rn(d.x, s)), ds);
            b.y = __fdiv_rn(__fsub_rn(cy, __fmul_rn(d.y, s)), ds);
            b.z = __fdiv_rn(__fadd_rn(cx, __fmul_rn(d.z, s)), ds);
            b.w = __fdiv_rn(__fadd_rn(cy, __fmul_rn(d.w, s)), ds);
            *reinterpret_cast<float4*>(boxes + o * 4) = b;
            scores[o] = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-lg)));
            const float* k = kp + (int64_t)a * 10;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                aux[o * 10 + 2 * i] = __fdiv_rn(__fadd_rn(cx, __fmul_rn(k[2 * i], s)), ds);
                aux[o * 10 + 2 * i + 1] = __fdiv_rn(__fadd_rn(cy, __fmul_rn(k[2 * i + 1], s)), ds);
            }
        }
        kept += total;
        __syncthreads();                                             // wave_cnt is rewritten by the next chunk
    }
    if (tid == 0) counts[seg] = kept < cap ? kept : cap;
}

}  // namespace

extern "C" int fr_scrfd_decode(const float* score, const float* bbox, const float* kps, int nframes, int Hl, int Wl, int A, int stride,
                               int level, float logit_thr, const float* det_scale, int cap, float* boxes, float* scores, float* aux,
                               int32_t* counts, fr_stream_t stream) {
    FR_REQUIRE(score && bbox && kps && det_scale && boxes && scores && aux && counts, "fr_scrfd_decode: null pointer");
    FR_REQUIRE(nframes > 0 && Hl > 0 && Wl > 0 && A > 0 && stride > 0 && cap > 0 && level >= 0 && level < 3,
               "fr_scrfd_decode: bad argument (level 0..2, positive sizes)");
    FR_REQUIRE((int64_t)Hl * Wl * A < (1 << 30), "fr_scrfd_decode: level too large");
    scrfd_decode<<<nframes, 1024, 0, fr_stream(stream)>>>(score, bbox, kps, Hl, Wl, A, stride, level, logit_thr, det_scale, cap, boxes,
                                                          scores, aux, counts);
    FR_CHECK_LAUNCH("scrfd_decode");
    return FR_OK;
}
