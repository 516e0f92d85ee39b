// Depthwise convolution: the layer MobileFaceNet and the small SCRFD detectors are built from.  NHWC f16
// activations with the channel count a multiple of 8 (det_conv.hip's layout), weights [K*K][C] tap-major, f32 accumulation
// over the in-bounds taps in (ky, kx) order, then bias, activation and ONE f16 rounding.  No matrix-core work: a layer
// reads its input once and writes its output once, and that traffic is its cost.
//
//   dw_band     a workgroup owns TR x 16 output pixels of one image for 64 channels: the (TR - 1) * stride + K input rows it
//               needs are staged in LDS once (16-byte loads, 8 lanes = 128 contiguous bytes of a pixel), a lane owns 8
//               channels and reads its K * K taps from there with 16-byte LDS reads
//   dw_global   K = H = W, pad 0 (the 7 x 7 "GDC" tail): one output pixel per image and channel; a lane owns 8 channels of one
//               image and walks the K * K taps straight from global memory, every element read once
//
// Both run the same operations per output element in the same order, so an element's bits depend on neither the path, the
// tile shape, the batch size nor the image's position in the batch.
#include <climits>
#include "common.h"

namespace {

constexpr int TW = 16;                  // output columns of a band tile

struct DwP {
    const half_t* x; const half_t* w; const float* bias; const float* slope; half_t* y;
    int N, H, W, C, CG, K, stride, pad, Ho, Wo, act;
    int TR, RI, CI, CIa;                // output rows of a tile; staged input rows / columns; LDS row pitch in pixels (CI up to 4)
    int tiles_y, tiles_x;
};

__device__ __forceinline__ void dw_store(const DwP& p, const float* acc, int cgg, int64_t pix) {
    const float4v b0 = *reinterpret_cast<const float4v*>(p.bias + (cgg << 3));
    const float4v b1 = *reinterpret_cast<const float4v*>(p.bias + (cgg << 3) + 4);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = acc[j] + (j < 4 ? b0[j] : b1[j - 4]);
    if (p.act == 1) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
    } else if (p.act == 2) {
        const float4v s0 = *reinterpret_cast<const float4v*>(p.slope + (cgg << 3));
        const float4v s1 = *reinterpret_cast<const float4v*>(p.slope + (cgg << 3) + 4);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = v[j] < 0.f ? v[j] * (j < 4 ? s0[j] : s1[j - 4]) : v[j];
    }
    half8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)v[j];
    *reinterpret_cast<half8*>(p.y + pix * p.C + (cgg << 3)) = o;
}

// LDS image: [RI][CIa] pixels of 8 x 16 bytes.  A wave reads 8 neighbouring output pixels x 8 channel groups per tap; the
// 16-lane groups of a 16-byte LDS read hold half the channel groups of 4 pixels.  At stride 1 those lie 128 bytes apart and
// cover the 256-byte bank row once.  At stride 2 they lie 256 bytes apart and would meet on the same banks two by two, so the
// columns of every aligned group of 4 are stored in the order 0 1 3 2: columns c and c + 2 then sit an odd number of pixels apart.
template <int KT>
__global__ __launch_bounds__(256) void dw_band(DwP p) {
    extern __shared__ int4v tile[];
    const int K = KT ? KT : p.K;
    const int cg = threadIdx.x & 7, slot = threadIdx.x >> 3;
    const int cgg = blockIdx.y * 8 + cg;
    const bool cv = cgg < p.CG;
    int t = blockIdx.x;
    const int tx = t % p.tiles_x; t /= p.tiles_x;
    const int ty = t % p.tiles_y;
    const int n = t / p.tiles_y;
    const int oy0 = ty * p.TR, ox0 = tx * TW;
    const int iy0 = oy0 * p.stride - p.pad, ix0 = ox0 * p.stride - p.pad;
    const bool swz = p.stride == 2;
    if (cv) {
        for (int i = slot; i < p.RI * p.CI; i += 32) {
            const int r = i / p.CI, c = i - r * p.CI;
            const int iy = iy0 + r, ix = ix0 + c;
            if ((unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W) {
                const int pc = swz ? c ^ ((c >> 1) & 1) : c;
                tile[(r * p.CIa + pc) * 8 + cg] =
                    *reinterpret_cast<const int4v*>(p.x + ((((int64_t)n * p.H + iy) * p.W + ix) * p.C + (cgg << 3)));
            }
        }
    }
    __syncthreads();
    if (!cv) return;
    [[maybe_unused]] half8 wr[KT == 3 ? 9 : 1];
    if constexpr (KT == 3) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) wr[tap] = *reinterpret_cast<const half8*>(p.w + (int64_t)tap * p.C + (cgg << 3));
    }
    for (int px = slot; px < p.TR * TW; px += 32) {
        const int ly = px / TW, lx = px - ly * TW;
        const int oy = oy0 + ly, ox = ox0 + lx;
        if (oy >= p.Ho || ox >= p.Wo) continue;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        auto tap = [&](int ky, int kx, const half8& wv) {
            const int r = ly * p.stride + ky, c = lx * p.stride + kx;
            if ((unsigned)(iy0 + r) >= (unsigned)p.H || (unsigned)(ix0 + c) >= (unsigned)p.W) return;      // a tap outside the input is skipped
            const int pc = swz ? c ^ ((c >> 1) & 1) : c;
            const half8 v = __builtin_bit_cast(half8, tile[(r * p.CIa + pc) * 8 + cg]);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)v[j] * (float)wv[j];                               // the product of two f16 is exact in f32
        };
        if constexpr (KT == 3) {
            static_for<9>([&](auto t) { tap(t.value / 3, t.value % 3, wr[t.value]); });
        } else {
            for (int ky = 0; ky < K; ++ky)
                for (int kx = 0; kx < K; ++kx)
                    tap(ky, kx, *reinterpret_cast<const half8*>(p.w + (int64_t)(ky * K + kx) * p.C + (cgg << 3)));
        }
        dw_store(p, acc, cgg, ((int64_t)n * p.Ho + oy) * p.Wo + ox);
    }
}

__global__ __launch_bounds__(256) void dw_global(DwP p) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.N * p.CG) return;
    const int cgg = (int)(i % p.CG);
    const int64_t n = i / p.CG;
    const int T = p.K * p.K;
    const half_t* xs = p.x + n * T * p.C + (cgg << 3);
    const half_t* ws = p.w + (cgg << 3);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int tap = 0; tap < T; ++tap) {                                         // tap = ky * K + kx: the band kernel's order
        const half8 v = *reinterpret_cast<const half8*>(xs + (int64_t)tap * p.C);
        const half8 wv = *reinterpret_cast<const half8*>(ws + (int64_t)tap * p.C);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)v[j] * (float)wv[j];
    }
    dw_store(p, acc, cgg, n);
}

}  // namespace

extern "C" int fr_dw_conv_f16(const void* x, const void* w, const float* bias, const float* slope, void* y, int N, int H, int W,
                              int C, int K, int stride, int pad, int Ho, int Wo, int act, fr_stream_t stream) {
    FR_REQUIRE(x && w && bias && y, "fr_dw_conv_f16: null pointer");
    FR_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "fr_dw_conv_f16: C %d must be a positive multiple of 8 (N %d, H %d, W %d)", C, N, H, W);
    FR_REQUIRE(K >= 1 && K <= 7 && (K & 1) && (stride == 1 || stride == 2) && pad >= 0 && pad <= K / 2,
               "fr_dw_conv_f16: kernel %d stride %d pad %d not supported (odd kernel <= 7, stride 1 / 2, pad <= kernel / 2)", K, stride, pad);
    FR_REQUIRE(H + 2 * pad >= K && W + 2 * pad >= K && Ho == (H + 2 * pad - K) / stride + 1 && Wo == (W + 2 * pad - K) / stride + 1,
               "fr_dw_conv_f16: output %d x %d does not follow from input %d x %d", Ho, Wo, H, W);
    FR_REQUIRE(act >= 0 && act <= 2, "fr_dw_conv_f16: act %d is none of 0 (none), 1 (ReLU), 2 (PReLU)", act);
    FR_REQUIRE(act != 2 || slope, "fr_dw_conv_f16: act 2 (PReLU) needs the slope vector");
    DwP p;
    p.x = static_cast<const half_t*>(x); p.w = static_cast<const half_t*>(w); p.bias = bias; p.slope = slope;
    p.y = static_cast<half_t*>(y);
    p.N = N; p.H = H; p.W = W; p.C = C; p.CG = C / 8; p.K = K; p.stride = stride; p.pad = pad; p.Ho = Ho; p.Wo = Wo; p.act = act;
    p.TR = p.RI = p.CI = p.CIa = p.tiles_y = p.tiles_x = 0;
    hipStream_t s = fr_stream(stream);
    if (K == H && K == W && pad == 0) {
        const int64_t n = (int64_t)N * p.CG;
        FR_REQUIRE(n / 256 < INT_MAX, "fr_dw_conv_f16: batch %d too large", N);
        dw_global<<<fr_cdiv(n, 256), 256, 0, s>>>(p);
        FR_CHECK_LAUNCH("dw_global");
        return FR_OK;
    }
    p.CI = (TW - 1) * stride + K;
    p.CIa = (p.CI + 3) & ~3;
    p.TR = 8;
    while (p.TR > 1 && (p.TR / 2 >= Ho || ((p.TR - 1) * stride + K) * p.CIa * 128 > 48 * 1024)) p.TR /= 2;
    p.RI = (p.TR - 1) * stride + K;
    p.tiles_y = fr_cdiv(Ho, p.TR); p.tiles_x = fr_cdiv(Wo, TW);
    const int64_t tiles = (int64_t)N * p.tiles_y * p.tiles_x;
    FR_REQUIRE(tiles <= INT_MAX && fr_cdiv(p.CG, 8) <= 65535, "fr_dw_conv_f16: %lld tiles x %d channels exceed one launch", (long long)tiles, C);
    const dim3 grid((unsigned)tiles, (unsigned)fr_cdiv(p.CG, 8));
    const size_t lds = (size_t)p.RI * p.CIa * 128;
    if (K == 3) dw_band<3><<<grid, 256, lds, s>>>(p);
    else dw_band<0><<<grid, 256, lds, s>>>(p);
    FR_CHECK_LAUNCH("dw_band");
    return FR_OK;
}
