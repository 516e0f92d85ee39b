// The SCRFD detector's layers: NHWC f16 activations whose channel count is padded to a multiple of 8
// with zeros, f32 accumulation.  The body widths of SCRFD-10GF (28 / 56 / 88 / 224 / 80) are no multiples of 64, and its
// blocks end in relu(conv + bias + identity): neither fits fr_conv_nhwc_f16 (64-channel granule, prelu-then-residual).
//
//   fr_det_conv_f16          1x1 / 3x3, stride 1 / 2, zero padding: implicit GEMM on the f16 16x16x32 MFMA
//   fr_det_conv_act_f16      the same kernel with a PReLU epilogue (the recognition plans of mbf.py)
//   fr_det_input_f16         u8 BGR canvas -> f16 RGB (x - 127.5) / 128, 8 channels
//   fr_det_pool_f16          max / average pool
//   fr_det_upsample_add_f16  lateral + nearest x2 (or x1) of the coarser map
#include "common.h"

namespace {

struct DetConvP {
    const half_t* x; const half_t* w; const float* bias; const float* slope; const half_t* res; void* y;
    int H, W, Cin, Ho, Wo, KW, stride, pad;
    int G, CG, ksteps;              // 8-channel groups of the K axis (taps * Cin / 8), groups per tap, K steps of 4 groups
    int ntiles, CoutW;              // 16-channel output tiles, packed output channels (ntiles * 16)
    int cout_store, ldo, relu, out_f32;
    int64_t M;                      // output pixels N * Ho * Wo
};

// One wave: MT * 16 output pixels x NT * 16 output channels.  The K axis is (tap, input channel) flattened in groups of 8
// channels; an MFMA step takes 4 groups, lane l supplying group 4 * step + (l >> 4) of output channel / pixel (l & 15) - so a
// step may straddle taps and only the last step of a layer carries zero groups (Cin = 8 at the stem: 9 groups, 3 steps).
// The weights are the MFMA's A operand and the pixels its B operand: a lane then holds 4 CONSECUTIVE output channels of one
// pixel, stored as one 8-byte word.
// PRELU: the epilogue's activation is v < 0 ? v * slope[channel] : v instead of the optional ReLU (a separate instantiation, so
// the detector's kernels are the code they were).
template <int MT, int NT, bool PRELU>
__global__ __launch_bounds__(256) void det_conv(DetConvP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * (MT * 16);
    if (m0 >= p.M) return;                                           // wave-uniform
    const int nt0 = blockIdx.y * NT;
    int64_t nbase[MT];
    int iy0[MT], ix0[MT];
    bool pv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int64_t m = m0 + mt * 16 + r;
        pv[mt] = m < p.M;
        const int64_t mm = pv[mt] ? m : 0;
        const int n = (int)(mm / ((int64_t)p.Ho * p.Wo));
        const int rem = (int)(mm - (int64_t)n * p.Ho * p.Wo);
        const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0[mt] = oy * p.stride - p.pad;
        ix0[mt] = ox * p.stride - p.pad;
        nbase[mt] = (int64_t)n * p.H;
    }
    float4v acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = float4v{0.f, 0.f, 0.f, 0.f};
    int g = q, tap = 0, cg = q;
    while (cg >= p.CG) { cg -= p.CG; ++tap; }
    const int4v zero = int4v{0, 0, 0, 0};
    for (int ks = 0; ks < p.ksteps; ++ks) {
        int4v wf[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int tile = nt0 + nt;
            wf[nt] = zero;
            if (tile < p.ntiles)
                wf[nt] = *reinterpret_cast<const int4v*>(p.w + ((((int64_t)ks * p.CoutW + tile * 16 + r) * 4 + q) << 3));
        }
        const bool gv = g < p.G;
        const int ky = p.KW == 1 ? 0 : (tap * 11) >> 5;              // tap / 3 for tap < 12
        const int kx = tap - ky * p.KW;
        int4v xf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int iy = iy0[mt] + ky, ix = ix0[mt] + kx;
            xf[mt] = zero;
            if (pv[mt] && gv && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W)
                xf[mt] = *reinterpret_cast<const int4v*>(p.x + (((nbase[mt] + iy) * p.W + ix) * p.Cin + (cg << 3)));
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = mfma16(wf[nt], xf[mt], acc[mt][nt]);
        g += 4; cg += 4;
        while (cg >= p.CG) { cg -= p.CG; ++tap; }
    }
    // epilogue: + bias, + residual, ReLU / PReLU, in that order; acc[mt][nt][i] = channel tile*16 + 4q + i of pixel m0 + 16 mt + r
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int64_t m = m0 + mt * 16 + r;
        if (m >= p.M) continue;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int tile = nt0 + nt;
            if (tile >= p.ntiles) continue;
            const int c0 = tile * 16 + q * 4;
            if (c0 >= p.cout_store) continue;
            const float4v b = *reinterpret_cast<const float4v*>(p.bias + c0);
            float4v sl = float4v{0.f, 0.f, 0.f, 0.f};
            if constexpr (PRELU) sl = *reinterpret_cast<const float4v*>(p.slope + c0);
            auto act = [&](float v, int i) { return PRELU ? (v < 0.f ? v * sl[i] : v) : (p.relu ? fmaxf(v, 0.f) : v); };
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = acc[mt][nt][i] + b[i];
            if (p.out_f32) {
                float* y = static_cast<float*>(p.y) + m * p.ldo;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (c0 + i < p.cout_store) y[c0 + i] = act(v[i], i);
            } else {                                                 // cout_store and ldo are multiples of 8 here
                if (p.res) {
                    const half4 rr = *reinterpret_cast<const half4*>(p.res + m * p.ldo + c0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = v[i] + (float)rr[i];
                }
                half4 o;
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = (half_t)act(v[i], i);
                *reinterpret_cast<half4*>(static_cast<half_t*>(p.y) + m * p.ldo + c0) = o;
            }
        }
    }
}

__global__ __launch_bounds__(256) void det_input(const uint8_t* __restrict__ canvas, half_t* __restrict__ y, int64_t npix) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const uint8_t* s = canvas + i * 3;
    half8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (half_t)0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (half_t)(((float)s[2 - c] - 127.5f) / 128.0f);      // BGR -> RGB; exact in f16
    *reinterpret_cast<half8*>(y + i * 8) = o;
}

// kind 0: max over the window's in-bounds taps.  kind 1: their mean - the sum in f64 (exact for f16 operands), divided by
// the in-bounds count, rounded ONCE to f16.  The host admits only windows that hold at least one in-bounds tap (and refuses
// count_include_pad wherever a window meets padding or the edge, so the in-bounds count is the only divisor there is).
__global__ __launch_bounds__(256) void det_pool(const half_t* __restrict__ x, half_t* __restrict__ y, int N, int H, int W, int C,
                                                int Ho, int Wo, int kind, int k, int stride, int pad) {
    const int CG = C >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * Ho * Wo * CG) return;
    const int cg = (int)(i % CG);
    const int64_t pix = i / CG;
    const int ox = (int)(pix % Wo);
    const int oy = (int)((pix / Wo) % Ho);
    const int n = (int)(pix / ((int64_t)Wo * Ho));
    double sum[8];
    float mx[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) { sum[c] = 0.0; mx[c] = -__builtin_inff(); }
    int cnt = 0;
    for (int ky = 0; ky < k; ++ky) {
        const int iy = oy * stride - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < k; ++kx) {
            const int ix = ox * stride - pad + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const half8 v = *reinterpret_cast<const half8*>(x + ((((int64_t)n * H + iy) * W + ix) * C + (cg << 3)));
            ++cnt;
#pragma unroll
            for (int c = 0; c < 8; ++c) { sum[c] += (double)v[c]; mx[c] = fmaxf(mx[c], (float)v[c]); }
        }
    }
    const double div = (double)(cnt > 0 ? cnt : 1);
    half8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = kind == 0 ? (half_t)mx[c] : (half_t)(sum[c] / div);
    *reinterpret_cast<half8*>(y + (pix * C + (cg << 3))) = o;
}

__global__ __launch_bounds__(256) void det_upsample_add(const half_t* __restrict__ coarse, const half_t* __restrict__ lateral,
                                                        half_t* __restrict__ y, int N, int H, int W, int C, int up) {
    const int CG = C >> 3;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * H * W * CG) return;
    const int cg = (int)(i % CG);
    const int64_t pix = i / CG;
    const int ox = (int)(pix % W);
    const int oy = (int)((pix / W) % H);
    const int n = (int)(pix / ((int64_t)W * H));
    const int Hc = H / up, Wc = W / up;
    const half8 a = *reinterpret_cast<const half8*>(lateral + pix * C + (cg << 3));
    const half8 b = *reinterpret_cast<const half8*>(coarse + ((((int64_t)n * Hc + oy / up) * Wc + ox / up) * C + (cg << 3)));
    half8 o;
#pragma unroll
    for (int c = 0; c < 8; ++c) o[c] = (half_t)((float)a[c] + (float)b[c]);       // f32 holds the sum of two f16 exactly enough: one rounding
    *reinterpret_cast<half8*>(y + pix * C + (cg << 3)) = o;
}

template <int MT, int NT>
void launch_conv(const DetConvP& p, hipStream_t s) {
    const dim3 grid((unsigned)fr_cdiv(p.M, (int64_t)MT * 64), (unsigned)fr_cdiv(p.ntiles, NT));
    if (p.slope) det_conv<MT, NT, true><<<grid, 256, 0, s>>>(p);
    else det_conv<MT, NT, false><<<grid, 256, 0, s>>>(p);
}

// what: the entry point's name in front of its messages.  slope != nullptr selects the PReLU epilogue.
int conv_entry(const char* what, const void* x, const void* w, const float* bias, const float* slope, const void* residual, void* y,
               int N, int H, int W, int Cin, int cout_packed, int K, int stride, int pad, int Ho, int Wo, int cout_store, int ldo,
               int relu, int out_f32, int tile, fr_stream_t stream) {
    FR_REQUIRE(x && w && bias && y, "%s: null pointer", what);
    FR_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 8 == 0, "%s: Cin %d must be a positive multiple of 8", what, Cin);
    FR_REQUIRE(cout_packed > 0 && cout_packed % 16 == 0, "%s: packed Cout %d must be a multiple of 16", what, cout_packed);
    FR_REQUIRE((K == 1 || K == 3) && (stride == 1 || stride == 2) && pad >= 0 && pad < K,
               "%s: kernel %d stride %d pad %d not supported (1x1 / 3x3, stride 1 / 2, pad < kernel)", what, K, stride, pad);
    FR_REQUIRE(H + 2 * pad >= K && W + 2 * pad >= K && Ho == (H + 2 * pad - K) / stride + 1 && Wo == (W + 2 * pad - K) / stride + 1,
               "%s: output %d x %d does not follow from input %d x %d", what, Ho, Wo, H, W);
    FR_REQUIRE(cout_store > 0 && cout_store <= cout_packed && cout_store <= ldo, "%s: bad cout_store %d / ldo %d", what, cout_store, ldo);
    FR_REQUIRE(out_f32 ? residual == nullptr : (cout_store % 8 == 0 && ldo % 8 == 0),
               "%s: f16 output needs cout_store and ldo in multiples of 8; f32 output takes no residual", what);
    DetConvP p;
    p.x = static_cast<const half_t*>(x); p.w = static_cast<const half_t*>(w); p.bias = bias; p.slope = slope;
    p.res = static_cast<const half_t*>(residual); p.y = y;
    p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.KW = K; p.stride = stride; p.pad = pad;
    p.CG = Cin / 8; p.G = K * K * p.CG; p.ksteps = (p.G + 3) / 4;
    p.ntiles = cout_packed / 16; p.CoutW = cout_packed;
    p.cout_store = cout_store; p.ldo = ldo; p.relu = relu != 0; p.out_f32 = out_f32 != 0;
    p.M = (int64_t)N * Ho * Wo;
    if (tile == 0) {
        const int nt = p.ntiles <= 2 ? 2 : 4;
        const int64_t cols = fr_cdiv(p.ntiles, nt);
        const int mt = (p.M / 64) * cols >= 2048 ? 4 : (p.M / 32) * cols >= 1024 ? 2 : 1;
        tile = mt * 10 + nt;
    }
    hipStream_t s = fr_stream(stream);
    switch (tile) {
        case 44: launch_conv<4, 4>(p, s); break;
        case 24: launch_conv<2, 4>(p, s); break;
        case 14: launch_conv<1, 4>(p, s); break;
        case 42: launch_conv<4, 2>(p, s); break;
        case 22: launch_conv<2, 2>(p, s); break;
        case 12: launch_conv<1, 2>(p, s); break;
        default: FR_REQUIRE(false, "%s: unknown tile shape %d (0, 44, 24, 14, 42, 22, 12)", what, tile);
    }
    FR_CHECK_LAUNCH("det_conv");
    return FR_OK;
}

}  // namespace

extern "C" size_t fr_det_conv_weight_halves(int Cin, int cout_packed, int K) {
    if (Cin <= 0 || cout_packed <= 0 || K <= 0) return 0;
    const int G = K * K * (Cin / 8);
    return (size_t)((G + 3) / 4) * (size_t)cout_packed * 32;
}

extern "C" int fr_det_conv_f16(const void* x, const void* w, const float* bias, const void* residual, void* y, int N, int H, int W,
                               int Cin, int cout_packed, int K, int stride, int pad, int Ho, int Wo, int cout_store, int ldo,
                               int relu, int out_f32, int tile, fr_stream_t stream) {
    return conv_entry("fr_det_conv_f16", x, w, bias, nullptr, residual, y, N, H, W, Cin, cout_packed, K, stride, pad, Ho, Wo, cout_store,
                      ldo, relu, out_f32, tile, stream);
}

extern "C" int fr_det_conv_act_f16(const void* x, const void* w, const float* bias, const float* slope, const void* residual, void* y,
                                   int N, int H, int W, int Cin, int cout_packed, int K, int stride, int pad, int Ho, int Wo,
                                   int cout_store, int ldo, int act, int out_f32, int tile, fr_stream_t stream) {
    FR_REQUIRE(act >= 0 && act <= 2, "fr_det_conv_act_f16: act %d is none of 0 (none), 1 (ReLU), 2 (PReLU)", act);
    FR_REQUIRE(act != 2 || slope, "fr_det_conv_act_f16: act 2 (PReLU) needs the slope vector");
    return conv_entry("fr_det_conv_act_f16", x, w, bias, act == 2 ? slope : nullptr, residual, y, N, H, W, Cin, cout_packed, K, stride, pad,
                      Ho, Wo, cout_store, ldo, act == 1, out_f32, tile, stream);
}

extern "C" int fr_det_input_f16(const uint8_t* canvas, void* y, int N, int H, int W, fr_stream_t stream) {
    FR_REQUIRE(canvas && y && N > 0 && H > 0 && W > 0, "fr_det_input_f16: bad argument");
    const int64_t npix = (int64_t)N * H * W;
    det_input<<<fr_cdiv(npix, 256), 256, 0, fr_stream(stream)>>>(canvas, static_cast<half_t*>(y), npix);
    FR_CHECK_LAUNCH("det_input");
    return FR_OK;
}

extern "C" int fr_det_pool_f16(const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int kind, int k, int stride,
                               int pad, fr_stream_t stream) {
    FR_REQUIRE(x && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "fr_det_pool_f16: bad argument (C in multiples of 8)");
    FR_REQUIRE((kind == 0 || kind == 1) && k >= 1 && k <= 3 && stride >= 1 && stride <= 2 && pad >= 0 && pad < k,
               "fr_det_pool_f16: kind %d kernel %d stride %d pad %d not supported", kind, k, stride, pad);
    // every window holds an in-bounds tap (the last one may hang over the edge: ceil mode)
    FR_REQUIRE(Ho > 0 && Wo > 0 && (Ho - 1) * stride - pad < H && (Wo - 1) * stride - pad < W,
               "fr_det_pool_f16: output %d x %d has windows outside the %d x %d input", Ho, Wo, H, W);
    const int64_t n = (int64_t)N * Ho * Wo * (C / 8);
    det_pool<<<fr_cdiv(n, 256), 256, 0, fr_stream(stream)>>>(static_cast<const half_t*>(x), static_cast<half_t*>(y), N, H, W, C, Ho, Wo,
                                                            kind, k, stride, pad);
    FR_CHECK_LAUNCH("det_pool");
    return FR_OK;
}

extern "C" int fr_det_upsample_add_f16(const void* coarse, const void* lateral, void* y, int N, int H, int W, int C, int up,
                                       fr_stream_t stream) {
    FR_REQUIRE(coarse && lateral && y && N > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "fr_det_upsample_add_f16: bad argument");
    FR_REQUIRE((up == 1 || up == 2) && H % up == 0 && W % up == 0, "fr_det_upsample_add_f16: factor %d on %d x %d", up, H, W);
    const int64_t n = (int64_t)N * H * W * (C / 8);
    det_upsample_add<<<fr_cdiv(n, 256), 256, 0, fr_stream(stream)>>>(static_cast<const half_t*>(coarse), static_cast<const half_t*>(lateral),
                                                                    static_cast<half_t*>(y), N, H, W, C, up);
    FR_CHECK_LAUNCH("det_upsample_add");
    return FR_OK;
}
