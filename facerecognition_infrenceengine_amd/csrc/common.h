// Shared helpers for libfrhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include "../../include/frhip.h"

#define FR_WAVE 64

void fr_set_error(const char* fmt, ...);

#define FR_REQUIRE(cond, ...)                      \
    do {                                           \
        if (!(cond)) {                             \
            fr_set_error(__VA_ARGS__);             \
            return FR_E_INVALID;                   \
        }                                          \
    } while (0)

#define FR_CHECK_LAUNCH(name)                                                     \
    do {                                                                          \
        hipError_t e_ = hipGetLastError();                                        \
        if (e_ != hipSuccess) {                                                   \
            fr_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
            return FR_E_LAUNCH;                                                   \
        }                                                                         \
    } while (0)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: one atomic bit per device ordinal
// remembers where it has been raised (idempotent; the only process-wide state the library keeps).
struct FrDevLatch { std::atomic<unsigned long long> mask{0}; };
static inline bool fr_raise_lds(const void* kernel, size_t bytes, FrDevLatch& latch) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
    if (bit && (latch.mask.load(std::memory_order_acquire) & bit)) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    if (bit) latch.mask.fetch_or(bit, std::memory_order_release);
    return true;
}

static inline hipStream_t fr_stream(fr_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
static inline int fr_cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef int int2v __attribute__((ext_vector_type(2)));
typedef int int4v __attribute__((ext_vector_type(4)));
typedef int int8v __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;                  // LDS destination of a buffer -> LDS load
typedef unsigned long long u64_unaligned __attribute__((aligned(1)));       // 8-byte load from any byte address

// Unrolls f(integral_constant<0>) .. f(integral_constant<N - 1>): the index is a compile-time constant in the body.
template <int N, int I = 0, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

// Keeps the compiler from moving any instruction across this point.
#define FR_PIN() __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Raw buffer descriptor over bytes [p, p + bytes): loads past the end return 0, stores past it are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
}

// f16 16x16x32 MFMA on operands held as raw 16-byte fragments.
__device__ __forceinline__ float4v mfma16(const int4v& a, const int4v& b, float4v c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, a), __builtin_bit_cast(half8, b), c, 0, 0, 0);
}

// 4 floats -> 4 fp8 e4m3 (OCP) bytes, saturating at +-448 (the conversion itself would produce NaN past the range)
__device__ __forceinline__ int pack_fp8x4(float a, float b, float c, float d) {
    a = __builtin_amdgcn_fmed3f(a, -448.f, 448.f); b = __builtin_amdgcn_fmed3f(b, -448.f, 448.f);
    c = __builtin_amdgcn_fmed3f(c, -448.f, 448.f); d = __builtin_amdgcn_fmed3f(d, -448.f, 448.f);
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
    return v;
}

// query slot q belongs to segment q / seg_len and is real iff its position in the segment < seg_counts[segment]
__device__ __forceinline__ bool slot_valid(const int32_t* seg_counts, int seg_len, int q) {
    const int seg = q / seg_len;
    return q - seg * seg_len < seg_counts[seg];
}
