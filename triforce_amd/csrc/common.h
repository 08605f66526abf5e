// Shared device helpers for the gfx950 kernels.  Wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/triforce_hip.h"

typedef _Float16 h16;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define TF_WAVE 64

#define TF_LAUNCH_CHECK()                      \
    do {                                       \
        hipError_t e__ = hipGetLastError();    \
        if (e__ != hipSuccess) return (int)e__; \
    } while (0)

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// fp16 product / sum with torch's half semantics: compute in fp32, round once to fp16.
__device__ __forceinline__ h16 hmul_rn(h16 a, h16 b) { return (h16)((float)a * (float)b); }
__device__ __forceinline__ h16 hadd_rn(h16 a, h16 b) { return (h16)((float)a + (float)b); }

// fp16(a * b) with the contract's TWO roundings: the product to fp32, that to fp16 (include/triforce_hip.h, "ROUNDING OF
// fp16(a * b)").  Written as (h16)(a * b) the compiler folds the pair into v_fma_mixlo_f16, which rounds the exact product
// once — one fp16 ulp apart wherever the fp32 product lands on an fp16 midpoint (found by the exact probes of
// tests/test_gpu_qk_norm.py, pinned site by site by tests/test_gpu_rounding_probes.py).  The empty asm keeps the fp32 value.
__device__ __forceinline__ h16 f32_then_h16(float p) {          // p: an fp32 product formed just before
    asm volatile("" : "+v"(p));
    return (h16)p;
}
__device__ __forceinline__ h16 mul_f32_then_h16(float a, float b) { return f32_then_h16(a * b); }

__device__ __forceinline__ half8 load_half8(const h16* p) { return *reinterpret_cast<const half8*>(p); }
// Streamed-once data (KV pages, weights in a decode forward): non-temporal 16-B load (global_load_dwordx4 ... nt)
// — shorter issue->landed latency for data no other CU will re-read (MI355X_MICROARCH.md, row nt-weights).
__device__ __forceinline__ half8 load_half8_stream(const h16* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const half8*>(p));
}
__device__ __forceinline__ void store_half8(h16* p, half8 v) { *reinterpret_cast<half8*>(p) = v; }
