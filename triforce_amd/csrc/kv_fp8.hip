// FP8 (OCP e4m3fn) storage of the target's full KV cache: the append quantizer and the FP8 -> fp16 row copy.
// The decode attention over the codes is tf_attn_decode_fp8_act in attn.hip.
//
// Contract (include/triforce_hip.h, "FP8 KV cache"): one exponent per (layer, head, token) row of
// D = 128 values, separately for K and V.  a = max |x| of the row; e = the smallest integer with 448 * 2^e >= a, clamped to
// [-15, 7] (an all-zero row: -15); stored as the byte e + 127.  code = e4m3fn(clamp(x * 2^-e, -448, 448)), round to nearest
// even.  deq = fp16(code) * 2^e, exact in fp16 over that exponent range.
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

#define KVQ_D 128
#define KVQ_EMIN (-15)
#define KVQ_EMAX 7

// e4m3fn code of |y| <= 448, round to nearest even, in integer-exact steps (no dependence on the conversion instructions'
// rounding or saturation modes): below 2^-6 the codes are the multiples of 2^-9; above, 8 mantissa steps per binade
__device__ __forceinline__ unsigned e4m3_rne(float y) {
    const unsigned s = (__float_as_uint(y) >> 24) & 0x80u;
    const float a = fabsf(y);
    unsigned c;
    if (a < 0.015625f) {
        c = (unsigned)rintf(a * 512.0f);                       // 0 .. 8 (8 = 2^-6, the first normal code)
    } else {
        const int E = (int)((__float_as_uint(a) >> 23) & 0xffu) - 127;                // -6 .. 8
        c = (unsigned)((E + 7) << 3) + (unsigned)rintf(ldexpf(a, 3 - E)) - 8u;      // a carry into the next binade is exact
    }
    return s | c;
}

// One wave per (head, row): lane l owns values 2 l, 2 l + 1.  blockIdx.z: 0 = K, 1 = V.
__global__ __launch_bounds__(256) void kv_quant_rows_kernel(const h16* __restrict__ k_in, const h16* __restrict__ v_in,
                                                            int64_t in_st, int64_t in_sh, uint8_t* __restrict__ k_code,
                                                            uint8_t* __restrict__ v_code, uint8_t* __restrict__ k_exp,
                                                            uint8_t* __restrict__ v_exp, int64_t code_st, int64_t code_sh,
                                                            int64_t exp_sh, int n, int slot0, const int32_t* __restrict__ slot0_dev,
                                                            h16* __restrict__ k_deq, h16* __restrict__ v_deq) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), h = blockIdx.y;
    if (r >= n) return;
    const bool isv = blockIdx.z != 0;
    const h16* x = (isv ? v_in : k_in) + (int64_t)h * in_sh + (int64_t)r * in_st + 2 * lane;
    const half2v xv = *reinterpret_cast<const half2v*>(x);
    const float x0 = (float)xv[0], x1 = (float)xv[1];
    const float a = wave_max(fmaxf(fabsf(x0), fabsf(x1)));
    int e = KVQ_EMIN;
    while (e < KVQ_EMAX && ldexpf(448.0f, e) < a) ++e;            // wave-uniform
    const float inv = ldexpf(1.0f, -e);
    const unsigned c0 = e4m3_rne(fminf(fmaxf(x0 * inv, -448.0f), 448.0f));
    const unsigned c1 = e4m3_rne(fminf(fmaxf(x1 * inv, -448.0f), 448.0f));
    const int slot = slot0_dev ? *slot0_dev : slot0;
    const int64_t row = (int64_t)slot + r;
    uint8_t* cd = (isv ? v_code : k_code) + (int64_t)h * code_sh + row * code_st + 2 * lane;
    *reinterpret_cast<unsigned short*>(cd) = (unsigned short)(c0 | (c1 << 8));
    if (lane == 0) (isv ? v_exp : k_exp)[(int64_t)h * exp_sh + row] = (uint8_t)(e + 127);
    h16* dq = isv ? v_deq : k_deq;
    if (dq) {
        const half2v p = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c0 | (c1 << 8), 1.0f, false);
        const float sc = ldexpf(1.0f, e);
        half2v o;
        o[0] = (h16)((float)p[0] * sc);                           // exact (the contract's exponent range)
        o[1] = (h16)((float)p[1] * sc);
        *reinterpret_cast<half2v*>(dq + (int64_t)h * in_sh + (int64_t)r * in_st + 2 * lane) = o;
    }
}

// (L, H, T, D) codes + (L, H, T) exponent bytes -> (L, H, T, D) fp16 rows; blockIdx.z: 0 = K, 1 = V.  A thread turns 16 codes
// into two half8 (kv_copy_rows_kernel's loop over a (layer, head) plane).
__global__ __launch_bounds__(256) void kv_dequant_rows_kernel(const uint8_t* __restrict__ sk, const uint8_t* __restrict__ sv,
                                                              int64_t ssl, int64_t sst, int64_t ssh,
                                                              const uint8_t* __restrict__ ek, const uint8_t* __restrict__ ev,
                                                              int64_t esl, int64_t esh, h16* __restrict__ dk,
                                                              h16* __restrict__ dv, int64_t dsl, int64_t dst_t, int64_t dsh,
                                                              int src_t0, int dst_t0, int n, int H, int D) {
    const int l = blockIdx.y / H, h = blockIdx.y % H;
    const bool isv = blockIdx.z != 0;
    const uint8_t* s = (isv ? sv : sk) + (int64_t)l * ssl + (int64_t)h * ssh;
    const uint8_t* ex = (isv ? ev : ek) + (int64_t)l * esl + (int64_t)h * esh;
    h16* d = (isv ? dv : dk) + (int64_t)l * dsl + (int64_t)h * dsh;
    const int vpr = D / 16;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * vpr; i += gridDim.x * blockDim.x) {
        const int r = i / vpr, dv16 = i - r * vpr;
        const u32x4 w = *reinterpret_cast<const u32x4*>(s + (int64_t)(src_t0 + r) * sst + 16 * dv16);
        const float sc = ldexpf(1.0f, (int)ex[src_t0 + r] - 127);
        half8 lo, hi;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const half2v p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[q], 1.0f, false);
            const half2v p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[q], 1.0f, true);
            half8& o = q < 2 ? lo : hi;
            const int b = (q & 1) * 4;
            o[b] = (h16)((float)p0[0] * sc);
            o[b + 1] = (h16)((float)p0[1] * sc);
            o[b + 2] = (h16)((float)p1[0] * sc);
            o[b + 3] = (h16)((float)p1[1] * sc);
        }
        h16* o = d + (int64_t)(dst_t0 + r) * dst_t + 16 * dv16;
        store_half8(o, lo);
        store_half8(o + 8, hi);
    }
}

// ---- C ABI ------------------------------------------------------------------------------------
extern "C" int tf_kv_quant_rows(const void* k_in, const void* v_in, int64_t in_stride_t, int64_t in_stride_h, void* k_codes,
                                void* v_codes, void* k_exp, void* v_exp, int64_t code_stride_t, int64_t code_stride_h,
                                int64_t exp_stride_h, int slot0, const int32_t* slot0_dev, int n, int H, int D, void* k_deq,
                                void* v_deq, void* stream) {
    if (!k_in || !v_in || !k_codes || !v_codes || !k_exp || !v_exp) return TF_EINVAL;
    if ((k_deq == nullptr) != (v_deq == nullptr)) return TF_EINVAL;
    if (D != KVQ_D || n < 0 || H < 1 || slot0 < 0) return TF_EINVAL;
    if (in_stride_t < D || (in_stride_t % 2) || (in_stride_h % 2)) return TF_EINVAL;           // 4-byte loads
    if (code_stride_t < D || (code_stride_t % 2) || (code_stride_h % 2) || exp_stride_h < 1) return TF_EINVAL;
    if (n == 0) return TF_OK;
    hipLaunchKernelGGL(kv_quant_rows_kernel, dim3((n + 3) / 4, H, 2), dim3(256), 0, (hipStream_t)stream, (const h16*)k_in,
                       (const h16*)v_in, in_stride_t, in_stride_h, (uint8_t*)k_codes, (uint8_t*)v_codes, (uint8_t*)k_exp,
                       (uint8_t*)v_exp, code_stride_t, code_stride_h, exp_stride_h, n, slot0, slot0_dev, (h16*)k_deq,
                       (h16*)v_deq);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_kv_dequant_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                                       int64_t src_stride_h, const void* exp_k, const void* exp_v, int64_t exp_stride_l,
                                       int64_t exp_stride_h, void* dst_k, void* dst_v, int64_t dst_stride_l,
                                       int64_t dst_stride_t, int64_t dst_stride_h, int src_t0, int dst_t0, int n, int L, int H,
                                       int D, void* stream) {
    if (!src_k || !src_v || !exp_k || !exp_v || !dst_k || !dst_v) return TF_EINVAL;
    if (n < 0 || L < 1 || H < 1 || D != KVQ_D || src_t0 < 0 || dst_t0 < 0) return TF_EINVAL;
    if ((src_stride_t % 16) || (src_stride_h % 16) || (src_stride_l % 16) || (dst_stride_t % 8) || (dst_stride_h % 8) ||
        (dst_stride_l % 8))
        return TF_EINVAL;
    if (n == 0) return TF_OK;
    int gx = (n * (D / 16) + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(kv_dequant_rows_kernel, dim3(gx, L * H, 2), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src_k,
                       (const uint8_t*)src_v, src_stride_l, src_stride_t, src_stride_h, (const uint8_t*)exp_k,
                       (const uint8_t*)exp_v, exp_stride_l, exp_stride_h, (h16*)dst_k, (h16*)dst_v, dst_stride_l, dst_stride_t,
                       dst_stride_h, src_t0, dst_t0, n, H, D);
    TF_LAUNCH_CHECK();
    return TF_OK;
}
