// FP8 (OCP e4m3fn) storage of the target's full KV cache: the append quantizer and the FP8 -> fp16 row copy; and of the
// retrieval cache: the chunk gather and the tail refresh into codes.
// The decode attention over the codes is tf_attn_decode_fp8_act / tf_attn_decode_fp8_tail_act in attn.hip.
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

// One wave quantizes one row of 128 values: lane l owns values 2 l, 2 l + 1 (x points at them).  Returns the pair of codes
// (low byte first) and, wave-uniform, the exponent e.
__device__ __forceinline__ unsigned kv_quant_row(const h16* __restrict__ x, int& e) {
    const half2v xv = *reinterpret_cast<const half2v*>(x);
    const float x0 = (float)xv[0], x1 = (float)xv[1];
    const float a = wave_max(fmaxf(fabsf(x0), fabsf(x1)));
    e = KVQ_EMIN;
    while (e < KVQ_EMAX && ldexpf(448.0f, e) < a) ++e;            // wave-uniform
    const float inv = ldexpf(1.0f, -e);
    const unsigned c0 = e4m3_rne(fminf(fmaxf(x0 * inv, -448.0f), 448.0f));
    const unsigned c1 = e4m3_rne(fminf(fmaxf(x1 * inv, -448.0f), 448.0f));
    return c0 | (c1 << 8);
}

// One wave per (head, row).  blockIdx.z: 0 = K, 1 = V.
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
    int e;
    const unsigned c = kv_quant_row((isv ? v_in : k_in) + (int64_t)h * in_sh + (int64_t)r * in_st + 2 * lane, e);
    const int slot = slot0_dev ? *slot0_dev : slot0;
    const int64_t row = (int64_t)slot + r;
    uint8_t* cd = (isv ? v_code : k_code) + (int64_t)h * code_sh + row * code_st + 2 * lane;
    *reinterpret_cast<unsigned short*>(cd) = (unsigned short)c;
    if (lane == 0) (isv ? v_exp : k_exp)[(int64_t)h * exp_sh + row] = (uint8_t)(e + 127);
    h16* dq = isv ? v_deq : k_deq;
    if (dq) {
        const half2v p = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c, 1.0f, false);
        const float sc = ldexpf(1.0f, e);
        half2v o;
        o[0] = (h16)((float)p[0] * sc);                           // exact (the contract's exponent range)
        o[1] = (h16)((float)p[1] * sc);
        *reinterpret_cast<half2v*>(dq + (int64_t)h * in_sh + (int64_t)r * in_st + 2 * lane) = o;
    }
}

// ---- FP8 retrieval cache (TRIFORCE_RETRIEVAL_KV=fp8): rows INTO codes from either source ----
// Both kernels below serve the chunk gather (idx != NULL: destination row r comes from source row idx[h][r / chunk] * chunk +
// r % chunk of one layer) and the tail refresh (idx == NULL: destination row dst_t0 + r from source row src_t0 + r of every
// layer).  blockIdx.y = l * H + h, blockIdx.z: 0 = K, 1 = V.
struct KvRowMap {
    const int32_t* idx;    // [H][sets] chunk ids, or NULL
    int sets, chunk, src_t0, dst_t0, n, H;
};
__device__ __forceinline__ int64_t kv_row_src(const KvRowMap& m, int h, int r) {
    if (!m.idx) return (int64_t)m.src_t0 + r;
    const int slot = r / m.chunk;
    return (int64_t)m.idx[(int64_t)h * m.sets + slot] * m.chunk + (r - slot * m.chunk);
}

// fp16 rows -> codes + exponents, the contract's quantizer: one wave per row
__global__ __launch_bounds__(256) void kv_rows_quant_kernel(const h16* __restrict__ sk, const h16* __restrict__ sv, int64_t ssl,
                                                            int64_t sst, int64_t ssh, uint8_t* __restrict__ dk,
                                                            uint8_t* __restrict__ dv, int64_t dsl, int64_t dst_t, int64_t dsh,
                                                            uint8_t* __restrict__ ek, uint8_t* __restrict__ ev, int64_t esl,
                                                            int64_t esh, KvRowMap m) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m.n) return;
    const int l = blockIdx.y / m.H, h = blockIdx.y % m.H;
    const bool isv = blockIdx.z != 0;
    int e;
    const unsigned c = kv_quant_row((isv ? sv : sk) + (int64_t)l * ssl + (int64_t)h * ssh + kv_row_src(m, h, r) * sst + 2 * lane, e);
    const int64_t row = (int64_t)m.dst_t0 + r;
    uint8_t* cd = (isv ? dv : dk) + (int64_t)l * dsl + (int64_t)h * dsh + row * dst_t + 2 * lane;
    *reinterpret_cast<unsigned short*>(cd) = (unsigned short)c;
    if (lane == 0) (isv ? ev : ek)[(int64_t)l * esl + (int64_t)h * esh + row] = (uint8_t)(e + 127);
}

// codes + exponents -> codes + exponents, bytes copied: 8 threads per 128-byte row, the first of them carries the exponent
__global__ __launch_bounds__(256) void kv_rows_copy_f8_kernel(const uint8_t* __restrict__ sk, const uint8_t* __restrict__ sv,
                                                              int64_t ssl, int64_t sst, int64_t ssh,
                                                              const uint8_t* __restrict__ sek, const uint8_t* __restrict__ sev,
                                                              int64_t sesl, int64_t sesh, uint8_t* __restrict__ dk,
                                                              uint8_t* __restrict__ dv, int64_t dsl, int64_t dst_t, int64_t dsh,
                                                              uint8_t* __restrict__ ek, uint8_t* __restrict__ ev, int64_t esl,
                                                              int64_t esh, KvRowMap m) {
    const int r = blockIdx.x * 32 + (threadIdx.x >> 3), p = threadIdx.x & 7;
    if (r >= m.n) return;
    const int l = blockIdx.y / m.H, h = blockIdx.y % m.H;
    const bool isv = blockIdx.z != 0;
    const int64_t srow = kv_row_src(m, h, r), row = (int64_t)m.dst_t0 + r;
    const uint8_t* s = (isv ? sv : sk) + (int64_t)l * ssl + (int64_t)h * ssh + srow * sst + 16 * p;
    uint8_t* d = (isv ? dv : dk) + (int64_t)l * dsl + (int64_t)h * dsh + row * dst_t + 16 * p;
    *reinterpret_cast<u32x4*>(d) = *reinterpret_cast<const u32x4*>(s);
    if (p == 0)
        (isv ? ev : ek)[(int64_t)l * esl + (int64_t)h * esh + row] = (isv ? sev : sek)[(int64_t)l * sesl + (int64_t)h * sesh + srow];
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

// Rows into an FP8 cache from an fp16 source (src_exp_* NULL: quantized, strides in halves) or from codes (src_exp_* given:
// bytes copied, strides in bytes).  Shared by the two entry points below.
static int kv_rows_to_f8(const void* src_k, const void* src_v, int64_t ssl, int64_t sst, int64_t ssh, const void* sek,
                         const void* sev, int64_t sesl, int64_t sesh, void* k_codes, void* v_codes, int64_t dsl, int64_t dst_t,
                         int64_t dsh, void* k_exp, void* v_exp, int64_t esl, int64_t esh, KvRowMap m, int L, int D, void* stream) {
    if (!src_k || !src_v || !k_codes || !v_codes || !k_exp || !v_exp) return TF_EINVAL;
    if ((sek == nullptr) != (sev == nullptr)) return TF_EINVAL;
    if (D != KVQ_D || m.n < 0 || L < 1 || m.H < 1 || m.src_t0 < 0 || m.dst_t0 < 0) return TF_EINVAL;
    if (dst_t < D || (dst_t % 16) || (dsh % 16) || (dsl % 16) || esh < 1 || esl < 0) return TF_EINVAL;      // 16-byte stores
    const int a = sek ? 16 : 2;                                          // 16-byte copies / 4-byte loads
    if (sst < D || (sst % a) || (ssh % a) || (ssl % a) || (sek && (sesh < 1 || sesl < 0))) return TF_EINVAL;
    if (m.n == 0) return TF_OK;
    if (sek)
        hipLaunchKernelGGL(kv_rows_copy_f8_kernel, dim3((m.n + 31) / 32, L * m.H, 2), dim3(256), 0, (hipStream_t)stream,
                           (const uint8_t*)src_k, (const uint8_t*)src_v, ssl, sst, ssh, (const uint8_t*)sek, (const uint8_t*)sev,
                           sesl, sesh, (uint8_t*)k_codes, (uint8_t*)v_codes, dsl, dst_t, dsh, (uint8_t*)k_exp, (uint8_t*)v_exp,
                           esl, esh, m);
    else
        hipLaunchKernelGGL(kv_rows_quant_kernel, dim3((m.n + 3) / 4, L * m.H, 2), dim3(256), 0, (hipStream_t)stream,
                           (const h16*)src_k, (const h16*)src_v, ssl, sst, ssh, (uint8_t*)k_codes, (uint8_t*)v_codes, dsl, dst_t,
                           dsh, (uint8_t*)k_exp, (uint8_t*)v_exp, esl, esh, m);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_retrieval_gather_fp8(const void* k_src, const void* v_src, int64_t src_stride_t, int64_t src_stride_h,
                                       const void* k_src_exp, const void* v_src_exp, int64_t src_exp_stride_h,
                                       const int32_t* idx, void* k_codes, void* v_codes, void* k_exp, void* v_exp,
                                       int64_t code_stride_t, int64_t code_stride_h, int64_t exp_stride_h, int sets, int chunk,
                                       int H, int D, void* stream) {
    if (!idx || sets < 1 || chunk < 1 || H < 1 || (int64_t)sets * chunk > 0x7fffffff) return TF_EINVAL;
    if (exp_stride_h < (int64_t)sets * chunk) return TF_EINVAL;          // one exponent byte per gathered row of a head
    const KvRowMap m{idx, sets, chunk, 0, 0, sets * chunk, H};
    return kv_rows_to_f8(k_src, v_src, 0, src_stride_t, src_stride_h, k_src_exp, v_src_exp, 0, src_exp_stride_h, k_codes,
                         v_codes, 0, code_stride_t, code_stride_h, k_exp, v_exp, 0, exp_stride_h, m, 1, D, stream);
}

extern "C" int tf_kv_quant_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                                     int64_t src_stride_h, const void* src_exp_k, const void* src_exp_v,
                                     int64_t src_exp_stride_l, int64_t src_exp_stride_h, void* k_codes, void* v_codes,
                                     int64_t code_stride_l, int64_t code_stride_t, int64_t code_stride_h, void* k_exp,
                                     void* v_exp, int64_t exp_stride_l, int64_t exp_stride_h, int src_t0, int dst_t0, int n,
                                     int L, int H, int D, void* stream) {
    const KvRowMap m{nullptr, 0, 1, src_t0, dst_t0, n, H};
    return kv_rows_to_f8(src_k, src_v, src_stride_l, src_stride_t, src_stride_h, src_exp_k, src_exp_v, src_exp_stride_l,
                         src_exp_stride_h, k_codes, v_codes, code_stride_l, code_stride_t, code_stride_h, k_exp, v_exp,
                         exp_stride_l, exp_stride_h, m, L, D, stream);
}
