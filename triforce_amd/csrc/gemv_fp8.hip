// FP8-WEIGHT skinny (decode) GEMMs for gfx950 — the retrieval-cache ("spec") forward of the target model with its five
// GEMMs streaming e4m3fn weight codes instead of fp16 (TRIFORCE_RETRIEVAL_WEIGHTS=fp8).  That forward
// only DRAFTS: the target verify keeps the fp16 weights and the accept rule keeps the output exact for whatever
// distribution the draft tokens were sampled from, so quantizing this tier changes acceptance, never the output.
//
// Contract (include/triforce_hip.h, "FP8-weight skinny GEMMs"):
//   * weight-only: W[n][k] ~= s[n] * e4m3fn(code[n][k]); activations stay fp16.  Every e4m3fn value is exact in fp16, so
//     the codes are decoded to fp16 with scale 1.0 (v_cvt_scalef32_pk_f16_fp8) and multiplied on the SAME
//     v_mfma_f32_16x16x32_f16 as the 16-bit kernel (csrc/gemv.hip), fp32 accumulation;
//   * the row scale is applied once, in fp32, on the accumulator, exactly where the 16-bit kernel rounds:
//     fp16(acc) there, fp16(s[n] * acc) here (gate and up each with their own scale before their own rounding);
//   * every other rounding point is the 16-bit kernel's: norm prologue, residual add, SwiGLU, RoPE + append, the fp32
//     cast of the logits, the sum-of-squares hand-off (ss_in / ss_out).
//
// Packing (triforce_amd.ops.pack_weight_fp8): [N/16 panels][K/64 super-chunks][4 (g)][16 (i)][16 bytes]; the 16 bytes of
// piece (g, i) are W[n0+i][k0+8g .. +7] (bytes 0-7, 32-wide chunk 2s) and W[n0+i][k0+32+8g .. +7] (bytes 8-15, chunk
// 2s+1).  One 16x64 tile is one contiguous KiB (the memory shape of the 16-bit form's 16x32 tile): a lane's 16-byte load
// feeds the A operands of two MFMAs, over exactly the k-octets the 16-bit kernel's two consecutive chunks would use — so
// the B operand (x, either activation layout) is read as there.  Requires K % 64 == 0.
//
// Structure: one workgroup per 16-row panel, its waves split the panel's K range, partial accumulators meet in LDS, wave
// 0 runs the epilogue — the 16-bit kernel's one-panel form without the split-K, exchange and two-panel variants (none of
// them is on the single-GPU spec forward).
#include "common.h"

#define F8_LOAD(p) __builtin_nontemporal_load(p)   // weights are read once per forward: non-temporal

// Launch rule: waves per workgroup.  Grids of few panels (o_proj / down_proj at 7B: 256 panels) take the wide form, as in
// the 16-bit kernel; gate|up GEMMs never do.
constexpr int F8_WAVES = 4;
constexpr int F8_WAVES_WIDE = 8;
constexpr int F8_WIDE_MAX_PANELS = 512;   // grids of up to this many panels run F8_WAVES_WIDE waves per panel

enum { F8_PLAIN = 0, F8_GATEUP = 1, F8_F32 = 2, F8_QKV = 3 };

struct F8Act {                        // element (m, k) at base[m * sm + (k / 8) * sk + (k % 8)]  (see tf_skinny_gemm_act)
    int64_t sm, sk;
};

struct F8Rope {                       // arguments of the RoPE + KV-append epilogue (F8_QKV), as SgRope in csrc/gemv.hip
    const h16* cosb;
    const h16* sinb;
    const int64_t* positions;
    h16* q_out;
    h16* k_cache;
    h16* v_cache;
    int64_t stride_t, stride_h;
    const int32_t* slot0_dev;
    int slot0, H, D, rotate_k;
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));

// 16 e4m3fn codes -> the two half8 A operands (bytes 0-7, bytes 8-15); exact, scale 1.0
__device__ __forceinline__ void f8_decode(u32x4 w, half8& lo, half8& hi) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const half2v p0 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[d], 1.0f, false);   // bytes 0, 1 of the dword
        const half2v p1 = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[d], 1.0f, true);    // bytes 2, 3
        half8& o = d < 2 ? lo : hi;
        const int e = (d & 1) * 4;
        o[e] = p0[0];
        o[e + 1] = p0[1];
        o[e + 2] = p1[0];
        o[e + 3] = p1[1];
    }
}

// h = w_ln * fp16(x * inv) (the 16-bit kernel's sg_normalise)
__device__ __forceinline__ half8 f8_normalise(half8 xv, half8 wv, float inv) {
    half8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = hmul_rn(wv[e], (h16)((float)xv[e] * inv));
    return o;
}

// U = super-chunks (KiB of codes per weight stream) in flight per wave.
template <int MT, int MODE, bool NORM, int WAVES, int U>
__global__ __launch_bounds__(WAVES * 64) void skinny_gemm_fp8_kernel(const u32x4* __restrict__ wp,
                                                                     const u32x4* __restrict__ wp_up,
                                                                     const h16* __restrict__ x,
                                                                     const float* __restrict__ ss_in,
                                                                     const h16* __restrict__ ln_w, int K, int M,
                                                                     int xa_sm, int xa_sk, float eps,
                                                                     const float* __restrict__ sc,
                                                                     const float* __restrict__ sc_up, const h16* resid,
                                                                     F8Act ra, void* yv, F8Act ya, F8Rope rp,
                                                                     float* __restrict__ ss_out) {
    constexpr bool GATEUP = MODE == F8_GATEUP;
    constexpr int NA = GATEUP ? 2 : 1;
    const F8Act xa = {(int64_t)xa_sm, (int64_t)xa_sk};
    const int panel = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int nsc = K >> 6, nchunks = K >> 5;
    const int cpw = (nsc + WAVES - 1) / WAVES;
    const int c0 = wave * cpw, c1 = min(nsc, c0 + cpw);

    __shared__ float sm[WAVES][NA][MT][64][4];
    __shared__ float sm_ss[NORM ? WAVES : 1][MT][16];
    __shared__ float red[NORM ? MT : 1][NORM ? WAVES * 4 : 1][16];

    f32x4 acc[NA][MT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[a][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t pstride = (int64_t)nsc * 64;               // 16-byte pieces per panel
    const u32x4* wa = wp + (int64_t)panel * pstride + lane;
    const u32x4* wu = GATEUP ? (wp_up + (int64_t)panel * pstride + lane) : wa;
    const int64_t xcs = 4 * xa.sk;                           // elements per 32-wide k-chunk step of the B operand
    const h16* xr[MT];
    bool xok[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = t * 16 + li;
        xok[t] = m < M;
        xr[t] = x + (int64_t)(xok[t] ? m : 0) * xa.sm + (int64_t)g * xa.sk;
    }
    const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

    // the first batch of weight codes goes out before the norm's reductions (they only need x / the partials)
    u32x4 a0[U][NA];
    const bool any = c0 < c1;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int cu = any ? min(c0 + u, c1 - 1) : 0;
        a0[u][0] = F8_LOAD(wa + (int64_t)cu * 64);
        if (GATEUP) a0[u][NA - 1] = F8_LOAD(wu + (int64_t)cu * 64);
    }
    // this lane's row scales (wave 0 runs the epilogue): 16 rows per panel, lane (g, li) owns rows 4g .. 4g+3
    float sn[4], su[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        sn[r] = sc[panel * 16 + 4 * g + r];
        su[r] = GATEUP ? sc_up[panel * 16 + 4 * g + r] : 0.f;
    }

    float inv[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) inv[t] = 1.f;
    if constexpr (NORM) {
        float tot[MT];
        if (ss_in) {
            // per-panel sums of squares left by the producer of x, folded in the 16-bit kernel's order: thread (pg, m)
            // sums the partials of panels pg, pg + G, ... in turn, then the G group sums are added in group order
            constexpr int G = WAVES * 4;
            const int nparts = K >> 4, pg = tid >> 4, m16 = tid & 15;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                float part = 0.f;
                for (int p = pg; p < nparts; p += G) part += ss_in[(int64_t)p * 32 + t * 16 + m16];
                red[t][pg][m16] = part;
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                tot[t] = 0.f;
                for (int j = 0; j < G; ++j) tot[t] += red[t][j][li];
            }
        } else {
            // sum(x^2) over ALL of K: this wave's share of 32-wide chunks, then across the waves (the 16-bit kernel's order)
            float ss[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) ss[t] = 0.f;
            const int cpa = (nchunks + WAVES - 1) / WAVES;
            const int n0 = wave * cpa, n1 = min(nchunks, n0 + cpa);
            for (int cc = n0; cc < n1; ++cc) {
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const half8 v = xok[t] ? load_half8(xr[t] + xcs * cc) : zero8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float f = (float)v[e];
                        ss[t] = fmaf(f, f, ss[t]);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                ss[t] += __shfl_xor(ss[t], 16, 64);
                ss[t] += __shfl_xor(ss[t], 32, 64);
                if (g == 0) sm_ss[wave][t][li] = ss[t];
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                tot[t] = 0.f;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) tot[t] += sm_ss[w][t][li];
            }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) inv[t] = 1.0f / sqrtf(tot[t] / (float)K + eps);
    }

    // K loop: U super-chunks per batch, every load of a batch issued before its MFMAs.  Loads past the wave's end re-read
    // its last super-chunk instead of being predicated (a conditional load makes the waitcnt pass wait for everything);
    // their MFMAs are skipped.
    for (int c = c0; c < c1; c += U) {
        u32x4 a[U][NA];
        half8 b[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = min(c + u, c1 - 1);
#pragma unroll
            for (int aa = 0; aa < NA; ++aa) {
                if (c == c0) a[u][aa] = a0[u][aa];
                else a[u][aa] = F8_LOAD((aa ? wu : wa) + (int64_t)cu * 64);
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int ch = 2 * cu + h;                   // 32-wide chunk of this half of the super-chunk
                half8 lw = zero8;
                if (NORM) lw = load_half8(ln_w + 32 * ch + 8 * g);
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    const half8 v = load_half8(xr[t] + xcs * ch);
                    b[u][t][h] = xok[t] ? (NORM ? f8_normalise(v, lw, inv[t]) : v) : zero8;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u < c1) {
#pragma unroll
                for (int aa = 0; aa < NA; ++aa) {
                    half8 lo, hi;
                    f8_decode(a[u][aa], lo, hi);
#pragma unroll
                    for (int t = 0; t < MT; ++t) {
                        acc[aa][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(lo, b[u][t][0], acc[aa][t], 0, 0, 0);
                        acc[aa][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(hi, b[u][t][1], acc[aa][t], 0, 0, 0);
                    }
                }
            }
        }
    }

    // merge across the waves; C layout: lane holds D[n = 4g + r][m = li]
#pragma unroll
    for (int aa = 0; aa < NA; ++aa)
#pragma unroll
        for (int t = 0; t < MT; ++t) *reinterpret_cast<f32x4*>(&sm[wave][aa][t][lane][0]) = acc[aa][t];
    __syncthreads();
    if (wave != 0) return;

    // epilogue operands: RoPE tables of this lane's columns, residual pointer offsets
    half4 rope_cs[MT], rope_sn[MT];
    if constexpr (MODE == F8_QKV) {
        const int H = rp.H, D = rp.D, pph = D >> 4;
        const int sec = panel / (H * pph), pp = panel % pph;
        const int d = 8 * pp + 4 * (g & 1) + ((g >= 2) ? (D >> 1) : 0);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = t * 16 + li;
            rope_cs[t] = half4{0, 0, 0, 0};
            rope_sn[t] = half4{0, 0, 0, 0};
            if (m < M && sec != 2 && (sec == 0 || rp.rotate_k)) {
                const int64_t pos = rp.positions[m];
                rope_cs[t] = *reinterpret_cast<const half4*>(rp.cosb + pos * D + d);
                rope_sn[t] = *reinterpret_cast<const half4*>(rp.sinb + pos * D + d);
            }
        }
    }
    const int64_t r_off = (int64_t)(2 * panel + (g >> 1)) * ra.sk + 4 * (g & 1);   // this lane's 4 columns, piece form
    const int64_t y_off = (int64_t)(2 * panel + (g >> 1)) * ya.sk + 4 * (g & 1);

#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = t * 16 + li;
        float s[4], s2[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) {
                a += sm[w][0][t][lane][r];
                if (GATEUP) b += sm[w][NA - 1][t][lane][r];
            }
            s[r] = sn[r] * a;                                    // the row scale, once, on the fp32 accumulator
            s2[r] = GATEUP ? su[r] * b : 0.f;
        }
        if constexpr (MODE == F8_QKV) {
            // panel -> (section, head, 8-wide rotary block): q and k panels hold rows d0..d0+7 | d0+D/2..d0+D/2+7
            const int H = rp.H, D = rp.D, half = D >> 1, pph = D >> 4;
            const int sec = panel / (H * pph), hd = (panel / pph) % H, pp = panel % pph;
            h16 val[4], oth[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                val[r] = (h16)s[r];                                      // (two roundings by the compiler's choice; guard: tests/test_gpu_rounding_probes.py)
                oth[r] = (h16)__shfl_xor((float)val[r], 32, 64);         // rotary partner: lane g <-> g ^ 2 (exact)
            }
            if (m >= M) continue;
            const int slot = (rp.slot0_dev ? *rp.slot0_dev : rp.slot0) + m;
            half4 out;
            if (sec == 2) {                                              // v: natural row order, plain copy
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r] = val[r];
                h16* dst = rp.v_cache + (int64_t)slot * rp.stride_t + (int64_t)hd * rp.stride_h + 16 * pp + 4 * g;
                *reinterpret_cast<half4*>(dst) = out;
                continue;
            }
            const bool hi = g >= 2;
            const int d = 8 * pp + 4 * (g & 1) + (hi ? half : 0);
            if (sec == 0 || rp.rotate_k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const h16 cs = rope_cs[t][r], sn_ = rope_sn[t][r];
                    const h16 rh = hi ? oth[r] : (h16)(-(float)oth[r]);
                    out[r] = hadd_rn(hmul_rn(val[r], cs), hmul_rn(rh, sn_));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) out[r] = val[r];
            }
            h16* dst = (sec == 0) ? rp.q_out + ((int64_t)m * H + hd) * D + d
                                  : rp.k_cache + (int64_t)slot * rp.stride_t + (int64_t)hd * rp.stride_h + d;
            *reinterpret_cast<half4*>(dst) = out;
            continue;
        }
        const bool row_ok = m < M;
        if (!row_ok && !(MODE == F8_PLAIN && ss_out)) continue;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (row_ok) {
            if (MODE == F8_F32) {                                        // logits.float(): fp16 result, then cast
                float* dst = (float*)yv + (int64_t)m * ya.sm + panel * 16 + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[r] = (float)(h16)s[r];   // (two roundings by the compiler's choice; guard: tests/test_gpu_rounding_probes.py)
            } else {
                half4 o;
                if (GATEUP) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const h16 gt = (h16)s[r], up = (h16)s2[r];       // (two roundings by the compiler's choice; guard: tests/test_gpu_rounding_probes.py)
                        const float gf = (float)gt;
                        const h16 act = (h16)(gf / (1.0f + expf(-gf)));
                        o[r] = hmul_rn(act, up);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        o[r] = f32_then_h16(s[r]);                           // two roundings: written (h16)s[r] it folds (common.h)
                        if (resid) o[r] = hadd_rn(resid[(int64_t)m * ra.sm + r_off + r], o[r]);   // residual + hidden
                        q[r] = (float)o[r];
                    }
                }
                h16* dst = (h16*)yv + (int64_t)m * ya.sm + y_off;
                if (((ya.sm | ya.sk) % 4) == 0 && (reinterpret_cast<uintptr_t>(yv) % 8) == 0) {
                    *reinterpret_cast<half4*>(dst) = o;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) dst[r] = o[r];
                }
            }
        }
        if (MODE == F8_PLAIN && ss_out) {            // this panel's share of sum(y^2) per row, for the next norm prologue
            float ssq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            ssq += __shfl_xor(ssq, 16, 64);
            ssq += __shfl_xor(ssq, 32, 64);
            if (g == 0) ss_out[(int64_t)panel * 32 + m] = ssq;
        }
    }
}

struct F8Args {
    const void *wp, *wp_up, *x, *ln_w, *resid;
    const float *sc, *sc_up;
    void* y;
    F8Act xa, ra, ya;
    float eps;
    int M, N, K;
    const float* ss_in;
    float* ss_out;
};

template <int MT, int MODE, bool NORM, int WAVES>
static void launch_f8_w(const F8Args& a, const F8Rope& rp, hipStream_t st) {
    constexpr int U = MODE == F8_GATEUP ? 2 : 4;                   // 4 KiB of codes in flight per wave
    hipLaunchKernelGGL((skinny_gemm_fp8_kernel<MT, MODE, NORM, WAVES, U>), dim3(a.N / 16), dim3(WAVES * 64), 0, st,
                       (const u32x4*)a.wp, (const u32x4*)a.wp_up, (const h16*)a.x, a.ss_in, (const h16*)a.ln_w, a.K, a.M,
                       (int)a.xa.sm, (int)a.xa.sk, a.eps, a.sc, a.sc_up, (const h16*)a.resid, a.ra, a.y, a.ya, rp,
                       a.ss_out);
}

template <int MODE, bool NORM>
static int launch_f8(const F8Args& a, const F8Rope& rp, hipStream_t st) {
    const int panels = a.N / 16, nsc = a.K >> 6;
    // few panels (o / down at 7B: 256 on 256 CUs) -> more waves per panel, while every wave keeps >= 2 super-chunks
    const bool wide = MODE != F8_GATEUP && panels <= F8_WIDE_MAX_PANELS && nsc >= 2 * F8_WAVES_WIDE;
    if (a.M <= 16) {
        if (wide) launch_f8_w<1, MODE, NORM, F8_WAVES_WIDE>(a, rp, st);
        else launch_f8_w<1, MODE, NORM, F8_WAVES>(a, rp, st);
    } else {
        if (wide) launch_f8_w<2, MODE, NORM, F8_WAVES_WIDE>(a, rp, st);
        else launch_f8_w<2, MODE, NORM, F8_WAVES>(a, rp, st);
    }
    TF_LAUNCH_CHECK();
    return TF_OK;
}

static bool f8_act_ok(const F8Act& s) { return s.sm > 0 && s.sk > 0 && (s.sm % 8) == 0 && (s.sk % 8) == 0; }

static bool f8_shape_ok(int M, int N, int K, const F8Act& xa) {
    return M >= 1 && M <= 32 && N >= 16 && (N % 16) == 0 && K >= 64 && (K % 64) == 0 && f8_act_ok(xa) &&
           xa.sm <= 0x7fffffff && xa.sk <= 0x7fffffff;     // (the kernel takes x's two strides as 32-bit arguments)
}

extern "C" int tf_skinny_gemm_fp8_act(const void* w_fp8, const float* scale, const void* x, int64_t xs_m, int64_t xs_k,
                                      const void* ln_w, float eps, const float* ss_in, const void* resid, int64_t rs_m,
                                      int64_t rs_k, float* ss_out, void* y, int64_t ys_m, int64_t ys_k, int M, int N, int K,
                                      int out_f32, void* stream) {
    F8Args a = {};
    a.wp = w_fp8, a.sc = scale, a.x = x, a.ln_w = ln_w, a.resid = resid, a.y = y;
    a.xa = F8Act{xs_m, xs_k}, a.ra = F8Act{rs_m, rs_k}, a.ya = F8Act{ys_m, ys_k};
    a.eps = eps, a.M = M, a.N = N, a.K = K, a.ss_in = ss_in, a.ss_out = ss_out;
    if (!w_fp8 || !scale || !x || !y || !f8_shape_ok(M, N, K, a.xa)) return TF_EINVAL;
    if ((out_f32 && (resid || ss_out)) || (ss_in && !ln_w)) return TF_EINVAL;
    if (ys_m <= 0 || (!out_f32 && ys_k <= 0) || (resid && (rs_m <= 0 || rs_k <= 0))) return TF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const F8Rope rp = {};
    if (out_f32) return ln_w ? launch_f8<F8_F32, true>(a, rp, st) : launch_f8<F8_F32, false>(a, rp, st);
    return ln_w ? launch_f8<F8_PLAIN, true>(a, rp, st) : launch_f8<F8_PLAIN, false>(a, rp, st);
}

extern "C" int tf_skinny_gemm_swiglu_fp8_act(const void* gate_fp8, const float* gate_scale, const void* up_fp8,
                                             const float* up_scale, const void* x, int64_t xs_m, int64_t xs_k,
                                             const void* ln_w, float eps, const float* ss_in, void* act, int64_t ys_m,
                                             int64_t ys_k, int M, int I, int K, void* stream) {
    F8Args a = {};
    a.wp = gate_fp8, a.wp_up = up_fp8, a.sc = gate_scale, a.sc_up = up_scale, a.x = x, a.ln_w = ln_w, a.y = act;
    a.xa = F8Act{xs_m, xs_k}, a.ya = F8Act{ys_m, ys_k}, a.ra = F8Act{8, 8};
    a.eps = eps, a.M = M, a.N = I, a.K = K, a.ss_in = ss_in;
    if (!gate_fp8 || !up_fp8 || !gate_scale || !up_scale || !x || !act || !f8_shape_ok(M, I, K, a.xa) || (ss_in && !ln_w))
        return TF_EINVAL;
    if (ys_m <= 0 || ys_k <= 0) return TF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const F8Rope rp = {};
    return ln_w ? launch_f8<F8_GATEUP, true>(a, rp, st) : launch_f8<F8_GATEUP, false>(a, rp, st);
}

extern "C" int tf_skinny_qkv_rope_fp8_act(const void* wqkv_fp8, const float* scale, const void* x, int64_t xs_m,
                                          int64_t xs_k, const void* ln_w, float eps, const float* ss_in, const void* cosb,
                                          const void* sinb, const int64_t* positions, void* q_out, void* k_cache,
                                          void* v_cache, int64_t stride_t, int64_t stride_h, int slot0,
                                          const int32_t* slot0_dev, int M, int H, int D, int K, int rotate_k,
                                          void* stream) {
    if (!wqkv_fp8 || !scale || !x || !cosb || !sinb || !positions || !q_out || !k_cache || !v_cache) return TF_EINVAL;
    F8Args a = {};
    a.wp = wqkv_fp8, a.sc = scale, a.x = x, a.ln_w = ln_w;
    a.xa = F8Act{xs_m, xs_k}, a.ra = F8Act{8, 8}, a.ya = F8Act{8, 8};
    a.eps = eps, a.M = M, a.N = 3 * H * D, a.K = K, a.ss_in = ss_in;
    if (H < 1 || D < 32 || (D % 32) || !f8_shape_ok(M, a.N, K, a.xa) || (ss_in && !ln_w)) return TF_EINVAL;
    if ((stride_t % 4) || (stride_h % 4)) return TF_EINVAL;                          // 8-byte epilogue stores
    hipStream_t st = (hipStream_t)stream;
    F8Rope rp;
    rp.cosb = (const h16*)cosb;
    rp.sinb = (const h16*)sinb;
    rp.positions = positions;
    rp.q_out = (h16*)q_out;
    rp.k_cache = (h16*)k_cache;
    rp.v_cache = (h16*)v_cache;
    rp.stride_t = stride_t;
    rp.stride_h = stride_h;
    rp.slot0_dev = slot0_dev;
    rp.slot0 = slot0;
    rp.H = H;
    rp.D = D;
    rp.rotate_k = rotate_k;
    return ln_w ? launch_f8<F8_QKV, true>(a, rp, st) : launch_f8<F8_QKV, false>(a, rp, st);
}
