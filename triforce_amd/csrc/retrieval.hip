// Retrieval-cache build and KV row movement for gfx950.
//
// Replaces RetrievalCache.init_graph_cache (models/cache.py:146-178; distributed twin :517-556):
//   chunk_k = K[:prefill].view(C, chunk, H, D).mean(dim=-3)            -> tf_retrieval_score
//   chunk_attn = q @ chunk_k^T   (fp16, un-scaled)                      -> tf_retrieval_score
//   topk(chunk_attn[:, :, 1:], k = sets-1) + 1, chunk 0 prepended       -> tf_retrieval_topk
//   gather of whole chunks for K and V                                  -> tf_retrieval_gather
// and RetrievalCache.update_graph_cache / StreamingLLMEvictionCache.evict_* (cache.py:180-182,
// 252-265) -> tf_kv_copy_rows / tf_kv_shift_rows.
//
// All of it is HBM-bound byte work: K is streamed exactly once (16-B loads, 256-B row segments
// per 16-lane group), nothing is staged in a temporary, the top-k runs in LDS.
#include "common.h"
#include "retrieval_rule.h"

// ---- scoring ------------------------------------------------------------------------------
// One 16-lane group per chunk (a wave scores 4 chunks per step); lane (c4, li) owns 8 d's.
// Rounding points follow the reference: mean -> fp16, dot -> fp16.  The mean is fp16(fp32(sum * (1 / chunk))), two roundings
// (mul_f32_then_h16, common.h), here and in chunk_mean_kernel alike: their bit-identity depends on it at chunks 12 and 24.
template <int D>
__global__ __launch_bounds__(256) void retrieval_score_kernel(const h16* __restrict__ k, int64_t stride_t,
                                                              int64_t stride_h, const h16* __restrict__ q,
                                                              h16* __restrict__ scores, int C, int chunk) {
    static_assert(D == 128 || D == 64, "head_dim");
    constexpr int LPR = D / 8;                   // lanes per row (16 for D=128, 8 for D=64)
    constexpr int GPB = 256 / LPR;               // chunk groups per block
    const int h = blockIdx.y;
    const int grp = threadIdx.x / LPR, li = threadIdx.x % LPR;
    const h16* kb = k + (int64_t)h * stride_h + 8 * li;
    float qf[8];
    {
        const half8 qv = load_half8(q + (int64_t)h * D + 8 * li);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)qv[e];
    }
    const float inv = 1.0f / (float)chunk;
    for (int c = blockIdx.x * GPB + grp; c < C; c += gridDim.x * GPB) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const h16* kp = kb + (int64_t)c * chunk * stride_t;
        for (int r = 0; r < chunk; ++r) {          // sequential fp32 accumulation over the chunk rows
            const half8 kv = load_half8_stream(kp + (int64_t)r * stride_t);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)kv[e];
        }
        float dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const h16 mean = mul_f32_then_h16(acc[e], inv);   // chunk mean: fp32 product, then fp16 (cache.py:154)
            dot = fmaf(qf[e], (float)mean, dot);
        }
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        if (li == 0) scores[(int64_t)h * C + c] = (h16)dot;
    }
}

// ---- chunk-mean index (opt-in: RetrievalCache(index=True)) ----------------
// The scorer above spends its time re-reading K for means that never change.  The index keeps them: index[h][c][d] =
// fp16(mean of chunk c), written once per chunk by chunk_mean_kernel and extended as the covered region grows, so a
// rebuild scores from chunk-size times fewer bytes.  Both kernels keep retrieval_score_kernel's lane ownership (lane li
// of a group owns d = 8 li .. 8 li + 7), its row-order fp32 sum, its fmaf element order and its xor-shuffle reduction:
// index + indexed score is bit-identical to the one-pass scorer over the same K.
template <int D>
__global__ __launch_bounds__(256) void chunk_mean_kernel(const h16* __restrict__ k, int64_t stride_t, int64_t stride_h,
                                                         h16* __restrict__ index, int64_t index_stride_h, int c0, int c1,
                                                         int chunk) {
    static_assert(D == 128 || D == 64, "head_dim");
    constexpr int LPR = D / 8;
    constexpr int GPB = 256 / LPR;
    const int h = blockIdx.y;
    const int grp = threadIdx.x / LPR, li = threadIdx.x % LPR;
    const h16* kb = k + (int64_t)h * stride_h + 8 * li;
    h16* ib = index + (int64_t)h * index_stride_h + 8 * li;
    const float inv = 1.0f / (float)chunk;
    for (int c = c0 + blockIdx.x * GPB + grp; c < c1; c += gridDim.x * GPB) {
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const h16* kp = kb + (int64_t)c * chunk * stride_t;
        for (int r = 0; r < chunk; ++r) {          // sequential fp32 accumulation over the chunk rows
            const half8 kv = load_half8_stream(kp + (int64_t)r * stride_t);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)kv[e];
        }
        half8 mean;
#pragma unroll
        for (int e = 0; e < 8; ++e) mean[e] = mul_f32_then_h16(acc[e], inv);
        store_half8(ib + (int64_t)c * D, mean);
    }
}

// Four chunks per group and trip: their loads are issued together (one 16-byte load per lane and chunk is all the memory
// work there is, so the loop is latency-bound otherwise); each chunk's arithmetic is the scorer's.
template <int D>
__global__ __launch_bounds__(256) void retrieval_score_indexed_kernel(const h16* __restrict__ index,
                                                                      int64_t index_stride_h, const h16* __restrict__ q,
                                                                      h16* __restrict__ scores, int C) {
    static_assert(D == 128 || D == 64, "head_dim");
    constexpr int LPR = D / 8;
    constexpr int GPB = 256 / LPR;
    constexpr int U = 4;
    const int h = blockIdx.y;
    const int grp = threadIdx.x / LPR, li = threadIdx.x % LPR;
    const h16* ib = index + (int64_t)h * index_stride_h + 8 * li;
    float qf[8];
    {
        const half8 qv = load_half8(q + (int64_t)h * D + 8 * li);
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[e] = (float)qv[e];
    }
    const int step = gridDim.x * GPB;
    for (int c = blockIdx.x * GPB + grp; c < C; c += U * step) {
        half8 m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int cu = c + u * step;
            if (cu < C) m[u] = load_half8_stream(ib + (int64_t)cu * D);
            else m[u] = half8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) dot = fmaf(qf[e], (float)m[u][e], dot);
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
            const int cu = c + u * step;
            if (li == 0 && cu < C) scores[(int64_t)h * C + cu] = (h16)dot;
        }
    }
}

// ---- per-head top-k: full bitonic sort of (score, chunk) keys in LDS ------------------------
__device__ __forceinline__ uint32_t sortable_fp16(uint32_t b) {
    return (b & 0x8000u) ? ((~b) & 0xFFFFu) : (b | 0x8000u);
}

__global__ __launch_bounds__(1024) void retrieval_topk_kernel(const uint16_t* __restrict__ scores,
                                                               int32_t* __restrict__ idx, int C, int sets,
                                                               int npow2) {
    extern __shared__ uint32_t keys[];
    const int h = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint16_t* sc = scores + (int64_t)h * C;
    // candidates are chunks 1..C-1; key = sortable(score) << 16 | (65535 - chunk): descending key
    // order == descending score, ascending chunk among equal scores.  Padding sorts last.
    for (int i = tid; i < npow2; i += nt) {
        const int c = i + 1;
        keys[i] = (c < C) ? ((sortable_fp16(sc[c]) << 16) | (uint32_t)(65535 - (c & 0xFFFF))) : 0u;
    }
    __syncthreads();
    for (int kk = 2; kk <= npow2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npow2; i += nt) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool desc = ((i & kk) == 0);
                    const uint32_t a = keys[i], b = keys[ixj];
                    if ((a < b) == desc) {
                        keys[i] = b;
                        keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    int32_t* out = idx + (int64_t)h * sets;
    if (tid == 0) out[0] = 0;
    for (int i = tid; i < sets - 1; i += nt) out[1 + i] = 65535 - (int32_t)(keys[i] & 0xFFFFu);
}

// ---- per-head top-k, select-then-sort form ---------------------------------------------------
// The keys are distinct 32-bit integers, so the m-th largest one is found EXACTLY by a 4-pass radix select
// (8 bits per pass, one 256-bin LDS histogram each, integer atomics: deterministic), the m keys >= it are compacted
// and only those are bitonic-sorted: for cfg2 (m = 511 of 15 615) 4 histogram passes + 45 passes over 512 keys
// instead of 105 passes over 16 384 keys (213 us -> ~25 us per layer).  Same output, bit for bit, as the full sort.
__global__ __launch_bounds__(1024) void retrieval_topk_select_kernel(const uint16_t* __restrict__ scores,
                                                                      int32_t* __restrict__ idx, int C, int sets,
                                                                      int n, int mpow2) {
    extern __shared__ uint32_t smem_u[];
    uint32_t* keys = smem_u;                 // [n]   candidate keys (chunks 1..C-1)
    uint32_t* sel = smem_u + n;              // [mpow2] the winners, then sorted in place
    __shared__ int hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_remaining, s_count;
    const int h = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const uint16_t* sc = scores + (int64_t)h * C;
    const int m = sets - 1;
    for (int i = tid; i < n; i += nt) {
        const int c = i + 1;
        keys[i] = (sortable_fp16(sc[c]) << 16) | (uint32_t)(65535 - (c & 0xFFFF));
    }
    for (int i = tid; i < mpow2; i += nt) sel[i] = 0u;                   // padding sorts last
    if (tid == 0) { s_prefix = 0u; s_remaining = m; s_count = 0; }
    __syncthreads();
    if (m > 0) {
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t pmask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const uint32_t prefix = s_prefix;
            for (int i = tid; i < n; i += nt) {
                const uint32_t k = keys[i];
                if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
            }
            __syncthreads();
            if (tid == 0) {                                              // digit of the remaining-th largest key
                int rem = s_remaining, b = 255, cum = 0;
                for (; b > 0; --b) {
                    if (cum + hist[b] >= rem) break;
                    cum += hist[b];
                }
                s_remaining = rem - cum;
                s_prefix = prefix | ((uint32_t)b << shift);
            }
            __syncthreads();
        }
        const uint32_t T = s_prefix;                                     // the m-th largest key (keys are distinct)
        for (int i = tid; i < n; i += nt) {
            const uint32_t k = keys[i];
            if (k >= T) {
                const int p = atomicAdd(&s_count, 1);
                if (p < mpow2) sel[p] = k;
            }
        }
        __syncthreads();
        for (int kk = 2; kk <= mpow2; kk <<= 1) {
            for (int j = kk >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < mpow2; i += nt) {
                    const int ixj = i ^ j;
                    if (ixj > i) {
                        const bool desc = ((i & kk) == 0);
                        const uint32_t a = sel[i], b = sel[ixj];
                        if ((a < b) == desc) {
                            sel[i] = b;
                            sel[ixj] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
    int32_t* out = idx + (int64_t)h * sets;
    if (tid == 0) out[0] = 0;
    for (int i = tid; i < m; i += nt) out[1 + i] = 65535 - (int32_t)(sel[i] & 0xFFFFu);
}

// ---- per-head top-k above 32 768 chunks: streamed radix select, ordered compaction, 64-bit sort ----------------------
// Neither the candidates (131 072 keys are 512 KiB) nor (score, chunk) in 32 bits fit any more, so nothing but the winners
// is held: one 1024-thread workgroup per head streams its score row from global memory three times (the whole [H][C] fp16
// array is a few MB and stays in L2 / Infinity Cache between the passes).
//   steps     the row is walked in STEPS of at most 8 192 entries in ascending chunk order: step 0 is the unaligned head
//             (chunks [1, a), scalar loads, one entry per lane), steps 1 .. nb the 16-byte-aligned body (one 16-byte load
//             of 8 consecutive scores per lane), the last step the tail (< 8 entries, scalar loads).  Row h starts at byte
//             2 h C: unaligned whenever C is not a multiple of 8.
//   threshold radix select on the 16-bit sortable pattern alone: pass one histograms its high byte, pass two the low byte
//             of the entries whose high byte matched; one private 256-bin LDS histogram per wave, folded after the pass
//             (integer counts: deterministic).  Gives T, the pattern of the m-th best entry, and r, how many entries equal
//             to T belong to the result.
//   compact   every entry above T is a winner (slot from an LDS counter: the winners are sorted afterwards); an entry
//             equal to T is one only while fewer than r of them were taken IN CHUNK ORDER: a workgroup-wide exclusive scan
//             of the per-lane tie counts per step plus the running total of the steps before.  This is what keeps
//             "ascending chunk among ties" exact when thousands of equal scores straddle the threshold.
//   sort      the m <= 8 192 winners as 64-bit keys pattern << 32 | (0xFFFFFFFF - chunk), padding 0 (sorts last: a real
//             key has a non-zero low word), bitonic, descending, in place.
constexpr int RTL_THREADS = 1024, RTL_WAVES = RTL_THREADS / TF_WAVE, RTL_VEC = 8;

struct RtlRow {                // how one head's row splits into steps
    const uint16_t* sc;        // the row (chunk 0 first)
    int a, nvec, t, C, nsteps; // body = chunks [a, t) in nvec vectors of 8; head [1, a), tail [t, C); nsteps = nb + 2
};

__device__ __forceinline__ RtlRow rtl_row(const uint16_t* sc, int C) {
    RtlRow r;
    r.sc = sc;
    r.C = C;
    const int to_aligned = (int)(((16u - (unsigned)((uintptr_t)(sc + 1) & 15u)) & 15u) >> 1);   // entries before a 16-byte bound
    r.a = min(1 + to_aligned, C);
    r.nvec = (C - r.a) / RTL_VEC;
    r.t = r.a + r.nvec * RTL_VEC;
    r.nsteps = (r.nvec + RTL_THREADS - 1) / RTL_THREADS + 2;
    return r;
}

// The entries of this lane in step s: n sortable patterns p[0 .. n) of the consecutive chunks c0, c0 + 1, ...; lanes in
// thread order hold ascending chunks.
__device__ __forceinline__ void rtl_load(const RtlRow& r, int s, int tid, uint32_t (&p)[RTL_VEC], int& n, int& c0) {
    n = 0;
    if (s == 0 || s == r.nsteps - 1) {
        c0 = (s == 0 ? 1 : r.t) + tid;
        if (c0 < (s == 0 ? r.a : r.C)) {
            p[0] = sortable_fp16(r.sc[c0]);
            n = 1;
        }
        return;
    }
    const int v = (s - 1) * RTL_THREADS + tid;
    c0 = r.a + v * RTL_VEC;
    if (v < r.nvec) {
        const uint4 w = *reinterpret_cast<const uint4*>(r.sc + c0);
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            p[2 * j] = sortable_fp16(ws[j] & 0xFFFFu);
            p[2 * j + 1] = sortable_fp16(ws[j] >> 16);
        }
        n = RTL_VEC;
    }
}

__global__ __launch_bounds__(RTL_THREADS) void retrieval_topk_large_kernel(const uint16_t* __restrict__ scores,
                                                                          int32_t* __restrict__ idx, int C, int sets,
                                                                          int mpow2) {
    extern __shared__ unsigned long long rtl_keys[];                     // [mpow2] the winners, then sorted in place
    __shared__ int hist[RTL_WAVES][256];
    __shared__ int wave_ties[RTL_WAVES];
    __shared__ int s_digit, s_remaining, s_count;
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & (TF_WAVE - 1), wave = tid / TF_WAVE;
    const RtlRow row = rtl_row(scores + (int64_t)h * C, C);
    const int m = sets - 1;
    int32_t* out = idx + (int64_t)h * sets;
    if (tid == 0) out[0] = 0;
    if (m == 0) return;
    for (int i = tid; i < mpow2; i += RTL_THREADS) rtl_keys[i] = 0ull;   // padding sorts last
    if (tid == 0) { s_remaining = m; s_count = 0; }
    uint32_t p[RTL_VEC];
    int n, c0;

    // ---- threshold: high byte, then low byte among the entries whose high byte matched ----
    uint32_t hi = 0u;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = tid; i < RTL_WAVES * 256; i += RTL_THREADS) (&hist[0][0])[i] = 0;
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < row.nsteps; ++s) {
            rtl_load(row, s, tid, p, n, c0);
#pragma unroll
            for (int j = 0; j < RTL_VEC; ++j)
                if (j < n) {
                    if (pass == 0) atomicAdd(&hist[wave][p[j] >> 8], 1);
                    else if ((p[j] >> 8) == hi) atomicAdd(&hist[wave][p[j] & 255u], 1);
                }
        }
        __syncthreads();
        if (tid < 256) {                                                 // fold the waves' histograms into wave 0's
            int sum = 0;
#pragma unroll
            for (int w = 0; w < RTL_WAVES; ++w) sum += hist[w][tid];
            hist[0][tid] = sum;
        }
        __syncthreads();
        if (tid == 0) {                                                  // digit of the remaining-th best entry
            int rem = s_remaining, b = 255, cum = 0;
            for (; b > 0; --b) {
                if (cum + hist[0][b] >= rem) break;
                cum += hist[0][b];
            }
            s_remaining = rem - cum;
            s_digit = b;
        }
        __syncthreads();
        if (pass == 0) hi = (uint32_t)s_digit;
    }
    const uint32_t T = (hi << 8) | (uint32_t)s_digit;                    // pattern of the m-th best entry
    const int r = s_remaining;                                           // entries equal to T that belong to the result, >= 1

    // ---- compaction, in ascending chunk order ----
    int taken = 0;                                                       // ties seen in the steps before (uniform)
#pragma unroll 1
    for (int s = 0; s < row.nsteps; ++s) {
        rtl_load(row, s, tid, p, n, c0);
        int ties = 0;
#pragma unroll
        for (int j = 0; j < RTL_VEC; ++j)
            if (j < n) {
                if (p[j] > T) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < mpow2)
                        rtl_keys[slot] = ((unsigned long long)p[j] << 32) | (0xFFFFFFFFu - (uint32_t)(c0 + j));
                } else if (p[j] == T) {
                    ++ties;
                }
            }
        if (taken >= r) continue;                                        // (uniform) every tie of the result is taken
        int inc = ties;
#pragma unroll
        for (int o = 1; o < TF_WAVE; o <<= 1) {
            const int up = __shfl_up(inc, o, TF_WAVE);
            if (lane >= o) inc += up;
        }
        __syncthreads();                                                 // (the step before has read wave_ties)
        if (lane == TF_WAVE - 1) wave_ties[wave] = inc;
        __syncthreads();
        int rank = taken + inc - ties, total = 0;                        // ties in front of this lane's, in chunk order
#pragma unroll
        for (int w = 0; w < RTL_WAVES; ++w) {
            const int t = wave_ties[w];
            if (w < wave) rank += t;
            total += t;
        }
        taken += total;
        if (ties > 0 && rank < r) {
#pragma unroll
            for (int j = 0; j < RTL_VEC; ++j)
                if (j < n && p[j] == T) {
                    if (rank < r) {
                        const int slot = atomicAdd(&s_count, 1);
                        if (slot < mpow2)
                            rtl_keys[slot] = ((unsigned long long)T << 32) | (0xFFFFFFFFu - (uint32_t)(c0 + j));
                    }
                    ++rank;
                }
        }
    }
    __syncthreads();

    // ---- sort the winners, descending ----
    for (int kk = 2; kk <= mpow2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < mpow2; i += RTL_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool desc = ((i & kk) == 0);
                    const unsigned long long a = rtl_keys[i], b = rtl_keys[ixj];
                    if ((a < b) == desc) {
                        rtl_keys[i] = b;
                        rtl_keys[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < m; i += RTL_THREADS) out[1 + i] = (int32_t)(0xFFFFFFFFu - (uint32_t)rtl_keys[i]);
}

// ---- gather ---------------------------------------------------------------------------------
// One 128-thread workgroup per (slot, head, K | V): a 2-KiB chunk, one 16-byte vector per thread.  In situ 24.9 us for the
// 134 MB (67 read + 67 written) of a cfg2 layer = 5.4 TB/s.  A coarser form — one workgroup per 8 slots, all chunk ids
// read first, 8 loads in flight per lane before the 8 stores — measured 26.0 us (round 3, bench.py roofline_stages on two
// boxes): the copy is bound by the mixed read / write stream, not by loads in flight; the simple form stays.
__global__ __launch_bounds__(128) void retrieval_gather_kernel(
    const h16* __restrict__ k_src, const h16* __restrict__ v_src, int64_t sst, int64_t ssh,
    const int32_t* __restrict__ idx, h16* __restrict__ k_dst, h16* __restrict__ v_dst, int64_t dst_t, int64_t dsh,
    int sets, int chunk, int D) {
    const int slot = blockIdx.x, h = blockIdx.y;
    const bool is_v = blockIdx.z != 0;
    const h16* src = (is_v ? v_src : k_src) + (int64_t)h * ssh;
    h16* dst = (is_v ? v_dst : k_dst) + (int64_t)h * dsh;
    const int c = idx[(int64_t)h * sets + slot];
    const int vec_per_row = D / 8;
    for (int e = threadIdx.x; e < chunk * vec_per_row; e += blockDim.x) {
        const int r = e / vec_per_row, dv = e - r * vec_per_row;
        const half8 x = load_half8(src + ((int64_t)c * chunk + r) * sst + 8 * dv);
        store_half8(dst + ((int64_t)slot * chunk + r) * dst_t + 8 * dv, x);
    }
}

// ---- row copies -----------------------------------------------------------------------------
// (blockIdx.z = 1: the second (src, dst) pair of the same geometry — K and V of one cache in one launch)
__global__ __launch_bounds__(256) void kv_copy_rows_kernel(const h16* __restrict__ src, int64_t ssl, int64_t sst,
                                                           int64_t ssh, h16* __restrict__ dst, int64_t dsl,
                                                           int64_t dst_t, int64_t dsh, int src_t0, int dst_t0, int n,
                                                           int H, int D, const h16* __restrict__ src2,
                                                           h16* __restrict__ dst2) {
    const int l = blockIdx.y / H, h = blockIdx.y % H;
    const h16* s = (blockIdx.z ? src2 : src) + (int64_t)l * ssl + (int64_t)h * ssh;
    h16* d = (blockIdx.z ? dst2 : dst) + (int64_t)l * dsl + (int64_t)h * dsh;
    const int vpr = D / 8;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * vpr; e += gridDim.x * blockDim.x) {
        const int r = e / vpr, dv = e - r * vpr;
        store_half8(d + (int64_t)(dst_t0 + r) * dst_t + 8 * dv, load_half8(s + (int64_t)(src_t0 + r) * sst + 8 * dv));
    }
}

// In-place downward shift (dst_t0 <= src_t0), overlap allowed: one workgroup per (layer, head)
// walks the rows in ascending blocks; inside a block every thread reads before anyone writes.
__global__ __launch_bounds__(256) void kv_shift_rows_kernel(h16* __restrict__ cache, int64_t sl, int64_t st,
                                                            int64_t sh, int src_t0, int dst_t0, int n, int H, int D,
                                                            h16* __restrict__ cache2) {
    const int l = blockIdx.x / H, h = blockIdx.x % H;
    h16* base = (blockIdx.y ? cache2 : cache) + (int64_t)l * sl + (int64_t)h * sh;
    const int vpr = D / 8;
    const int rows_per_blk = 256 / vpr;
    const int r_in = threadIdx.x / vpr, dv = threadIdx.x % vpr;
    for (int r0 = 0; r0 < n; r0 += rows_per_blk) {
        const int r = r0 + r_in;
        half8 x;
        const bool ok = (r < n) && (r_in < rows_per_blk);
        if (ok) x = load_half8(base + (int64_t)(src_t0 + r) * st + 8 * dv);
        __syncthreads();
        if (ok) store_half8(base + (int64_t)(dst_t0 + r) * st + 8 * dv, x);
        __syncthreads();
    }
}

// ---- C ABI ------------------------------------------------------------------------------------
extern "C" int tf_retrieval_score(const void* k, int64_t stride_t, int64_t stride_h, const void* q, void* scores,
                                  int C, int chunk, int H, int D, void* stream) {
    if (!k || !q || !scores || C < 1 || chunk < 1 || H < 1) return TF_EINVAL;
    if ((stride_t % 8) || (stride_h % 8)) return TF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int gx = rt_chunk_grid_x(C, H, D);          // (retrieval_rule.h: 8 resident workgroups per CU, grid-stride beyond)
    if (D == 128)
        hipLaunchKernelGGL((retrieval_score_kernel<128>), dim3(gx, H), dim3(256), 0, st, (const h16*)k, stride_t,
                           stride_h, (const h16*)q, (h16*)scores, C, chunk);
    else if (D == 64)
        hipLaunchKernelGGL((retrieval_score_kernel<64>), dim3(gx, H), dim3(256), 0, st, (const h16*)k, stride_t,
                           stride_h, (const h16*)q, (h16*)scores, C, chunk);
    else
        return TF_EINVAL;
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_chunk_mean(const void* k, int64_t stride_t, int64_t stride_h, void* index_layer, int64_t index_stride_h,
                             int c0, int c1, int chunk, int H, int D, void* stream) {
    if (!k || !index_layer || c0 < 0 || c1 < c0 || chunk < 1 || H < 1 || (D != 128 && D != 64)) return TF_EINVAL;
    if ((stride_t % 8) || (stride_h % 8) || (index_stride_h % 8) || index_stride_h < (int64_t)c1 * D) return TF_EINVAL;
    if (c1 == c0) return TF_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(rt_chunk_grid_x(c1 - c0, H, D), H);
    if (D == 128)
        hipLaunchKernelGGL((chunk_mean_kernel<128>), grid, dim3(256), 0, st, (const h16*)k, stride_t, stride_h,
                           (h16*)index_layer, index_stride_h, c0, c1, chunk);
    else
        hipLaunchKernelGGL((chunk_mean_kernel<64>), grid, dim3(256), 0, st, (const h16*)k, stride_t, stride_h,
                           (h16*)index_layer, index_stride_h, c0, c1, chunk);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_retrieval_score_indexed(const void* index_layer, int64_t index_stride_h, const void* q, void* scores,
                                          int C, int H, int D, void* stream) {
    if (!index_layer || !q || !scores || C < 1 || H < 1 || (D != 128 && D != 64)) return TF_EINVAL;
    if ((index_stride_h % 8) || index_stride_h < (int64_t)C * D) return TF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(rt_chunk_grid_x(C, H, D), H);
    if (D == 128)
        hipLaunchKernelGGL((retrieval_score_indexed_kernel<128>), grid, dim3(256), 0, st, (const h16*)index_layer,
                           index_stride_h, (const h16*)q, (h16*)scores, C);
    else
        hipLaunchKernelGGL((retrieval_score_indexed_kernel<64>), grid, dim3(256), 0, st, (const h16*)index_layer,
                           index_stride_h, (const h16*)q, (h16*)scores, C);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

// ORDER of tf_retrieval_topk: chunk 0 first, then the sets - 1 best candidates of [1, C) by fp16 BIT-PATTERN order
// (sortable_fp16: sign-magnitude, so -0 sorts below +0 and +NaN first, above +inf), ascending chunk among ties.  "Ties" means
// equal bit patterns: a (+0, -0) pair is NOT a tie.  That differs from IEEE equality (torch.topk sees the pair as equal) and
// is equally admissible against the reference, whose order among equal scores is unspecified.  Both kernels sort the same
// distinct 32-bit keys, so the form rt_topk_pick chooses never shows in the output.
extern "C" int tf_retrieval_topk(const void* scores, int32_t* idx, int C, int sets, int H, void* stream) {
    if (!scores || !idx || C < 2 || sets < 1 || sets > C || H < 1) return TF_EINVAL;
    if (C > 32768) return TF_ERANGE;
    const RtTopkPick pk = rt_topk_pick(C, sets);      // retrieval_rule.h: the form, its LDS, whether the attribute must be raised
    if (pk.form == RT_TOPK_SELECT) {
        if (pk.raise) {
            static bool raised_sel = false;
            if (!raised_sel) {
                hipError_t e = hipFuncSetAttribute((const void*)retrieval_topk_select_kernel,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk.raise_to);
                if (e != hipSuccess) return (int)e;
                raised_sel = true;
            }
        }
        hipLaunchKernelGGL(retrieval_topk_select_kernel, dim3(H), dim3(1024), pk.lds, (hipStream_t)stream,
                           (const uint16_t*)scores, idx, C, sets, C - 1, pk.mpow2);
        TF_LAUNCH_CHECK();
        return TF_OK;
    }
    if (pk.raise) {
        static bool raised = false;
        if (!raised) {
            hipError_t e = hipFuncSetAttribute((const void*)retrieval_topk_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk.raise_to);
            if (e != hipSuccess) return (int)e;
            raised = true;
        }
    }
    hipLaunchKernelGGL(retrieval_topk_kernel, dim3(H), dim3(1024), pk.lds, (hipStream_t)stream,
                       (const uint16_t*)scores, idx, C, sets, pk.npow2);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

// tf_retrieval_topk's contract, word for word, for 2 <= C <= 1 048 576 and sets - 1 <= 8 192 (retrieval_topk_large_kernel).
static_assert(TF_RETRIEVAL_TOPK_LARGE_MAX_CHUNKS == RT_LARGE_MAX_CHUNKS, "header macro and launch rule disagree");
extern "C" int tf_retrieval_topk_large(const void* scores, int32_t* idx, int C, int sets, int H, void* stream) {
    if (!scores || !idx || C < 2 || sets < 1 || sets > C || H < 1) return TF_EINVAL;
    if (C > RT_LARGE_MAX_CHUNKS || sets - 1 > RT_SELECT_MPOW2_MAX) return TF_ERANGE;
    const RtTopkLargePick pk = rt_topk_large_pick(C, sets);   // retrieval_rule.h: the LDS, whether the attribute must be raised
    if (pk.raise) {
        static bool raised_large = false;
        if (!raised_large) {
            hipError_t e = hipFuncSetAttribute((const void*)retrieval_topk_large_kernel,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk.raise_to);
            if (e != hipSuccess) return (int)e;
            raised_large = true;
        }
    }
    hipLaunchKernelGGL(retrieval_topk_large_kernel, dim3(H), dim3(RTL_THREADS), pk.lds, (hipStream_t)stream,
                       (const uint16_t*)scores, idx, C, sets, pk.mpow2);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_retrieval_gather(const void* k_src, const void* v_src, int64_t src_stride_t, int64_t src_stride_h,
                                   const int32_t* idx, void* k_dst, void* v_dst, int64_t dst_stride_t,
                                   int64_t dst_stride_h, int sets, int chunk, int H, int D, void* stream) {
    if (!k_src || !v_src || !idx || !k_dst || !v_dst || sets < 1 || chunk < 1 || H < 1 || (D % 8)) return TF_EINVAL;
    if ((src_stride_t % 8) || (src_stride_h % 8) || (dst_stride_t % 8) || (dst_stride_h % 8)) return TF_EINVAL;
    hipLaunchKernelGGL(retrieval_gather_kernel, dim3(sets, H, 2), dim3(128), 0, (hipStream_t)stream,
                       (const h16*)k_src, (const h16*)v_src, src_stride_t, src_stride_h, idx, (h16*)k_dst, (h16*)v_dst,
                       dst_stride_t, dst_stride_h, sets, chunk, D);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

// Compaction of accepted tree nodes (DistributedSimpleCache.gather_kv_incremental, models/cache.py:333-343):
// rows offset + idx[j] -> offset + j for j in [0, n), K and V, every layer and head.  idx must be strictly
// increasing (a root-to-leaf path of the Sequoia tree: node ids grow with depth), so idx[j] >= j and walking the
// rows in ascending batches with read-all / barrier / write-all is overlap-safe without the reference's clone().
__global__ __launch_bounds__(256) void kv_gather_rows_kernel(h16* __restrict__ kc, h16* __restrict__ vc, int64_t sl,
                                                             int64_t st, int64_t sh, int offset,
                                                             const int32_t* __restrict__ idx, int n, int H, int D) {
    const int l = blockIdx.x / H, h = blockIdx.x % H;
    h16* base = (blockIdx.y ? vc : kc) + (int64_t)l * sl + (int64_t)h * sh;
    const int vpr = D / 8;
    const int rows_per_blk = 256 / vpr;
    const int r_in = threadIdx.x / vpr, dv = threadIdx.x % vpr;
    for (int r0 = 0; r0 < n; r0 += rows_per_blk) {
        const int r = r0 + r_in;
        half8 x;
        const bool ok = (r < n) && (r_in < rows_per_blk);
        if (ok) x = load_half8(base + (int64_t)(offset + idx[r]) * st + 8 * dv);
        __syncthreads();
        if (ok) store_half8(base + (int64_t)(offset + r) * st + 8 * dv, x);
        __syncthreads();
    }
}

extern "C" int tf_kv_gather_rows(void* k_cache, void* v_cache, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                                 int offset, const int32_t* idx, int n, int L, int H, int D, void* stream) {
    if (!k_cache || !v_cache || !idx || n < 1 || offset < 0 || L < 1 || H < 1 || D < 8 || (D % 8) || D > 2048)
        return TF_EINVAL;
    hipLaunchKernelGGL(kv_gather_rows_kernel, dim3(L * H, 2), dim3(256), 0, (hipStream_t)stream, (h16*)k_cache,
                       (h16*)v_cache, stride_l, stride_t, stride_h, offset, idx, n, H, D);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

static int kv_copy_rows_launch(const void* src, const void* src2, int64_t src_stride_l, int64_t src_stride_t,
                               int64_t src_stride_h, void* dst, void* dst2, int64_t dst_stride_l, int64_t dst_stride_t,
                               int64_t dst_stride_h, int src_t0, int dst_t0, int n, int L, int H, int D, void* stream) {
    if (n == 0) return TF_OK;
    if (!src || !dst || n < 0 || L < 1 || H < 1 || (D % 8) || src_t0 < 0 || dst_t0 < 0) return TF_EINVAL;
    if ((src_stride_t % 8) || (src_stride_h % 8) || (src_stride_l % 8) || (dst_stride_t % 8) || (dst_stride_h % 8) ||
        (dst_stride_l % 8))
        return TF_EINVAL;
    const int gx = rt_copy_grid_x(n, D);
    hipLaunchKernelGGL(kv_copy_rows_kernel, dim3(gx, L * H, src2 ? 2 : 1), dim3(256), 0, (hipStream_t)stream,
                       (const h16*)src, src_stride_l, src_stride_t, src_stride_h, (h16*)dst, dst_stride_l, dst_stride_t,
                       dst_stride_h, src_t0, dst_t0, n, H, D, (const h16*)src2, (h16*)dst2);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_kv_copy_rows(const void* src, int64_t src_stride_l, int64_t src_stride_t, int64_t src_stride_h,
                               void* dst, int64_t dst_stride_l, int64_t dst_stride_t, int64_t dst_stride_h,
                               int src_t0, int dst_t0, int n, int L, int H, int D, void* stream) {
    return kv_copy_rows_launch(src, nullptr, src_stride_l, src_stride_t, src_stride_h, dst, nullptr, dst_stride_l,
                               dst_stride_t, dst_stride_h, src_t0, dst_t0, n, L, H, D, stream);
}

// K and V rows of one cache pair in ONE launch (same strides and row ranges for both): the decode step's tail copies
extern "C" int tf_kv_copy_rows_pair(const void* src_k, const void* src_v, int64_t src_stride_l, int64_t src_stride_t,
                                    int64_t src_stride_h, void* dst_k, void* dst_v, int64_t dst_stride_l,
                                    int64_t dst_stride_t, int64_t dst_stride_h, int src_t0, int dst_t0, int n, int L, int H,
                                    int D, void* stream) {
    if (n != 0 && (!src_v || !dst_v)) return TF_EINVAL;
    return kv_copy_rows_launch(src_k, src_v, src_stride_l, src_stride_t, src_stride_h, dst_k, dst_v, dst_stride_l,
                               dst_stride_t, dst_stride_h, src_t0, dst_t0, n, L, H, D, stream);
}

static int kv_shift_rows_launch(void* cache, void* cache2, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                                int src_t0, int dst_t0, int n, int L, int H, int D, void* stream) {
    if (n == 0 || src_t0 == dst_t0) return TF_OK;
    if (!cache || n < 0 || L < 1 || H < 1 || (D % 8) || D > 2048 || dst_t0 > src_t0 || dst_t0 < 0) return TF_EINVAL;
    if ((stride_t % 8) || (stride_h % 8) || (stride_l % 8)) return TF_EINVAL;
    hipLaunchKernelGGL(kv_shift_rows_kernel, dim3(L * H, cache2 ? 2 : 1), dim3(256), 0, (hipStream_t)stream, (h16*)cache,
                       stride_l, stride_t, stride_h, src_t0, dst_t0, n, H, D, (h16*)cache2);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_kv_shift_rows(void* cache, int64_t stride_l, int64_t stride_t, int64_t stride_h, int src_t0,
                                int dst_t0, int n, int L, int H, int D, void* stream) {
    return kv_shift_rows_launch(cache, nullptr, stride_l, stride_t, stride_h, src_t0, dst_t0, n, L, H, D, stream);
}

extern "C" int tf_kv_shift_rows_pair(void* k_cache, void* v_cache, int64_t stride_l, int64_t stride_t, int64_t stride_h,
                                     int src_t0, int dst_t0, int n, int L, int H, int D, void* stream) {
    if (n != 0 && src_t0 != dst_t0 && !v_cache) return TF_EINVAL;
    return kv_shift_rows_launch(k_cache, v_cache, stride_l, stride_t, stride_h, src_t0, dst_t0, n, L, H, D, stream);
}
