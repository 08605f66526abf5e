// tf_topp_probs_large / tf_topk_topp_probs_large: temperature (+ top-k) + top-p + softmax for vocabularies up to 262 144
// (DESIGN section 26).  The contract and the arithmetic are those of tf_topp_probs / tf_topk_topp_probs (csrc/sampling.hip,
// include/triforce_hip.h): x = l / T, the top-k survivors by key, e = expf(x - max), masses as 2^-40 fixed-point integers, Z and
// tau = floor(top_p * Z) exact, the boundary by a 3-round radix select on mass, ties at the boundary in index order, e / Zk.
// Every helper that decides a bit is the one csrc/sampling.hip uses (topp_select.h), so for V <= 32768 the output is
// bit-identical to those kernels.
//
// Form: ONE workgroup of 1 024 threads per row, as there; what changes is where the row lives.  128 - 256 entries per thread
// fit neither registers nor LDS, so the row is STREAMED: x, then e, are kept in the caller's workspace (4 bytes per entry, read
// and written by the thread that owns the entry with 16-byte accesses: L2 / Infinity Cache traffic, no ordering question), and
// the few entries that can hold the boundary (e >= cut, the candidate rule of topp_probs_kernel) are compacted into a second
// workspace list so that rounds 2 and 3 of the select visit the candidates only.  No workgroup hands anything to another one:
// there is no flag, no ticket and no cross-workgroup reduction, every sum is an LDS integer, and the workspace carries no state
// from one launch to the next (the list length lives in LDS), so back-to-back graph replays need no clearing.
#include "topp_select.h"

#define TOPP_LARGE_MAX_V TF_TOPP_LARGE_MAX_VOCAB
#define TOPP_LARGE_MAX_ROWS 32
static_assert(TF_TOPP_LARGE_WS_BYTES(1, 1) == 2 * 4096 * 4, "workspace: two padded float rows per row of logits");

struct ToppLargeShared {
    ToppShared s;
    unsigned nlist;                                // candidates in the workspace list
};

// the 4 entries thread-slab (s, tid) owns, entries past V as -inf (exp(-inf) = 0 mass)
__device__ __forceinline__ f32x4 tl_load4(const float* __restrict__ lr, int i0, int V, bool vec) {
    f32x4 a = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    if (vec) {
        if (i0 < V) a = *reinterpret_cast<const f32x4*>(lr + i0);      // V % 4 == 0: a float4 never straddles the end
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < V) a[j] = lr[i0 + j];
    }
    return a;
}

// list[nlist ...] <- v of the active lanes (wave-uniform call); the order inside the list is irrelevant: it only feeds integer
// histograms
__device__ __forceinline__ void tl_list_push(ToppLargeShared* sh, float* __restrict__ list, bool active, float v, int lane) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    unsigned base = 0u;
    if (lane == __ffsll((long long)act) - 1) base = atomicAdd(&sh->nlist, (unsigned)__popcll(act));
    base = (unsigned)__shfl((int)base, __ffsll((long long)act) - 1, 64);
    if (active) list[base + (unsigned)__popcll(act & ((1ull << lane) - 1ull))] = v;
}

// One round of the mass select over the candidate list: hist[digit(e)] += mass(e) for the candidates under `prefix`.
//   ROUND 2: candidates with (bits >> 20) == prefix, digit = bits 19..10      ROUND 3: (bits >> 10) == prefix, bits 9..0 (+ counts)
template <int ROUND>
__device__ __forceinline__ void tl_list_round(ToppLargeShared* sh, const float* __restrict__ list, unsigned n, unsigned prefix,
                                              int tid) {
    for (unsigned base = (unsigned)(tid & ~63); base < n; base += TOPP_THREADS) {          // wave-uniform trip count
        const unsigned i = base + (unsigned)(tid & 63);
        const bool has = i < n;
        const float xv = has ? list[i] : 0.f;
        const unsigned b = __float_as_uint(xv);
        const bool in = has && (b >> (ROUND == 2 ? 20 : 10)) == prefix;
        topp_hist_add(&sh->s, in, (int)((ROUND == 2 ? (b >> 10) : b) & 1023u), in ? topp_fix(xv) : 0ull, ROUND == 3);
    }
}

// MINP = true: tf_minp_probs_large (the rule is stated at topp_probs_body, csrc/sampling.hip) — behind the
// select, K' = { i in K : bits(e_i) >= umin = bits(min_p) }.  umin <= ustar changes nothing; otherwise Zk' is one more exact
// integer sum: over the candidate list when umin is at or above the candidate cut (every kept entry with mass is in the list),
// else over one more streamed pass of the row.  Everything new sits under `if constexpr (MINP)`.  The MINP instances and their
// entry are compiled from this file by csrc/minp_large.hip (TOPP_LARGE_MINP_ENTRY): built next to them in one translation
// unit, topp_large_kernel<true, false> came out with another schedule than it had before (the guard).
// MinP is the pack (float) in the MINP instances and empty otherwise: the MINP = false instances keep the argument list, and with
// it the instruction stream, they had before min-p existed.
__device__ __forceinline__ float tl_min_p() { return 0.f; }
__device__ __forceinline__ float tl_min_p(float min_p) { return min_p; }

template <bool TOPK, bool MINP, typename... MinP>
__global__ __launch_bounds__(TOPP_THREADS) void topp_large_kernel(const float* __restrict__ logits, float* __restrict__ probs,
                                                                  float* __restrict__ ws, int V, float temperature, int top_k,
                                                                  float top_p, MinP... min_p) {
    static_assert(sizeof...(MinP) == (MINP ? 1 : 0), "min_p is an argument of the MINP instances only");
    __shared__ ToppLargeShared lsh;
    ToppShared* sh = &lsh.s;
    const int nslab = (V + 4095) >> 12;                                 // <= 64 slabs of 4 096 entries
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lr = logits + (int64_t)row * V;
    float* pr = probs + (int64_t)row * V;
    // workspace of the row: [ x / e : nslab * 4096 floats | candidate list : nslab * 4096 floats ], 16-byte aligned
    float* rowe = ws + (int64_t)row * 2 * nslab * 4096;
    float* list = rowe + (int64_t)nslab * 4096;
    // thread t owns entries 4096 s + 4 t + j (s < nslab, j < 4) — the ownership and the index order (s, t, j) of
    // topp_probs_kernel: only the tie ranking at the boundary ever needs the order
    const bool vec = (V % 4) == 0 && ((reinterpret_cast<uintptr_t>(lr) | reinterpret_cast<uintptr_t>(pr)) & 15) == 0;
    f32x4* mine = reinterpret_cast<f32x4*>(rowe) + tid;                  // slab s at mine[1024 * s]

    // ---- pass 0: x = l / T (sampling.py:56) -> workspace, row max; 4 slabs of loads in flight ----
    float mx = -INFINITY;
#pragma unroll 1
    for (int s0 = 0; s0 < nslab; s0 += 4) {
        f32x4 a[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            a[k] = (s0 + k < nslab) ? tl_load4(lr, 4096 * (s0 + k) + 4 * tid, V, vec)
                                    : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (s0 + k < nslab) {
                f32x4 x;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[j] = a[k][j] / temperature;
                    mx = fmaxf(mx, x[j]);
                }
                mine[1024 * (s0 + k)] = x;
            }
        }
    }
    if (TOPK) {
        unsigned* w = reinterpret_cast<unsigned*>(sh->hist);           // every word: the count histogram uses the pad slots too
        for (int i = tid; i < 2 * (TOPP_BINS + TOPP_BINS / 16); i += TOPP_THREADS) w[i] = 0u;
        if (tid == 0) sh->krem = (unsigned)top_k;                       // 1 <= top_k < V (the host routes top_k >= V to TOPK = false)
    } else {
        sh->hist[TOPP_HB(tid)] = 0ull;
    }
    sh->cnt[TOPP_HB(tid)] = 0u;
    if (tid == 0) lsh.nlist = 0u;
    mx = block_max_1024(mx, sh->red, tid);

    // ---- top-k: the key of the top_k-th largest x (with multiplicity); survivors are the entries with key >= kthkey ----
    unsigned kthkey = 0u;
    if (TOPK) {
        unsigned* kc = reinterpret_cast<unsigned*>(sh->hist);
        unsigned pre = 0u;
#pragma unroll 1
        for (int r = 0; r < 3; ++r) {
            const int shift = r == 0 ? 21 : (r == 1 ? 10 : 0);          // digits: bits 31..21, 20..10, 9..0
            const unsigned dmask = r == 2 ? 1023u : 2047u;
#pragma unroll 1
            for (int s = 0; s < nslab; ++s) {
                const f32x4 x = mine[1024 * s];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned key = topk_key(x[j]);
                    // entries past V count nowhere (their -inf would otherwise compete with a real -inf logit)
                    const bool in = 4096 * s + 4 * tid + j < V && (r == 0 || (key >> (shift + (r == 1 ? 11 : 10))) == pre);
                    topk_cnt_add(kc, in, (int)((key >> shift) & dmask));
                }
            }
            __syncthreads();
            if (wave == 0) topk_scan(sh, kc, lane);
            __syncthreads();
            pre = (pre << (r == 2 ? 10 : 11)) | (unsigned)sh->kdigit;
        }
        kthkey = pre;
    }

    // ---- round 1: e = exp(x - max) back to the workspace; Z from every entry; mass histogram over bits 29..20 of the
    //      CANDIDATES (e >= cut, the rule and the cut of topp_probs_kernel), which are also compacted into `list` ----
    unsigned cutpat = 0u;
    if (top_p < 1.0f) cutpat = __float_as_uint((1.0f - top_p) / (2.0f * (float)V)) & ~((1u << 20) - 1u);
    unsigned long long zacc = 0ull;
#pragma unroll 1
    for (int s = 0; s < nslab; ++s) {
        f32x4 x = mine[1024 * s];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool out = TOPK && topk_key(x[j]) < kthkey;          // below the k-th value: zero mass from here on
            x[j] = out ? 0.f : expf(x[j] - mx);
        }
        mine[1024 * s] = x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long m = topp_fix(x[j]);
            zacc += m;
            const bool c = m != 0ull && __float_as_uint(x[j]) >= cutpat;
            tl_list_push(&lsh, list, c, x[j], lane);
            topp_hist_add(sh, c, (int)(__float_as_uint(x[j]) >> 20), m, false);
        }
    }
    {
        const unsigned long long zw = wave_sum_u64(zacc);
        if (lane == 0) sh->zpart[wave] = zw;
    }
    __syncthreads();
    if (wave == 0) topp_scan(sh, lane, true, false, top_p);
    __syncthreads();
    if (sh->digit == -2) {                                       // block-uniform; unreachable for the cut above (kept as
        __syncthreads();                                         // the exact fallback): histogram and list of ALL entries
        if (tid == 0) lsh.nlist = 0u;
        __syncthreads();
#pragma unroll 1
        for (int s = 0; s < nslab; ++s) {
            const f32x4 x = mine[1024 * s];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long m = topp_fix(x[j]);
                tl_list_push(&lsh, list, m != 0ull, x[j], lane);
                topp_hist_add(sh, m != 0ull, (int)(__float_as_uint(x[j]) >> 20), m, false);
            }
        }
        __syncthreads();
        if (wave == 0) topp_scan(sh, lane, true, false, top_p);
        __syncthreads();
    }
    const int d1 = sh->digit;
    const unsigned nlist = lsh.nlist;                            // (the barriers above also order the list's stores)
    unsigned ustar = 0u, ties = 0u;
    unsigned long long nkeep = 0ull;
    if (d1 >= 0) {                                               // block-uniform; -1: top_p >= 1 keeps everything
        // ---- round 2: bits 19..10 of the candidates inside the boundary bin ----
        tl_list_round<2>(&lsh, list, nlist, (unsigned)d1, tid);
        __syncthreads();
        if (wave == 0) topp_scan(sh, lane, false, false, top_p);
        __syncthreads();
        const unsigned pre = ((unsigned)d1 << 10) | (unsigned)sh->digit;
        // ---- round 3: bits 9..0, with tie counts ----
        tl_list_round<3>(&lsh, list, nlist, pre, tid);
        __syncthreads();
        if (wave == 0) topp_scan(sh, lane, false, true, top_p);
        __syncthreads();
        ustar = (pre << 10) | (unsigned)sh->digit;
        ties = sh->ties;
        nkeep = sh->nkeep;
    }
    unsigned long long zk = sh->zk;
    bool minp_cut = false;                                       // min-p is the tighter filter (block-uniform)
    unsigned umin = 0u;
    if constexpr (MINP) {
        umin = __float_as_uint(tl_min_p(min_p...));              // 0 < min_p <= 1: patterns order like values
        minp_cut = d1 < 0 || umin > ustar;
        if (minp_cut) {
            unsigned long long acc = 0ull;
            if (umin >= cutpat) {                                // block-uniform: the list holds every entry with mass >= the cut
                for (unsigned i = (unsigned)tid; i < nlist; i += TOPP_THREADS) {
                    const float xv = list[i];
                    if (__float_as_uint(xv) >= umin) acc += topp_fix(xv);
                }
            } else {
                // umin below the cut: one more streamed pass.  (With the cut derived above, ustar >= cutpat, and top_p >= 1 has
                // cutpat = 0: like digit == -2 this is the exact fallback, not a path any row takes.)
#pragma unroll 1
                for (int s = 0; s < nslab; ++s) {
                    const f32x4 x = mine[1024 * s];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (__float_as_uint(x[j]) >= umin) acc += topp_fix(x[j]);
                }
            }
            const unsigned long long zw = wave_sum_u64(acc);
            if (lane == 0) sh->zpart[wave] = zw;                 // (last read by the first scan, barriers ago)
            __syncthreads();
            zk = 0ull;
#pragma unroll
            for (int w = 0; w < TOPP_THREADS / 64; ++w) zk += sh->zpart[w];      // exact integers: any order
        }
    }
    const float Zk = (float)((double)zk * (1.0 / 1099511627776.0));
    // kept: everything above the boundary pattern, and the first nkeep entries equal to it in INDEX order.  Usually
    // nkeep == ties (one entry carries the boundary value); otherwise the ties are ranked slab by slab with a
    // block-wide exclusive scan (block-uniform branch).
    const bool rank_ties = !(MINP && minp_cut) && d1 >= 0 && nkeep < (unsigned long long)ties;
    const unsigned ulow = (MINP && minp_cut) ? umin                             // min-p: a plain threshold, no ties to rank
                          : d1 < 0 ? 0u : (rank_ties ? ustar + 1u : ustar);     // patterns >= ulow stay unconditionally
    int basecnt = 0;
#pragma unroll 1
    for (int s = 0; s < nslab; ++s) {
        const f32x4 x = mine[1024 * s];
        unsigned tiekeep = 0u;
        if (rank_ties) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) c += (__float_as_uint(x[j]) == ustar) ? 1 : 0;
            int inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int n = __shfl_up(inc, o, 64);
                if (lane >= o) inc += n;
            }
            __syncthreads();
            if (lane == 63) sh->red_i[wave] = inc;
            __syncthreads();
            int rank = basecnt + inc - c, total = 0;
#pragma unroll
            for (int w = 0; w < TOPP_THREADS / 64; ++w) {
                const int t = sh->red_i[w];
                if (w < wave) rank += t;
                total += t;
            }
            basecnt += total;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (__float_as_uint(x[j]) == ustar) {
                    if ((unsigned long long)rank < nkeep) tiekeep |= 1u << j;
                    ++rank;
                }
        }
        const int i0 = 4096 * s + 4 * tid;
        unsigned keep = tiekeep;
#pragma unroll
        for (int j = 0; j < 4; ++j) keep |= (__float_as_uint(x[j]) >= ulow ? 1u : 0u) << j;
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (__ballot(keep != 0u)) {                              // a peaked row keeps nothing in most slabs: no division there
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = ((keep >> j) & 1u) ? x[j] / Zk : 0.f;
        }
        if (vec) {
            if (i0 < V) *reinterpret_cast<f32x4*>(pr + i0) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < V) pr[i0 + j] = o[j];
        }
    }
}

static int topp_large_gates(const float* logits, const float* probs, int rows, int V, float temperature, float top_p,
                            const void* ws, int64_t ws_bytes) {
    if (!logits || !probs || !ws || rows < 1 || rows > TOPP_LARGE_MAX_ROWS || V < 1 || !(temperature > 0.f) || !(top_p > 0.f))
        return TF_EINVAL;
    if (reinterpret_cast<uintptr_t>(ws) & 15) return TF_EINVAL;         // the workspace is read and written 16 bytes at a time
    if (V > TOPP_LARGE_MAX_V) return TF_ERANGE;
    if (ws_bytes < TF_TOPP_LARGE_WS_BYTES(rows, V)) return TF_ENOSPC;
    return TF_OK;
}

#ifndef TOPP_LARGE_MINP_ENTRY
extern "C" int tf_topp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, float top_p,
                                   void* ws, int64_t ws_bytes, void* stream) {
    const int rc = topp_large_gates(logits, probs, rows, V, temperature, top_p, ws, ws_bytes);
    if (rc) return rc;
    hipLaunchKernelGGL((topp_large_kernel<false, false>), dim3(rows), dim3(TOPP_THREADS), 0, (hipStream_t)stream, logits, probs,
                       static_cast<float*>(ws), V, temperature, 0, top_p);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

// top_k >= V filters nothing: that call IS tf_topp_probs_large, so its output is bit-identical by construction.
extern "C" int tf_topk_topp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, int top_k,
                                        float top_p, void* ws, int64_t ws_bytes, void* stream) {
    if (top_k < 1) return TF_EINVAL;
    const int rc = topp_large_gates(logits, probs, rows, V, temperature, top_p, ws, ws_bytes);
    if (rc) return rc;
    if (top_k >= V) return tf_topp_probs_large(logits, probs, rows, V, temperature, top_p, ws, ws_bytes, stream);
    hipLaunchKernelGGL((topp_large_kernel<true, false>), dim3(rows), dim3(TOPP_THREADS), 0, (hipStream_t)stream, logits, probs,
                       static_cast<float*>(ws), V, temperature, top_k, top_p);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

#else   // csrc/minp_large.hip: the MINP instances are built as a translation unit of their own
// top_k <= 0 or top_k >= V means no top-k filter: the TOPK = false instance.
extern "C" int tf_minp_probs_large(const float* logits, float* probs, int rows, int V, float temperature, int top_k,
                                   float top_p, float min_p, void* ws, int64_t ws_bytes, void* stream) {
    if (!(min_p > 0.f) || min_p > 1.f) return TF_EINVAL;
    const int rc = topp_large_gates(logits, probs, rows, V, temperature, top_p, ws, ws_bytes);
    if (rc) return rc;
    if (top_k >= 1 && top_k < V)
        hipLaunchKernelGGL((topp_large_kernel<true, true, float>), dim3(rows), dim3(TOPP_THREADS), 0, (hipStream_t)stream, logits, probs,
                           static_cast<float*>(ws), V, temperature, top_k, top_p, min_p);
    else
        hipLaunchKernelGGL((topp_large_kernel<false, true, float>), dim3(rows), dim3(TOPP_THREADS), 0, (hipStream_t)stream, logits, probs,
                           static_cast<float*>(ws), V, temperature, 0, top_p, min_p);
    TF_LAUNCH_CHECK();
    return TF_OK;
}
#endif
