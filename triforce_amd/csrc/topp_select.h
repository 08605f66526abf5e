// The exact top-k / top-p select shared by the one-workgroup-per-row normalisers: csrc/sampling.hip (topp_probs_kernel,
// topk_topp_probs_kernel: the row lives in LDS, V <= 32768) and csrc/topp_large.hip (the row streams through a workspace,
// V <= 262144).  Same helpers, same integers, hence the same bits: 2^-40 fixed-point masses, the order-preserving key of the
// top-k filter, the 1 024-bin mass histogram with its one-wave scan and the 2 048-bin count histogram with its one-wave scan.
// The arithmetic is described where it is used (csrc/sampling.hip, "Fused temperature + top-p + softmax").
#pragma once
#include "common.h"

#define TOPP_THREADS 1024
#define TOPP_SLABS 8                       // 16-byte slabs per thread: 8 * 4 * 1024 = 32768 entries
#define TOPP_EPT (4 * TOPP_SLABS)
#define TOPP_BINS 1024
#define TOPP_HB(b) ((b) + ((b) >> 4))      // one pad slot per 16 bins: the scan's 16-bins-per-lane reads spread over banks
#define TOPP_FIX_SHIFT 40                  // masses in units of 2^-40 (row total < 2^15 * 2^40)

struct ToppShared {
    unsigned long long hist[TOPP_BINS + TOPP_BINS / 16];
    unsigned cnt[TOPP_BINS + TOPP_BINS / 16];
    float red[TOPP_THREADS / 64];
    int red_i[TOPP_THREADS / 64];
    unsigned long long S, tau, nkeep, zk;
    unsigned long long zpart[TOPP_THREADS / 64];   // per-wave sums of all masses: Z does not come from the histogram
    unsigned ties;
    int digit;                                     // >= 0 boundary bin, -1 keep everything, -2 boundary below the candidate cut
    unsigned krem;                                 // top-k select: rank still looked for inside the current prefix
    int kdigit;                                    //               the bin the last count scan named
};

__device__ __forceinline__ float block_max_1024(float v, float* sm, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) sm[tid >> 6] = v;
    __syncthreads();
    float t = sm[0];
#pragma unroll
    for (int w = 1; w < TOPP_THREADS / 64; ++w) t = fmaxf(t, sm[w]);
    return t;
}

// floor(e * 2^40) for 0 <= e <= 1 straight from the bit pattern (monotone in e; 0 below 2^-40)
__device__ __forceinline__ unsigned long long topp_fix(float e) {
    const unsigned b = __float_as_uint(e);
    const int ex = (int)(b >> 23);
    const unsigned long long man = (unsigned long long)((b & 0x7FFFFFu) | 0x800000u);
    const int sh = ex - (127 + 23 - TOPP_FIX_SHIFT);
    if (ex == 0 || sh <= -24) return 0ull;
    return sh >= 0 ? (man << sh) : (man >> (-sh));
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// hist[digit] += m for the active lanes of a wave (wave-uniform call).  When more than 8 lanes are active and all of
// them name the same bin (degenerate rows: huge tie groups) the wave adds ONE pre-summed value instead of serialising up
// to 64 same-address atomics.
__device__ __forceinline__ void topp_hist_add(ToppShared* sh, bool active, int digit, unsigned long long m, bool count) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const int first = __ffsll((long long)act) - 1;
    const int dref = __shfl(digit, first, 64);
    if (__popcll(act) > 8 && __all(!active || digit == dref)) {
        const unsigned long long tot = wave_sum_u64(active ? m : 0ull);
        if ((int)(threadIdx.x & 63) == first) {
            atomicAdd(&sh->hist[TOPP_HB(dref)], tot);
            if (count) atomicAdd(&sh->cnt[TOPP_HB(dref)], (unsigned)__popcll(act));
        }
    } else if (active) {
        atomicAdd(&sh->hist[TOPP_HB(digit)], m);
        if (count) atomicAdd(&sh->cnt[TOPP_HB(digit)], 1u);
    }
}

// One wavefront scans the histogram from the top: lane l owns bins [16l, 16l+16).  Names the bin d with
//   S(d) <= tau < S(d) + mass(d),   S(d) = base + mass of the bins above d
// (sh->digit, sh->S = S(d)); no such bin (tau >= total: top_p >= 1) -> digit = -1.  The first round also fixes
// tau = floor(top_p * Z); the last round resolves the ties at the boundary pattern: the j-th tie (index order) is
// kept iff S + j * m <= tau.  Clears the bins it read for the next round.
__device__ __forceinline__ void topp_scan(ToppShared* sh, int lane, bool first_round, bool last_round, float top_p) {
    unsigned long long h[16];
    unsigned long long tot = 0ull;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        h[k] = sh->hist[TOPP_HB(16 * lane + k)];
        sh->hist[TOPP_HB(16 * lane + k)] = 0ull;
        tot += h[k];
    }
    unsigned long long inc = tot;                                   // inclusive suffix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned lo = (unsigned)__shfl_down((int)(unsigned)inc, o, 64);
        const unsigned hi = (unsigned)__shfl_down((int)(unsigned)(inc >> 32), o, 64);
        if (lane + o < 64) inc += ((unsigned long long)hi << 32) | lo;
    }
    unsigned long long base, tau, Z = 0ull;
    if (first_round) {
#pragma unroll
        for (int w = 0; w < TOPP_THREADS / 64; ++w) Z += sh->zpart[w];          // exact integers: any order
        const double t = (double)top_p * (double)Z;
        tau = (t >= 18446744073709549568.0) ? ~0ull : __double2ull_rd(t);
        base = 0ull;
        if (lane == 0) {
            sh->tau = tau;
            sh->zk = Z;
        }
    } else {
        base = sh->S;
        tau = sh->tau;
    }
    unsigned long long S = base + (inc - tot);
    int found = -1;
    unsigned long long Sf = 0ull, hf = 0ull;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        if (found < 0 && h[k] != 0ull && S <= tau && tau - S < h[k]) {
            found = k;
            Sf = S;
            hf = h[k];
        }
        S += h[k];
    }
    const unsigned long long hit = __ballot(found >= 0);
    if (!hit) {
        // nothing crossed: tau >= Z (top_p >= 1: keep everything) — or, first round only, the crossing lies among the
        // entries the candidate cut left out of the histogram (cannot happen for the cut topp_probs_kernel derives)
        if (lane == 0) sh->digit = (first_round && tau < Z) ? -2 : -1;
    } else if (found >= 0) {
        sh->digit = 16 * lane + found;
        sh->S = Sf;
        if (last_round) {
            const unsigned T = sh->cnt[TOPP_HB(16 * lane + found)];
            const unsigned long long m = hf / (unsigned long long)T;      // all ties share one pattern, hence one mass
            unsigned long long nk = (tau - Sf) / m + 1ull;
            if (nk > (unsigned long long)T) nk = T;
            sh->ties = T;
            sh->nkeep = nk;
            sh->zk = Sf + nk * m;
        }
    }
    if (last_round) {
#pragma unroll
        for (int k = 0; k < 16; ++k) sh->cnt[TOPP_HB(16 * lane + k)] = 0u;
    }
}

// ------------------------------------------------------------------------------------------------
// Top-k in front of the top-p select (tf_topk_topp_probs; reference utils/sampling.py:16-19: kth = topk(x, min(k, V))[-1],
// every x < kth masked to -inf — every entry TIED with the k-th value survives).  kth is found by a 3-round radix select
// (11 + 11 + 10 bits) over an order-preserving 32-bit key of x = l / T, on COUNT histograms in LDS: integers, so the
// result does not depend on the order in which the atomics land.  The 2 048 count bins live in ToppShared::hist viewed as
// 32-bit words (the mass histogram is not in use yet, and is left all-zero for it); lane l of the scanning wave owns bins
// [32 l, 32 l + 32), one pad word per 32 bins keeps the lanes' reads on different banks.
// ------------------------------------------------------------------------------------------------
#define TOPK_BINS 2048
#define TOPK_HB(b) ((b) + ((b) >> 5))
#define TOPK_WORDS (TOPK_BINS + TOPK_BINS / 32)
static_assert(TOPK_WORDS <= 2 * (TOPP_BINS + TOPP_BINS / 16), "the count histogram must fit in ToppShared::hist");

// bigger float -> bigger key; -0.0 and +0.0 share one key (they compare equal)
__device__ __forceinline__ unsigned topk_key(float x) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// cnt[digit] += 1 for the active lanes of a wave (wave-uniform call); a wave whose active lanes all name one bin (tie groups,
// the narrow exponent range of a row of logits) adds its lane count once
__device__ __forceinline__ void topk_cnt_add(unsigned* cnt, bool active, int digit) {
    const unsigned long long act = __ballot(active);
    if (!act) return;
    const int first = __ffsll((long long)act) - 1;
    const int dref = __shfl(digit, first, 64);
    if (__popcll(act) > 8 && __all(!active || digit == dref)) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&cnt[TOPK_HB(dref)], (unsigned)__popcll(act));
    } else if (active) {
        atomicAdd(&cnt[TOPK_HB(digit)], 1u);
    }
}

// One wavefront scans the count histogram from the top and names the bin d that holds the krem-th largest entry:
//   above(d) < krem <= above(d) + cnt(d),   above(d) = entries in the bins above d
// (sh->kdigit = d, sh->krem = krem - above(d): the rank inside the bin).  Clears the bins it read.
__device__ __forceinline__ void topk_scan(ToppShared* sh, unsigned* cnt, int lane) {
    unsigned h[32];
    unsigned tot = 0u;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        h[k] = cnt[TOPK_HB(32 * lane + k)];
        cnt[TOPK_HB(32 * lane + k)] = 0u;
        tot += h[k];
    }
    unsigned inc = tot;                                             // inclusive suffix sum over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned n = (unsigned)__shfl_down((int)inc, o, 64);
        if (lane + o < 64) inc += n;
    }
    const unsigned krem = sh->krem;
    unsigned above = inc - tot;
    int found = -1;
    unsigned af = 0u;
#pragma unroll
    for (int k = 31; k >= 0; --k) {
        if (found < 0 && above < krem && krem - above <= h[k]) {
            found = k;
            af = above;
        }
        above += h[k];
    }
    if (found >= 0) {                                               // exactly one lane: 1 <= krem <= entries counted
        sh->kdigit = 32 * lane + found;
        sh->krem = krem - af;
    }
}
