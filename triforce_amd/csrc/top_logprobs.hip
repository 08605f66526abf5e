// Top-N alternatives and the emitted token's rank beside the per-token log-probability.  For every fp32
// logits row: the N <= 20 entries that come first in the order "value descending, then id ascending", each with its
// log-probability x - M - log S, and rank = 1 + #{entries in front of the row's target in that order}.
//
// One workgroup of 1024 threads per row, one launch, no global workspace, integer counting only (LDS integer adds commute:
// the result does not depend on the order in which waves arrive).  The order is decided on ORDER KEYS: the fp32 bit pattern
// mapped to a uint32 that sorts like the value, -0 folded onto +0 so that key equality is value equality.
//   walk 1   the single-value kernel's walk (logprobs_row.h: same (M, log S) bit for bit) + the two rank counters against
//            x[t].  Every thread's running maximum is one entry of the row, so the N-th largest of the 1024 thread maxima — a
//            four-round radix select over registers, no walk — is a LOWER BOUND T on the row's N-th largest entry.
//   walk 2   every entry with key >= T goes into an LDS candidate list of (~key, id) words (slot by an LDS counter; the
//            slot order is arbitrary and is erased below).  On rows without long ties that is N .. a few dozen entries.
//            A thread that is handed a slot past the list stops offering: only "more than TL_CAND" is used from then on.
//   order    candidate c's place is the number of candidates with a smaller 64-bit word (the words are distinct: the ids
//            are) — counted, not sorted; places < N are written.  Done in two walks.
//   overflow more than TL_CAND entries >= T (plateaus, the all-equal row): the N-th largest key K is found exactly by a
//            radix select over the row, 8 bits per walk, restricted to the digits in which T and the row maximum differ
//            (T <= K <= max; an all-equal row needs no walk at all).  One walk then lists the < N entries above K; the
//            entries equal to K are taken in id order — every wave counts them on a contiguous id range, a prefix over the
//            16 wave counts, and each wave writes those of its range that fall below the need.  At most 4 + 1 + 2 walks,
//            whatever N is.
#include "logprobs_row.h"

#define TL_MAX_N 20
#define TL_CAND 1024
#define TL_BINS 256

typedef unsigned long long u64;

__device__ __forceinline__ unsigned tl_key(float x) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;                                    // -0 == +0 as values: one key
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int tl_wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct TlShared {
    float red_m[LP_WAVES], red_s[LP_WAVES];
    float M, logS;
    int gt[LP_WAVES], eq[LP_WAVES];                                  // rank counters per wave; the tie counts per wave
    int hist[TL_BINS];
    int digit, want, count;
    u64 cand[TL_CAND];
};

// hist[] holds the digit counts of the keys still in play; the digit d of the `want`-th largest: count(digit > d) < want <=
// count(digit >= d); want -= count(digit > d).  Wave 0 scans (four bins a lane), everyone reads the answer.  Two barriers;
// the caller has one in front (after its adds).  A histogram with fewer than `want` keys leaves digit 0 (NaN rows only).
__device__ __forceinline__ void tl_pick_digit(TlShared& sh, int tid, int& digit, int& want) {
    if (tid < 64) {
        const int c0 = sh.hist[4 * tid], c1 = sh.hist[4 * tid + 1], c2 = sh.hist[4 * tid + 2], c3 = sh.hist[4 * tid + 3];
        const int own = c0 + c1 + c2 + c3;
        int suffix = own;                                            // sum over lanes >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_down(suffix, o, 64);
            if (tid + o < 64) suffix += up;
        }
        if (tid == 0) {
            sh.digit = 0;
            sh.want = 1;
        }
        int above = suffix - own;                                    // keys in higher bins than this lane's four
        if (above < want && want <= suffix) {                        // exactly one lane
            int d = 4 * tid + 3;
            const int c[4] = {c0, c1, c2, c3};
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                if (above + c[j] >= want) {
                    d = 4 * tid + j;
                    break;
                }
                above += c[j];
            }
            sh.digit = d;
            sh.want = want - above;
        }
    }
    __syncthreads();
    digit = sh.digit;
    want = sh.want;
    __syncthreads();
}

__device__ __forceinline__ void tl_clear_hist(TlShared& sh, int tid) {
    if (tid < TL_BINS) sh.hist[tid] = 0;
    __syncthreads();
}

__global__ __launch_bounds__(LP_THREADS) void token_top_logprobs_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                                        const int64_t* __restrict__ targets, LpIds ids,
                                                                        int use_ids, int V, int N, int* __restrict__ top_ids,
                                                                        float* __restrict__ top_lp, int* __restrict__ rank,
                                                                        float* __restrict__ lp) {
    __shared__ TlShared sh;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (int64_t)row * row_stride;
    const int n = min(N, V);                                         // places to fill; [n, N) are pads
    int64_t t = use_ids ? (int64_t)ids.v[row] : (targets ? targets[row] : (int64_t)-1);
    if (t < 0 || t >= (int64_t)V) t = -1;
    const bool ranked = (use_ids || targets) && t >= 0;
    const float xt = ranked ? x[t] : 0.f;
    const int ti = (int)t;

    // ---- walk 1: (m, s) exactly as token_logprobs_kernel, and the rank counters --------------------------------------------
    float m = -INFINITY, s = 0.f;
    int gt = 0, eq = 0;                                              // entries > x[t]; entries == x[t] with a lower id
    lp_for_each(
        x, V, tid,
        [&](f32x4 v, int id) {
            lp_take4(v, m, s);
            if (ranked) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    gt += v[j] > xt;
                    eq += (v[j] == xt) & (id + j < ti);
                }
            }
        },
        [&](float v, int id) {
            lp_take1(v, m, s);
            if (ranked) {
                gt += v > xt;
                eq += (v == xt) & (id < ti);
            }
        });
    if (tid < TL_BINS) sh.hist[tid] = 0;
    if (tid == 0) sh.count = 0;
    gt = tl_wave_sum_i(gt);
    eq = tl_wave_sum_i(eq);
    if (lane == 0) {
        sh.gt[wave] = gt;
        sh.eq[wave] = eq;
    }
    float M, logS;
    if (lp_fold(m, s, sh.red_m, sh.red_s, lane, wave, M, logS)) {    // (its barrier publishes gt / eq / hist / count too)
        sh.M = M;
        sh.logS = logS;
        if (lp) lp[row] = lp_value(x, t, V, M, logS);
        if (rank && (use_ids || targets)) {
            int before = 0;
            for (int w = 0; w < LP_WAVES; ++w) before += sh.gt[w] + sh.eq[w];
            rank[row] = ranked ? 1 + before : 0;
        }
    }
    __syncthreads();
    M = sh.M;
    logS = sh.logS;
    const unsigned kmax = tl_key(M);

    // ---- T: the n-th largest of the 1024 thread maxima (a thread without entries holds -inf, the lowest key: T only gets
    //      lower, never wrong) -------------------------------------------------------------------------------------------------
    const unsigned kmine = tl_key(m);
    unsigned T = 0;
    {
        int want = n;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (shift == 24 || (kmine >> (shift + 8)) == T) atomicAdd(&sh.hist[(kmine >> shift) & 255u], 1);
            __syncthreads();
            int d;
            tl_pick_digit(sh, tid, d, want);
            T = (T << 8) | (unsigned)d;
            tl_clear_hist(sh, tid);
        }
    }

    // ---- walk 2: the candidates ------------------------------------------------------------------------------------------
    bool over = false;                                               // this thread has seen the list overflow: the count
    //                                                                  is past TL_CAND for good, nothing more to offer
    auto offer = [&](float v, int id) {                               // one LDS add per wave and call, not per entry
        const unsigned k = tl_key(v);
        const bool hit = !over && k >= T;
        const u64 mask = __ballot(hit);                              // (over the lanes that are here)
        if (hit) {
            const int leader = __ffsll((long long)mask) - 1;
            int slot = 0;
            if (lane == leader) slot = atomicAdd(&sh.count, __popcll(mask));
            slot = __shfl(slot, leader, 64) + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot < TL_CAND) sh.cand[slot] = ((u64)(~k) << 32) | (unsigned)id;
            else over = true;
        }
    };
    lp_for_each(
        x, V, tid,
        [&](f32x4 v, int id) {
#pragma unroll
            for (int j = 0; j < 4; ++j) offer(v[j], id + j);
        },
        offer);
    __syncthreads();
    int total = sh.count;
    __syncthreads();

    if (total > TL_CAND) {                                           // (uniform over the workgroup)
        // ---- K: the n-th largest key of the row, digit by digit where T and the maximum differ --------------------------
        unsigned K = 0;
        int want = n;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if ((T >> shift) == (kmax >> shift)) {                       // T <= K <= kmax: the digits they share are K's
                K = T >> shift;
                continue;
            }
            int run_d = -1, run_c = 0;                               // a thread's run of equal digits is one add
            auto count = [&](float v, int) {
                const unsigned k = tl_key(v);
                if (shift != 24 && (k >> (shift + 8)) != K) return;
                const int d = (int)((k >> shift) & 255u);
                if (d != run_d) {
                    if (run_c) atomicAdd(&sh.hist[run_d], run_c);
                    run_d = d;
                    run_c = 0;
                }
                ++run_c;
            };
            lp_for_each(
                x, V, tid,
                [&](f32x4 v, int id) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) count(v[j], id + j);
                },
                count);
            if (run_c) atomicAdd(&sh.hist[run_d], run_c);
            __syncthreads();
            int d;
            tl_pick_digit(sh, tid, d, want);
            K = (K << 8) | (unsigned)d;
            tl_clear_hist(sh, tid);
        }
        const int above = n - want;                                  // entries with key > K: fewer than n; `want` ties follow
        if (tid == 0) sh.count = 0;
        __syncthreads();
        auto higher = [&](float v, int id) {
            const unsigned k = tl_key(v);
            if (k > K) {
                const int slot = atomicAdd(&sh.count, 1);
                if (slot < TL_CAND) sh.cand[slot] = ((u64)(~k) << 32) | (unsigned)id;
            }
        };
        lp_for_each(
            x, V, tid,
            [&](f32x4 v, int id) {
#pragma unroll
                for (int j = 0; j < 4; ++j) higher(v[j], id + j);
            },
            higher);
        // ---- the ties, lowest ids first: wave w owns ids [w * seg, (w + 1) * seg), lane-contiguous 64 at a time -------------
        const int seg = (((V + LP_WAVES - 1) / LP_WAVES) + 63) & ~63;
        const int lo = (int)min((int64_t)V, (int64_t)wave * seg), hi = (int)min((int64_t)V, (int64_t)lo + seg);
        int mine = 0;
        for (int base = lo; base < hi; base += 64) {
            const int id = base + lane;
            const bool is = id < hi && tl_key(x[id]) == K;
            mine += __popcll(__ballot(is));
        }
        if (lane == 0) sh.eq[wave] = mine;
        __syncthreads();
        int first = 0;                                               // ties in the waves before this one
        for (int w = 0; w < wave; ++w) first += sh.eq[w];
        for (int base = lo; base < hi && first < want; base += 64) {
            const int id = base + lane;
            const bool is = id < hi && tl_key(x[id]) == K;
            const u64 mask = __ballot(is);
            const int place = first + __popcll(mask & ((1ull << lane) - 1ull));
            if (is && place < want && above + place < TL_CAND) sh.cand[above + place] = ((u64)(~K) << 32) | (unsigned)id;
            first += __popcll(mask);
        }
        total = n;
        __syncthreads();
    }

    // ---- order by counting; write the first n places and the pads -------------------------------------------------------
    total = min(total, TL_CAND);
    if (tid < total) {
        const u64 e = sh.cand[tid];
        int place = 0;
        for (int j = 0; j < total; ++j) place += sh.cand[j] < e;
        if (place < n) {
            const int id = (int)(unsigned)(e & 0xffffffffull);
            const float v = x[id];
            top_ids[(int64_t)row * N + place] = id;
            top_lp[(int64_t)row * N + place] = v == -INFINITY ? -INFINITY : (v - M) - logS;
        }
    }
    if (tid >= n && tid < N) {
        top_ids[(int64_t)row * N + tid] = -1;
        top_lp[(int64_t)row * N + tid] = -INFINITY;
    }
}

static int tl_launch(const float* logits, int64_t row_stride, const int64_t* targets, const LpIds& ids, int use_ids, int rows,
                     int V, int N, int32_t* top_ids, float* top_lp, int32_t* rank, float* lp, void* stream) {
    hipLaunchKernelGGL(token_top_logprobs_kernel, dim3((unsigned)rows), dim3(LP_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, targets, ids, use_ids, V, N, top_ids, top_lp, rank, lp);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_token_top_logprobs(const float* logits, int64_t row_stride, const int64_t* targets, int rows, int V, int N,
                                     int32_t* top_ids, float* top_lp, int32_t* rank, float* lp, void* stream) {
    if (!logits || !top_ids || !top_lp || rows < 1 || V < 1 || row_stride < (int64_t)V || N < 1 || N > TL_MAX_N)
        return TF_EINVAL;
    if (targets ? !rank : (rank || lp)) return TF_EINVAL;            // rank goes with targets; lp needs them
    LpIds none = {};
    return tl_launch(logits, row_stride, targets, none, 0, rows, V, N, top_ids, top_lp, rank, lp, stream);
}

extern "C" int tf_token_top_logprobs_ids(const float* logits, int64_t row_stride, const int64_t* host_ids, int rows, int V,
                                         int N, int32_t* top_ids, float* top_lp, int32_t* rank, float* lp, void* stream) {
    if (!logits || !host_ids || !top_ids || !top_lp || !rank || rows < 1 || rows > LP_MAX_IDS || V < 1 ||
        row_stride < (int64_t)V || N < 1 || N > TL_MAX_N)
        return TF_EINVAL;
    LpIds a;
    for (int i = 0; i < LP_MAX_IDS; ++i)
        a.v[i] = (i < rows && host_ids[i] >= 0 && host_ids[i] < (int64_t)V) ? (int)host_ids[i] : -1;
    return tl_launch(logits, row_stride, nullptr, a, 1, rows, V, N, top_ids, top_lp, rank, lp, stream);
}
