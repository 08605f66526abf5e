// Prompt-lookup n-gram draft (include/triforce_hip.h "N-GRAM DRAFT"): the draft tier without weights.
//   ctx = hist[0:L] ++ blk[0:m], T = L + m;  l(j) = longest n <= min(N, j + 1) with ctx[j - k] == ctx[T - 1 - k], k < n
//   j* = argmax (l(j), j) over 0 <= j <= T - 2;  d = ctx[j* + 1] when l(j*) >= 1, else ctx[T - 1];  q = one_hot(d)
// tf_ngram_draft is ONE launch of a fixed grid: every workgroup scans its share of the candidates j (16-byte loads of hist,
// grid-strided by groups of four), zero-fills its share of q (16-byte stores), publishes its best packed (l, j) with a 64-bit
// atomic max and takes a ticket; the workgroup that draws the last ticket reads the maximum, stores the 1.0 and info, and
// leaves key and ticket zero for the next launch — capturable, replayable back to back, no host read, nothing to zero.
// Ordering (attn.hip's fused merge, DESIGN section 12.1, in plain C++): a zero of q written on one XCD and the 1.0 written on
// another meet only in memory, so every thread releases its zero stores at agent scope (write-back + drain) BEFORE the
// barrier in front of the ticket, and the ticket itself is an acquire-release add; the last arriver's 1.0 is therefore behind
// every other workgroup's zero of that entry.  The zero-fill sits directly in front of the release on purpose: with stores
// outstanding the release's drain cannot be elided.
// tf_ngram_commit is the one writer of the history: one wave, outside every graph, after the step's host read.
#include "common.h"

#define NG_THREADS 256
#define NG_GRID 64                                 // fixed: 16 384 threads, 8 workgroups per XCD; 124 928 tokens = 2 groups per thread
#define NG_MAX_N 8
#define NG_MAX_BLK 32
#define NG_MAX_COMMIT 64

typedef int ng_i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool ng_valid(int c, int V) { return (unsigned)c < (unsigned)V; }

// ctx[i] as an int: an entry of blk that does not fit an int32 cannot be a token id and reads as -1
__device__ __forceinline__ int ng_ctx(const int32_t* __restrict__ hist, const int64_t* __restrict__ blk, int L, int i) {
    if (i < L) return hist[i];
    const int64_t t = blk[i - L];
    return (t >= 0 && t <= (int64_t)0x7fffffff) ? (int)t : -1;
}

__global__ __launch_bounds__(NG_THREADS) void ngram_draft_kernel(const int32_t* __restrict__ hist,
                                                                 const int32_t* __restrict__ len_dev,
                                                                 const int64_t* __restrict__ blk, int cap, int m, int N, int V,
                                                                 float* q, int32_t* __restrict__ info, unsigned long long* key,
                                                                 unsigned* ticket) {
    __shared__ int s_suf[NG_MAX_N];                                 // ctx[T - 1 - k], -1 where it matches nothing
    __shared__ unsigned long long s_best[NG_THREADS];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int gtid = blockIdx.x * NG_THREADS + tid, total = gridDim.x * NG_THREADS;
    int L = *len_dev;
    L = L < 0 ? 0 : (L > cap ? cap : L);
    const int T = L + m;
    if (tid < NG_MAX_N) {
        const int idx = T - 1 - tid;
        const int c = (tid < N && idx >= 0) ? ng_ctx(hist, blk, L, idx) : -1;
        s_suf[tid] = ng_valid(c, V) ? c : -1;
    }
    __syncthreads();
    const int suf0 = s_suf[0];
    unsigned long long best = 0;                                    // (l << 32) | j; 0 = no match (l >= 1 makes every key > 0)
    if (suf0 >= 0) {
        // candidates inside the history: j in [0, L), four per 16-byte load; j - k stays inside hist
        const int groups = (L + 3) >> 2;
        for (int g = gtid; g < groups; g += total) {
            const int j0 = g << 2;
            int c[4];
            if (j0 + 3 < cap) {
                const ng_i32x4 h = *reinterpret_cast<const ng_i32x4*>(hist + j0);
#pragma unroll
                for (int e = 0; e < 4; ++e) c[e] = h[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) c[e] = (j0 + e < cap) ? hist[j0 + e] : -1;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + e;
                if (j < L && c[e] == suf0) {
                    const int lim = N < j + 1 ? N : j + 1;
                    int l = 1;
                    while (l < lim && s_suf[l] >= 0 && hist[j - l] == s_suf[l]) ++l;
                    const unsigned long long k = ((unsigned long long)l << 32) | (unsigned)j;
                    best = k > best ? k : best;
                }
            }
        }
        // candidates inside the block: j in [L, T - 2], at most 31 of them, one thread each
        if (blockIdx.x == 0 && tid < m - 1) {
            const int j = L + tid;
            if (ng_ctx(hist, blk, L, j) == suf0) {
                const int lim = N < j + 1 ? N : j + 1;
                int l = 1;
                while (l < lim && s_suf[l] >= 0 && ng_ctx(hist, blk, L, j - l) == s_suf[l]) ++l;
                const unsigned long long k = ((unsigned long long)l << 32) | (unsigned)j;
                best = k > best ? k : best;
            }
        }
    }
    // q <- 0 whatever it held: scalar head up to the first 16-byte boundary, 16-byte body, scalar tail
    {
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(q) & 15u)) & 15u) >> 2);
        head = head > V ? V : head;
        const int nvec = (V - head) >> 2, tail0 = head + (nvec << 2);
        f32x4* q4 = reinterpret_cast<f32x4*>(q + head);
        const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = gtid; i < nvec; i += total) q4[i] = z;
        if (gtid < head) q[gtid] = 0.0f;
        if (gtid < V - tail0) q[tail0 + gtid] = 0.0f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");              // every thread: its zeros are in memory before the barrier
    s_best[tid] = best;
    __syncthreads();
    for (int o = NG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const unsigned long long a = s_best[tid], b = s_best[tid + o];
            s_best[tid] = a > b ? a : b;
        }
        __syncthreads();
    }
    if (tid == 0) {
        __hip_atomic_fetch_max(key, s_best[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = t == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || tid != 0) return;
    // the last arriver: every workgroup's key and zeros are behind its ticket
    const unsigned long long k = __hip_atomic_load(key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int l = (int)(k >> 32), j = (int)(k & 0xffffffffull);
    int d = ng_ctx(hist, blk, L, l >= 1 ? j + 1 : T - 1);           // (j <= T - 2; m >= 1 makes T >= 1)
    if (!ng_valid(d, V)) d = 0;
    q[d] = 1.0f;
    info[0] = d;
    info[1] = l;
    info[2] = l >= 1 ? j : -1;
    info[3] = T;
    __hip_atomic_store(key, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // left zero for the next launch (graph
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    //  replays included)
}

// hist[L + i] = (int32)src[i], i < n; L += n.  Every lane reads L before lane 0 rewrites it; L + n > cap writes nothing.
__global__ __launch_bounds__(NG_MAX_COMMIT) void ngram_commit_kernel(int32_t* hist, int32_t* len_dev,
                                                                     const int64_t* __restrict__ src, int cap, int n) {
    const int i = threadIdx.x;
    const int L = *len_dev;
    __syncthreads();
    if (L < 0 || L > cap - n) return;
    if (i < n) hist[L + i] = (int32_t)src[i];
    if (i == 0) *len_dev = L + n;
}

extern "C" int tf_ngram_draft_shape(int32_t* out) {
    if (!out) return TF_EINVAL;
    out[0] = NG_GRID * NG_THREADS;
    out[1] = 16;
    return TF_OK;
}

extern "C" int tf_ngram_draft(const int32_t* hist, int cap, const int32_t* len_dev, const int64_t* blk, int m, int N, int V,
                              float* q, int32_t* info, void* ws, void* stream) {
    if (!hist || !len_dev || !blk || !q || !info || !ws) return TF_EINVAL;
    if (cap < 1 || m < 1 || m > NG_MAX_BLK || N < 1 || N > NG_MAX_N || V < 1) return TF_EINVAL;
    if ((int64_t)cap + m > (int64_t)0x7fffffff) return TF_EINVAL;
    if ((reinterpret_cast<uintptr_t>(hist) & 15) || (reinterpret_cast<uintptr_t>(q) & 3) || (reinterpret_cast<uintptr_t>(ws) & 7))
        return TF_EINVAL;
    unsigned long long* key = reinterpret_cast<unsigned long long*>(ws);
    unsigned* ticket = reinterpret_cast<unsigned*>(key + 1);
    hipLaunchKernelGGL(ngram_draft_kernel, dim3(NG_GRID), dim3(NG_THREADS), 0, (hipStream_t)stream, hist, len_dev, blk, cap, m, N,
                       V, q, info, key, ticket);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_ngram_commit(int32_t* hist, int cap, int32_t* len_dev, const int64_t* src, int n, void* stream) {
    if (!hist || !len_dev || !src || cap < 1 || n < 0 || n > NG_MAX_COMMIT) return TF_EINVAL;
    if (n == 0) return TF_OK;
    hipLaunchKernelGGL(ngram_commit_kernel, dim3(1), dim3(NG_MAX_COMMIT), 0, (hipStream_t)stream, hist, len_dev, src, cap, n);
    TF_LAUNCH_CHECK();
    return TF_OK;
}
