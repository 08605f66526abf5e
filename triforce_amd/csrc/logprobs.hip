// Per-token log-probabilities of fp32 logits rows:
//   lp(r, t) = x[r][t] - max_i x[r][i] - log sum_i exp(x[r][i] - max_i x[r][i])
// the model's log-probability at temperature 1 with no top-k / top-p filter.  The sampling kernels (sampling.hip) hold a
// row in LDS or registers and stop at V = 32768; this one STREAMS the row — one pass, per-thread running maximum and
// rescaled sum — so it takes any V, any row stride and any number of rows.  One workgroup per row; wave reduction, then
// one LDS step across the waves; no atomics, no hand-off inside the launch, a fixed summation order (results are
// reproducible bit for bit).
#include <math.h>
#include "common.h"

#define LP_THREADS 1024
#define LP_WAVES (LP_THREADS / 64)
#define LP_MAX_IDS 32

struct LpIds { int v[LP_MAX_IDS]; };

// running (max, sum of exp(x - max)) over the entries seen so far; m = -inf, s = 0 before the first finite entry
__device__ __forceinline__ void lp_take4(f32x4 v, float& m, float& s) {
    const float vm = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (vm > m) {                                                   // rare after the first few vectors of a thread
        s *= expf(m - vm);                                          // m = -inf: s is 0 and stays 0
        m = vm;
    }
    if (m > -INFINITY) {                                            // (all -inf so far: mass 0, and -inf - -inf is NaN)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += expf(v[j] - m);            // a -inf entry adds expf(-inf) = 0
    }
}

__device__ __forceinline__ void lp_take1(float x, float& m, float& s) {
    if (x > m) {
        s *= expf(m - x);
        m = x;
    }
    if (m > -INFINITY) s += expf(x - m);
}

// use_ids: the row's target is ids.v[row] (rows <= 32, kernel arguments), else targets[row] (device memory, may be NULL).
__global__ __launch_bounds__(LP_THREADS) void token_logprobs_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                                    const int64_t* __restrict__ targets, LpIds ids,
                                                                    int use_ids, int V, float* __restrict__ logprob,
                                                                    float* __restrict__ lse) {
    __shared__ float red_m[LP_WAVES];
    __shared__ float red_s[LP_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (int64_t)row * row_stride;
    // [0, head) scalar up to the first 16-byte boundary, then nvec aligned 16-byte loads, then [tail0, V) scalar: whatever
    // the base address and the stride are, all but at most six entries of a row travel in 16-byte loads
    const int head = min(V, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2));
    const int nvec = (V - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const f32x4* xv = reinterpret_cast<const f32x4*>(x + head);
    float m = -INFINITY, s = 0.f;
    int i = tid;
    for (; i + 3 * LP_THREADS < nvec; i += 4 * LP_THREADS) {        // four loads in flight per thread
        const f32x4 a = xv[i], b = xv[i + LP_THREADS], c = xv[i + 2 * LP_THREADS], d = xv[i + 3 * LP_THREADS];
        lp_take4(a, m, s);
        lp_take4(b, m, s);
        lp_take4(c, m, s);
        lp_take4(d, m, s);
    }
    for (; i < nvec; i += LP_THREADS) lp_take4(xv[i], m, s);
    if (tid < head) lp_take1(x[tid], m, s);
    if (tid < V - tail0) lp_take1(x[tail0 + tid], m, s);

    // wave: common maximum, sums rescaled to it
    const float wm = wave_max(m);
    const float ws = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    if (lane == 0) {
        red_m[wave] = wm;
        red_s[wave] = ws;
    }
    __syncthreads();
    if (wave == 0) {
        const float pm = lane < LP_WAVES ? red_m[lane] : -INFINITY;
        const float ps = lane < LP_WAVES ? red_s[lane] : 0.f;
        const float M = wave_max(pm);
        const float S = wave_sum(pm > -INFINITY ? ps * expf(pm - M) : 0.f);
        if (lane == 0) {
            const float logS = logf(S);
            if (lse) lse[row] = M + logS;
            if (logprob) {
                const int64_t t = use_ids ? (int64_t)ids.v[row] : (targets ? targets[row] : (int64_t)-1);
                logprob[row] = (t >= 0 && t < (int64_t)V) ? (x[t] - M) - logS : 0.f;     // outside [0, V): no target
            }
        }
    }
}

extern "C" int tf_token_logprobs(const float* logits, int64_t row_stride, const int64_t* targets, int rows, int V,
                                 float* logprob, float* lse, void* stream) {
    if (!logits || rows < 1 || V < 1 || row_stride < (int64_t)V) return TF_EINVAL;
    if (!((targets && logprob) || lse)) return TF_EINVAL;
    LpIds none = {};
    hipLaunchKernelGGL(token_logprobs_kernel, dim3((unsigned)rows), dim3(LP_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, targets, none, 0, V, logprob, lse);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_token_logprobs_ids(const float* logits, int64_t row_stride, const int64_t* host_ids, int rows, int V,
                                     float* logprob, float* lse, void* stream) {
    if (!logits || !host_ids || !logprob || rows < 1 || rows > LP_MAX_IDS || V < 1 || row_stride < (int64_t)V)
        return TF_EINVAL;
    LpIds a;
    for (int i = 0; i < LP_MAX_IDS; ++i)
        a.v[i] = (i < rows && host_ids[i] >= 0 && host_ids[i] < (int64_t)V) ? (int)host_ids[i] : -1;
    hipLaunchKernelGGL(token_logprobs_kernel, dim3((unsigned)rows), dim3(LP_THREADS), 0, (hipStream_t)stream, logits,
                       row_stride, (const int64_t*)nullptr, a, 1, V, logprob, lse);
    TF_LAUNCH_CHECK();
    return TF_OK;
}
