// Per-token log-probabilities of fp32 logits rows:
//   lp(r, t) = x[r][t] - max_i x[r][i] - log sum_i exp(x[r][i] - max_i x[r][i])
// the model's log-probability at temperature 1 with no top-k / top-p filter.  The sampling kernels (sampling.hip) hold a
// row in LDS or registers and stop at V = 32768; this one STREAMS the row — one pass, per-thread running maximum and
// rescaled sum — so it takes any V, any row stride and any number of rows.  One workgroup per row; wave reduction, then
// one LDS step across the waves; no atomics, no hand-off inside the launch, a fixed summation order (results are
// reproducible bit for bit).
#include "logprobs_row.h"

// use_ids: the row's target is ids.v[row] (rows <= 32, kernel arguments), else targets[row] (device memory, may be NULL).
// The walk, the fold and the value expression live in logprobs_row.h, shared with top_logprobs.hip.
__global__ __launch_bounds__(LP_THREADS) void token_logprobs_kernel(const float* __restrict__ logits, int64_t row_stride,
                                                                    const int64_t* __restrict__ targets, LpIds ids,
                                                                    int use_ids, int V, float* __restrict__ logprob,
                                                                    float* __restrict__ lse) {
    __shared__ float red_m[LP_WAVES];
    __shared__ float red_s[LP_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (int64_t)row * row_stride;
    float m = -INFINITY, s = 0.f;
    lp_for_each(x, V, tid, [&](f32x4 v, int) { lp_take4(v, m, s); }, [&](float v, int) { lp_take1(v, m, s); });
    float M, logS;
    if (lp_fold(m, s, red_m, red_s, lane, wave, M, logS)) {
        if (lse) lse[row] = M + logS;
        if (logprob) {
            const int64_t t = use_ids ? (int64_t)ids.v[row] : (targets ? targets[row] : (int64_t)-1);
            logprob[row] = lp_value(x, t, V, M, logS);                                       // outside [0, V): no target
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
