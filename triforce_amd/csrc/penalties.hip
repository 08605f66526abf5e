// Repetition, frequency and presence penalties on fp32 logits rows of the target tier:
//   c    = gen_count[t] + #{ j <= i : ids[j] == t }
//   seen = prompt_seen[t] != 0 || c > 0
//   y    = x;  seen && repetition != 1: y = x > 0 ? x / repetition : x * repetition;  c > 0: y = (y - frequency * c) - presence
// tf_penalize_logits is out of place and only READS the state: one launch over V in which a thread owns four vocabulary
// entries for ALL rows — it loads their counts and prompt flags once and walks the rows, adding ids[i] == t as it goes (the
// block's ids sit in LDS).  No atomics, no workspace, nothing shared between workgroups: capturable, replayable back to back.
// tf_penalty_commit is the one writer of the counts: one wave, outside every graph, after the step's host read.
#include <math.h>
#include "common.h"

#define PEN_THREADS 64                             // one wave per workgroup: 256 entries, 125 workgroups at V = 32 000
#define PEN_PER_THREAD 4
#define PEN_MAX_ROWS 64

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float pen_apply(float x, int c, bool seen, float rep, float freq, float pres) {
    float y = x;
    if (seen && rep != 1.0f) y = (x > 0.0f) ? __fdiv_rn(x, rep) : __fmul_rn(x, rep);
    if (c > 0) {
        y = __fsub_rn(y, __fmul_rn(freq, (float)c));
        y = __fsub_rn(y, pres);
    }
    return y;                                                       // !seen: x, bit for bit
}

// VEC: V, ls_m, os_m are multiples of 4 and every base is aligned — a thread's four entries are CONSECUTIVE and travel in one
// 16-byte load / store per row.  Else: entry j of a thread is blk * 256 + j * 64 + lane (unit stride across the wave), scalar.
// logits and out may be the same buffer: a thread reads an entry of a row before it writes it and nobody else touches it.
template <bool VEC>
__global__ __launch_bounds__(PEN_THREADS) void penalize_logits_kernel(const float* logits, int64_t ls_m, float* out,
                                                                      int64_t os_m, const int64_t* __restrict__ ids,
                                                                      const int32_t* __restrict__ gen_count,
                                                                      const uint8_t* __restrict__ prompt_seen, int rows, int V,
                                                                      float rep, float freq, float pres) {
    __shared__ int s_ids[PEN_MAX_ROWS];
    const int tid = threadIdx.x;
    if (tid < rows) {                                               // rows <= 64 = PEN_THREADS; an id outside [0, V) matches nothing
        int64_t t = ids ? ids[tid] : (int64_t)-1;
        s_ids[tid] = (t >= 0 && t < (int64_t)V) ? (int)t : -1;
    }
    __syncthreads();
    const int base = blockIdx.x * (PEN_THREADS * PEN_PER_THREAD);
    int t[PEN_PER_THREAD], c[PEN_PER_THREAD];
    bool ps[PEN_PER_THREAD];
    if (VEC) {
        const int t0 = base + tid * PEN_PER_THREAD;
        if (t0 >= V) return;                                        // V % 4 == 0: all four or none
        const i32x4 g = *reinterpret_cast<const i32x4*>(gen_count + t0);
        const uint32_t p4 = *reinterpret_cast<const uint32_t*>(prompt_seen + t0);
#pragma unroll
        for (int j = 0; j < PEN_PER_THREAD; ++j) {
            t[j] = t0 + j;
            c[j] = g[j];
            ps[j] = ((p4 >> (8 * j)) & 0xffu) != 0;
        }
#pragma unroll 4
        for (int i = 0; i < rows; ++i) {
            const int id = s_ids[i];
            f32x4 x = *reinterpret_cast<const f32x4*>(logits + (int64_t)i * ls_m + t0);
#pragma unroll
            for (int j = 0; j < PEN_PER_THREAD; ++j) {
                c[j] += (id == t[j]) ? 1 : 0;
                x[j] = pen_apply(x[j], c[j], ps[j] || c[j] > 0, rep, freq, pres);
            }
            *reinterpret_cast<f32x4*>(out + (int64_t)i * os_m + t0) = x;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PEN_PER_THREAD; ++j) {
            t[j] = base + j * PEN_THREADS + tid;
            const bool in = t[j] < V;
            c[j] = in ? gen_count[t[j]] : 0;
            ps[j] = in ? prompt_seen[t[j]] != 0 : false;
            if (!in) t[j] = -2;                                     // matches no id (-1 = "no id") and is never stored
        }
#pragma unroll 2
        for (int i = 0; i < rows; ++i) {
            const int id = s_ids[i];
            const float* xr = logits + (int64_t)i * ls_m;
            float* yr = out + (int64_t)i * os_m;
            float x[PEN_PER_THREAD];
#pragma unroll
            for (int j = 0; j < PEN_PER_THREAD; ++j) x[j] = t[j] >= 0 ? xr[t[j]] : 0.0f;
#pragma unroll
            for (int j = 0; j < PEN_PER_THREAD; ++j) {
                c[j] += (id == t[j]) ? 1 : 0;
                if (t[j] >= 0) yr[t[j]] = pen_apply(x[j], c[j], ps[j] || c[j] > 0, rep, freq, pres);
            }
        }
    }
}

// gen_count[ids[j]] += 1 for j < n; duplicates accumulate (atomicAdd), an id outside [0, V) is skipped.
__global__ __launch_bounds__(PEN_THREADS) void penalty_commit_kernel(int32_t* __restrict__ gen_count,
                                                                     const int64_t* __restrict__ ids, int n, int V) {
    const int j = threadIdx.x;
    if (j >= n) return;
    const int64_t t = ids[j];
    if (t >= 0 && t < (int64_t)V) atomicAdd(gen_count + t, 1);
}

static bool pen_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

extern "C" int tf_penalize_logits(const float* logits, int64_t ls_m, float* out, int64_t os_m, const int64_t* ids,
                                  const int32_t* gen_count, const uint8_t* prompt_seen, int rows, int V, float repetition,
                                  float frequency, float presence, void* stream) {
    if (!logits || !out || !gen_count || !prompt_seen) return TF_EINVAL;
    if (rows < 1 || rows > PEN_MAX_ROWS || V < 1 || ls_m < (int64_t)V || os_m < (int64_t)V) return TF_EINVAL;
    if (!isfinite(repetition) || !(repetition > 0.0f) || !isfinite(frequency) || !isfinite(presence)) return TF_EINVAL;
    const unsigned grid = (unsigned)(((int64_t)V + PEN_THREADS * PEN_PER_THREAD - 1) / (PEN_THREADS * PEN_PER_THREAD));
    const bool vec = (V % 4 == 0) && (ls_m % 4 == 0) && (os_m % 4 == 0) && pen_aligned(logits, 16) && pen_aligned(out, 16) &&
                     pen_aligned(gen_count, 16) && pen_aligned(prompt_seen, 4);
    if (vec)
        hipLaunchKernelGGL(penalize_logits_kernel<true>, dim3(grid), dim3(PEN_THREADS), 0, (hipStream_t)stream, logits, ls_m,
                           out, os_m, ids, gen_count, prompt_seen, rows, V, repetition, frequency, presence);
    else
        hipLaunchKernelGGL(penalize_logits_kernel<false>, dim3(grid), dim3(PEN_THREADS), 0, (hipStream_t)stream, logits, ls_m,
                           out, os_m, ids, gen_count, prompt_seen, rows, V, repetition, frequency, presence);
    TF_LAUNCH_CHECK();
    return TF_OK;
}

extern "C" int tf_penalty_commit(int32_t* gen_count, const int64_t* ids, int n, int V, void* stream) {
    if (!gen_count || !ids || n < 0 || n > PEN_MAX_ROWS || V < 1) return TF_EINVAL;
    if (n == 0) return TF_OK;
    hipLaunchKernelGGL(penalty_commit_kernel, dim3(1), dim3(PEN_THREADS), 0, (hipStream_t)stream, gen_count, ids, n, V);
    TF_LAUNCH_CHECK();
    return TF_OK;
}
