// The row pass of the log-probability kernels (DESIGN sections 23 and 33), shared by logprobs.hip and top_logprobs.hip: how a
// workgroup of LP_THREADS walks one fp32 row, how a thread accumulates its running (max, sum of exp(x - max)), how the
// workgroup folds them, and the value expression.  Both kernels go through these functions, so a row's (M, log S) and every
// value x[t] - M - log S come out bit for bit the same from either.
#pragma once
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

// One walk of the row x[0 .. V) by the workgroup: [0, head) scalar up to the first 16-byte boundary, then nvec aligned 16-byte
// loads, then [tail0, V) scalar: whatever the base address and the stride are, all but at most six entries of a row travel in
// 16-byte loads.  f4(vector, id of its first entry) and f1(value, id) see every entry exactly once; a thread sees its
// vectors in ascending order, four loads in flight, then its head entry, then its tail entry.
template <class F4, class F1>
__device__ __forceinline__ void lp_for_each(const float* __restrict__ x, int V, int tid, F4&& f4, F1&& f1) {
    const int head = min(V, (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2));
    const int nvec = (V - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const f32x4* xv = reinterpret_cast<const f32x4*>(x + head);
    int i = tid;
    for (; i + 3 * LP_THREADS < nvec; i += 4 * LP_THREADS) {        // four loads in flight per thread
        const f32x4 a = xv[i], b = xv[i + LP_THREADS], c = xv[i + 2 * LP_THREADS], d = xv[i + 3 * LP_THREADS];
        f4(a, head + 4 * i);
        f4(b, head + 4 * (i + LP_THREADS));
        f4(c, head + 4 * (i + 2 * LP_THREADS));
        f4(d, head + 4 * (i + 3 * LP_THREADS));
    }
    for (; i < nvec; i += LP_THREADS) f4(xv[i], head + 4 * i);
    if (tid < head) f1(x[tid], tid);
    if (tid < V - tail0) f1(x[tail0 + tid], tail0 + tid);
}

// The workgroup's (M, log S) from every thread's (m, s): wave — common maximum, sums rescaled to it — then one LDS step
// across the waves.  Returns true on the one thread (lane 0 of wave 0) that holds the result.  One __syncthreads inside.
__device__ __forceinline__ bool lp_fold(float m, float s, float* red_m, float* red_s, int lane, int wave, float& M,
                                        float& logS) {
    const float wm = wave_max(m);
    const float ws = wave_sum(m > -INFINITY ? s * expf(m - wm) : 0.f);
    if (lane == 0) {
        red_m[wave] = wm;
        red_s[wave] = ws;
    }
    __syncthreads();
    if (wave != 0) return false;
    const float pm = lane < LP_WAVES ? red_m[lane] : -INFINITY;
    const float ps = lane < LP_WAVES ? red_s[lane] : 0.f;
    M = wave_max(pm);
    const float S = wave_sum(pm > -INFINITY ? ps * expf(pm - M) : 0.f);
    logS = logf(S);
    return lane == 0;
}

// the value of entry t of the row; outside [0, V): no target, 0
__device__ __forceinline__ float lp_value(const float* __restrict__ x, int64_t t, int V, float M, float logS) {
    return (t >= 0 && t < (int64_t)V) ? (x[t] - M) - logS : 0.f;
}
