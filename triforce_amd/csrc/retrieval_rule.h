// Launch rules of the retrieval build and the KV row moves, csrc/retrieval.hip: WHICH top-k kernel a (C, sets) pair gets
// and with how much LDS, and how many workgroups the chunk scorers and the row copy put along x.  Plain C++ (no HIP
// constructs) so that tests/native/test_retrieval_rule.cpp can pin the rules on the host with g++; retrieval.hip only
// dispatches what this header returns.
#pragma once
#include <cstddef>
#include <cstdint>

enum { RT_TOPK_SELECT = 0, RT_TOPK_FULL = 1 };

constexpr size_t RT_SELECT_LDS_MAX = 150 * 1024;    // dynamic LDS of the select form, at most (+ ~1 KiB static, of a CU's 160 KiB)
constexpr size_t RT_SELECT_LDS_PLAIN = 48 * 1024;   // ... above this the launch needs the raised attribute
constexpr int RT_SELECT_MPOW2_MAX = 8192;           // winners the select form sorts, at most (padded to a power of two)
constexpr size_t RT_FULL_LDS_PLAIN = 64 * 1024;     // dynamic LDS of the full sort above which the launch needs the raised attribute
constexpr size_t RT_FULL_LDS_MAX = 128 * 1024;      // C <= 32768: 32768 keys

struct RtTopkPick {
    int form;            // RT_TOPK_SELECT | RT_TOPK_FULL
    size_t lds;          // dynamic LDS bytes of the launch
    int mpow2;           // select: sets - 1 rounded up to a power of two, >= 2 (computed for either form)
    int npow2;           // full: C - 1 rounded up to a power of two, >= 2 (0 for the select form)
    bool raise;          // the launch needs hipFuncAttributeMaxDynamicSharedMemorySize raised (to raise_to) first
    size_t raise_to;
};

// select-then-sort when candidates + winners fit in LDS together (always for the paper's shapes), else the full sort.
// 2 <= C <= 32768 and 1 <= sets <= C are the caller's to check.
inline RtTopkPick rt_topk_pick(int C, int sets) {
    int mpow2 = 2;
    while (mpow2 < sets - 1) mpow2 <<= 1;
    const size_t lds_sel = (size_t)((C - 1) + mpow2) * sizeof(uint32_t);
    if (lds_sel <= RT_SELECT_LDS_MAX && mpow2 <= RT_SELECT_MPOW2_MAX)
        return {RT_TOPK_SELECT, lds_sel, mpow2, 0, lds_sel > RT_SELECT_LDS_PLAIN, RT_SELECT_LDS_MAX};
    int npow2 = 2;
    while (npow2 < C - 1) npow2 <<= 1;
    const size_t lds = (size_t)npow2 * sizeof(uint32_t);
    return {RT_TOPK_FULL, lds, mpow2, npow2, lds > RT_FULL_LDS_PLAIN, RT_FULL_LDS_MAX};
}

// Workgroups along x for n chunk groups of work at H heads (the scorer, tf_chunk_mean, the indexed scorer): one 16-byte lane
// per 8 d's, 256 / (D / 8) chunks per workgroup and trip, and 8 resident workgroups per CU and NOT ONE MORE: with
// ceil(2048 / H) the 32 (H = 40) or 2 (H = 5) workgroups past 2 048 start when the others retire and stream their share
// alone, latency-bound (0.59 of peak at H = 40 against 0.81 at H = 32, profiles/r03_bench_13b_cfg4_world1.json); grid-stride
// beyond.
inline int rt_chunk_grid_x(int n, int H, int D) {
    const int gpb = 256 / (D / 8);
    int gx = (n + gpb - 1) / gpb;
    const int cap = H <= 2048 ? 2048 / H : 1;
    if (gx > cap) gx = cap;
    return gx < 1 ? 1 : gx;
}

// Workgroups along x of kv_copy_rows for n rows of D: one 16-byte vector per thread and trip, 64 workgroups at most.
inline int rt_copy_grid_x(int n, int D) {
    int gx = (n * (D / 8) + 255) / 256;
    if (gx > 64) gx = 64;
    return gx;
}
