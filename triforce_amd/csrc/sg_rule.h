// Launch rule of the skinny (decode) GEMM, csrc/gemv.hip: WHICH form a shape gets — row tiles, waves per workgroup, panels
// per wave, K-splits across workgroups, and the batch of the narrow-panel form.  Plain C++ (no HIP constructs) so that
// tests/native/test_sg_rule.cpp can pin the rule on the host with g++; gemv.hip only dispatches what this header returns.
#pragma once

enum { SG_PLAIN = 0, SG_GATEUP = 1, SG_F32 = 2, SG_QKV = 3, SG_QKVG = 4 };   // SG_QKVG: SG_QKV with two head counts (GQA); same launch rule
// Attention bias: SG_PLAIN / SG_QKV / SG_QKVG with an fp16 bias added to the complete K sum.  Kernel
// modes of their own, so that the bias-free instantiations keep their names and their code; the launch rule sees the base mode.
enum { SG_PLAIN_B = 5, SG_QKV_B = 6, SG_QKVG_B = 7 };
constexpr bool sg_has_bias(int mode) { return mode >= SG_PLAIN_B; }
constexpr int sg_base_mode(int mode) { return mode == SG_PLAIN_B ? SG_PLAIN : mode == SG_QKV_B ? SG_QKV : mode == SG_QKVG_B ? SG_QKVG : mode; }

// Waves per workgroup = K-splits of one 16-row panel.  A wave keeps 4 KiB of weights in flight, so a grid of few panels
// (o_proj / down_proj: N = 4096 -> 256 workgroups, one per CU) needs more waves per panel to cover the HBM
// latency-bandwidth product (cold-cache graph replay, tools/tune.py): o_proj 9.0 -> 7.6 us, down_proj 20.8 -> 18.3 us with
// 8 waves per panel; 16 waves measured the same as 8.
constexpr int SG_WAVES = 4;
constexpr int SG_WAVES_WIDE = 8;
constexpr int SG_WIDE_MAX_PANELS = 512;       // <= 2 workgroups per CU -> the wide (more K-splits) form
// P = panels per wave: a wave that multiplies P weight panels against ONE B operand reads x once per P KiB of weights
// (x traffic through L2 -> L1 is panels * M * K * 2 bytes: as large as the weight stream itself at 17 rows with P = 1).
// Measured (profiles/r04_gemm_layout_ab.jsonl, k-octet-major x): P = 2 pays when the halved grid still puts two
// workgroups on most CUs — 13B q|k|v (480 groups) 32.0 -> 27.6 us at 17 rows, 26.9 -> 25.2 at 8; 13B gate|up (432)
// 49.8 -> 47.5 / 48.4 -> 44.7 — and LOSES below that: 7B q|k|v (384 groups) 20.5 -> 23.4, 7B gate|up (344) 32.2 -> 35.4.
// With 4 waves per workgroup it is bit-identical to the P = 1 form (same K ranges per wave, same merge order).
constexpr int SG_P_WIDE_MIN_GROUPS = 420;
constexpr int SG_KSPLIT_MAX = 4;              // workgroups per panel along K, at most
constexpr int SG_TICKETS = 4096;              // panels a split GEMM may have (one ticket each)
constexpr int SG_N8_WAVES = 8;                // waves per 8-row panel of the narrow-panel form

// What tf_sg_tune sets (A/B runs and the tests); the defaults are the shipped rule.
struct SgKnobs {
    int p2_rows = 1;                          // key 0: P = 2 from this many rows (33 = never)
    int p2_groups = SG_P_WIDE_MIN_GROUPS;     // key 2: ... while panels / 2 >= this
    // key 3: split K across workgroups below this many panel groups (0 = never).  Measured
    // (profiles/r04_tp_shard_structural_ab.jsonl, r04_tp8_7b_kernel_timeline_after_splitk.json): NO gain in situ — the 7B
    // TP-8 gate|up GEMM stays at 13.2 us with 258 workgroups instead of 86, q|k|v goes 9.1 -> 10.9 us: at 12-22 MB these
    // launches are made of fixed costs (dispatch, the norm prologue's dependent loads, merge, epilogue, drain), not of the
    // stream the extra CUs would shorten, and the hand-off adds a round trip.
    int ksplit_max_groups = 0;
    int ksplit_force = 0;                     // key 4 (A/B): > 1 that many K-splits for EVERY P = 1 GEMM, 1 never split, 0 the rule
    int few_panels = 200;                     // key 5: gate|up GEMMs of up to this many panels run 8 waves per panel at two row tiles
};

struct SgForm {
    int MT, WAVES, P;                         // 16-row tiles of x, waves per workgroup, panels per wave
};

// (norm: whether the launch has a norm prologue — part of a launch's identity, but no form depends on it.)
inline SgForm sg_pick_form(int mode, bool /*norm*/, int M, int N, int K, const SgKnobs& kn) {
    const int panels = N / 16, nchunks = K >> 5, MT = M <= 16 ? 1 : 2;
    // two panels per wave (x read once per 2 KiB of weights): from p2_rows activation rows up, while the halved grid
    // still covers every CU
    if (M >= kn.p2_rows && (panels % 2) == 0 && panels / 2 >= kn.p2_groups && nchunks >= 16) return {MT, SG_WAVES, 2};
    // Few-panel gate|up GEMMs at two row tiles (a tensor-parallel rank's shard at 17-32 rows: 108 panel pairs at 13B TP 8)
    // run 8 waves per panel like the other few-panel forms, not 4: 13B TP-8 retrieval verify 3 421 -> 3 215 us, target
    // verify 5 492 -> 5 278 (profiles/r04_tp_shard_waves_tail_ab.jsonl).  At ONE row tile more waves per panel were
    // measured and lose (16 waves: 7B TP-8 retrieval verify 1 877 -> 1 925 us; q|k|v 10.0 -> 10.9 us, gate|up 13.8 ->
    // 13.9): those launches are not bound by the length of a wave's K chain.
    if (mode == SG_GATEUP) return {MT, (M > 16 && panels <= kn.few_panels && nchunks >= 32) ? SG_WAVES_WIDE : SG_WAVES, 1};
    // wide form: few panels and enough k-chunks that every wave still gets >= 2 of them
    const bool wide = panels <= SG_WIDE_MAX_PANELS && nchunks >= 2 * SG_WAVES_WIDE;
    return {MT, wide ? SG_WAVES_WIDE : SG_WAVES, 1};
}

// Workgroups per panel along K (1 = no split), before the workspace has its say (gemv.hip: a registered workspace that
// holds the partials, a free stream slot): only the P = 1 forms, never lm_head, only few-panel grids, and only while every
// wave of every workgroup still gets >= 2 k-chunks.
inline int sg_pick_ks(int panels, int P, int nchunks, int WAVES, int mode, const SgKnobs& kn) {
    if (P != 1 || mode == SG_F32 || panels > SG_TICKETS || kn.ksplit_force == 1) return 1;
    int ks;
    if (kn.ksplit_force > 1) {
        ks = kn.ksplit_force;
    } else if (panels > 256 && panels <= 384 && nchunks >= 256) {
        // The one regime where the split pays (profiles/r04_gemm_ksplit_force_ab.jsonl): a grid a little larger than the
        // chip — 13B down_proj: 320 panels on 256 CUs, 64 CUs hold two workgroups and set the pace — with a LONG K
        // (432 k-chunks, 141.6 MB).  Three K-splits (960 workgroups, even): 41.8 -> 34.8 us at 17 rows, 32.4 -> 28.5 at 8,
        // 48.4 -> 39.8 at 32.  With a short K (13B o_proj, 160 k-chunks: 16.3 -> 19.2) or a grid that already fits
        // (7B: 256 panels) it loses.
        ks = 3;
    } else {
        if (panels >= kn.ksplit_max_groups) return 1;
        ks = (256 + panels - 1) / panels;
    }
    if (ks > SG_KSPLIT_MAX) ks = SG_KSPLIT_MAX;
    while (ks > 1 && nchunks / ks < 2 * WAVES) --ks;
    return ks < 1 ? 1 : ks;
}

// GEMM + exchange in one launch (tf_skinny_gemm_xchg): always one panel per wave; wide whenever K allows.
inline int sg_xchg_waves(int K) { return (K >> 5) >= 2 * SG_WAVES_WIDE ? SG_WAVES_WIDE : SG_WAVES; }

// Narrow-panel form (skinny_gemm_n8_kernel): 8-row tiles of x and U = 64-wide super-chunks a wave keeps in flight (x NA
// weight streams) — its whole share when that is <= 8 (7B: 8, one round trip per wave), else the even split of 10 (13B:
// 5 + 5).  The gate|up form holds two weight streams: from two row tiles up a batch of 4 (or 13B's 5 + 5) keeps it inside
// 256 registers; three row tiles of any other mode (q|k|v is the only one built) take 5.
struct SgN8Form {
    int MT, U;
};
inline SgN8Form sg_pick_n8(int mode, int M, int K) {
    const int nsc = K >> 6, cpw = (nsc + SG_N8_WAVES - 1) / SG_N8_WAVES, MT = M <= 8 ? 1 : M <= 16 ? 2 : 3;
    if ((cpw > 8 && (cpw % 5) == 0) || (mode != SG_GATEUP && MT == 3)) return {MT, 5};
    return {MT, (mode == SG_GATEUP && MT > 1) ? 4 : 8};
}
