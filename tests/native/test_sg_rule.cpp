// Host check of the skinny GEMM's launch rule (triforce_amd/csrc/sg_rule.h): the form of every decode GEMM of the
// project's configurations at the default knobs, and the knob edges the GPU tests rely on.  The expected values are
// written out from what the comments of sg_rule.h / gemv.hip and DESIGN sections 13-14 state, not computed by the rule:
//   7B q|k|v 768 panels = 384 pairs (< 420): one panel per wave, 4 waves; 13B q|k|v 480 pairs, 13B gate|up 432 pairs and
//   lm_head 1000 pairs: two panels per wave, 4 waves; 7B gate|up 344 pairs: one panel, 4 waves;
//   o / down (256 panels at 7B, 320 at 13B, <= 512): 8 waves; 13B down_proj (320 panels, 432 k-chunks): 3 K-splits;
//   13B o_proj (160 k-chunks): none; a TP-8 rank's q|k|v (96 / 120 panels): 8 waves; its gate|up (86 / 108 panels):
//   4 waves up to 16 rows, two row tiles and 8 waves above; lm_head is replicated on every rank.
#include <cstdio>
#include "../../triforce_amd/csrc/sg_rule.h"

struct Case {
    const char* name;
    int mode;
    bool norm;
    int N, K;
    int P;              // panels per wave
    int waves_lo;       // waves per workgroup at <= 16 rows
    int waves_hi;       // ... at 17-32 rows
    int ks;             // K-splits across workgroups at the default knobs
};

static const Case CASES[] = {
    // Llama-2 7B (hidden 4096, inter 11008), whole
    {"7B qkv", SG_QKV, true, 3 * 4096, 4096, 1, 4, 4, 1},
    {"7B o", SG_PLAIN, false, 4096, 4096, 1, 8, 8, 1},
    {"7B gate|up", SG_GATEUP, true, 11008, 4096, 1, 4, 4, 1},
    {"7B down", SG_PLAIN, false, 4096, 11008, 1, 8, 8, 1},
    {"7B lm_head", SG_F32, true, 32000, 4096, 2, 4, 4, 1},
    // 13B (hidden 5120, inter 13824), whole
    {"13B qkv", SG_QKV, true, 3 * 5120, 5120, 2, 4, 4, 1},
    {"13B o", SG_PLAIN, false, 5120, 5120, 1, 8, 8, 1},
    {"13B gate|up", SG_GATEUP, true, 13824, 5120, 2, 4, 4, 1},
    {"13B down", SG_PLAIN, false, 5120, 13824, 1, 8, 8, 3},
    {"13B lm_head", SG_F32, true, 32000, 5120, 2, 4, 4, 1},
    // a TP-8 rank's shards: q|k|v and gate|up cut along N, o and down along K, lm_head replicated
    {"7B/8 qkv", SG_QKV, true, 3 * 4096 / 8, 4096, 1, 8, 8, 1},
    {"7B/8 o", SG_PLAIN, false, 4096, 4096 / 8, 1, 8, 8, 1},
    {"7B/8 gate|up", SG_GATEUP, true, 11008 / 8, 4096, 1, 4, 8, 1},
    {"7B/8 down", SG_PLAIN, false, 4096, 11008 / 8, 1, 8, 8, 1},
    {"7B/8 lm_head", SG_F32, true, 32000, 4096, 2, 4, 4, 1},
    {"13B/8 qkv", SG_QKV, true, 3 * 5120 / 8, 5120, 1, 8, 8, 1},
    {"13B/8 o", SG_PLAIN, false, 5120, 5120 / 8, 1, 8, 8, 1},
    {"13B/8 gate|up", SG_GATEUP, true, 13824 / 8, 5120, 1, 4, 8, 1},
    {"13B/8 down", SG_PLAIN, false, 5120, 13824 / 8, 1, 8, 8, 1},
    {"13B/8 lm_head", SG_F32, true, 32000, 5120, 2, 4, 4, 1},
};
static const int ROWS[] = {1, 8, 16, 17, 32};

// the shapes of tests/test_gpu_ops.py::test_gemm_split_across_workgroups with key 3 = 200: panels 96, 120, 86, 108, 192, 64
// -> ceil(256 / panels) workgroups per panel, at most 4
struct SplitCase {
    int mode;
    bool norm;
    int N, K, ks;
};
static const SplitCase SPLIT[] = {
    {SG_QKV, true, 1536, 4096, 3},    {SG_QKV, true, 1920, 5120, 3},   {SG_GATEUP, true, 1376, 4096, 3},
    {SG_GATEUP, true, 1728, 5120, 3}, {SG_PLAIN, true, 3072, 4096, 2}, {SG_PLAIN, true, 1024, 11008, 4},
};
static const int SPLIT_ROWS[] = {1, 7, 17, 32};

static long checked = 0;
static int failed = 0;
#define CHECK(cond, ...)              \
    do {                              \
        ++checked;                    \
        if (!(cond)) {                \
            ++failed;                 \
            std::printf("MISMATCH "); \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
        }                             \
    } while (0)

static int ks_of(const Case& c, const SgForm& f, const SgKnobs& kn) {
    return sg_pick_ks(c.N / 16, f.P, c.K >> 5, f.WAVES, c.mode, kn);
}

int main() {
    const SgKnobs def;
    for (const Case& c : CASES)
        for (int M : ROWS) {
            const SgForm f = sg_pick_form(c.mode, c.norm, M, c.N, c.K, def);
            const int mt = M <= 16 ? 1 : 2, waves = M <= 16 ? c.waves_lo : c.waves_hi;
            CHECK(f.MT == mt && f.WAVES == waves && f.P == c.P, "%s M=%d: form {%d, %d, %d}, expected {%d, %d, %d}", c.name, M,
                  f.MT, f.WAVES, f.P, mt, waves, c.P);
            CHECK(ks_of(c, f, def) == c.ks, "%s M=%d: ks %d, expected %d", c.name, M, ks_of(c, f, def), c.ks);

            SgKnobs kn;                                                    // key 0 = 33: never two panels per wave
            kn.p2_rows = 33;
            CHECK(sg_pick_form(c.mode, c.norm, M, c.N, c.K, kn).P == 1, "%s M=%d: P = 2 with key 0 = 33", c.name, M);
            kn = SgKnobs();                                                // key 4 = 1: never split
            kn.ksplit_force = 1;
            CHECK(ks_of(c, f, kn) == 1, "%s M=%d: split with key 4 = 1", c.name, M);
        }
    {
        SgKnobs kn;                                                        // key 3 = 200
        kn.ksplit_max_groups = 200;
        for (const SplitCase& s : SPLIT)
            for (int M : SPLIT_ROWS) {
                const SgForm f = sg_pick_form(s.mode, s.norm, M, s.N, s.K, kn);
                const int ks = sg_pick_ks(s.N / 16, f.P, s.K >> 5, f.WAVES, s.mode, kn);
                CHECK(f.P == 1 && ks == s.ks, "N=%d K=%d M=%d key 3 = 200: P %d ks %d, expected 1 and %d", s.N, s.K, M, f.P, ks, s.ks);
                CHECK(ks >= 2 && ks <= 4 && (s.K >> 5) / ks >= 2 * f.WAVES, "N=%d K=%d M=%d: ks %d leaves %d k-chunks for %d waves",
                      s.N, s.K, M, ks, (s.K >> 5) / ks, f.WAVES);
                CHECK(sg_pick_ks(s.N / 16, f.P, s.K >> 5, f.WAVES, s.mode, def) == 1, "N=%d K=%d M=%d: split at the default knobs",
                      s.N, s.K, M);
            }
    }
    // the exchange GEMM (o / down of a TP rank): 8 waves from 16 k-chunks up
    CHECK(sg_xchg_waves(512) == 8 && sg_xchg_waves(1376) == 8 && sg_xchg_waves(640) == 8 && sg_xchg_waves(480) == 4, "xchg waves");
    // narrow panels: 7B (K 4096: 8 super-chunks per wave) one batch of 8, gate|up from two row tiles 4; 13B (K 5120: 10) 5 + 5;
    // q|k|v at three row tiles 5
    struct { int mode, M, K, MT, U; } const N8[] = {
        {SG_QKV, 1, 4096, 1, 8},    {SG_QKV, 8, 4096, 1, 8},    {SG_QKV, 9, 4096, 2, 8},     {SG_QKV, 16, 4096, 2, 8},
        {SG_QKV, 17, 4096, 3, 5},   {SG_QKV, 24, 4096, 3, 5},   {SG_GATEUP, 8, 4096, 1, 8},  {SG_GATEUP, 9, 4096, 2, 4},
        {SG_GATEUP, 17, 4096, 3, 4}, {SG_QKV, 8, 5120, 1, 5},   {SG_QKV, 16, 5120, 2, 5},    {SG_QKV, 24, 5120, 3, 5},
        {SG_GATEUP, 8, 5120, 1, 5}, {SG_GATEUP, 16, 5120, 2, 5}, {SG_GATEUP, 24, 5120, 3, 5},
    };
    for (const auto& n : N8) {
        const SgN8Form f = sg_pick_n8(n.mode, n.M, n.K);
        CHECK(f.MT == n.MT && f.U == n.U, "n8 mode %d M=%d K=%d: {%d, %d}, expected {%d, %d}", n.mode, n.M, n.K, f.MT, f.U, n.MT, n.U);
    }
    if (failed) return 1;
    std::printf("OK %ld rule checks\n", checked);
    return 0;
}
