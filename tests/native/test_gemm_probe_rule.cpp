// The launch rule of the skinny GEMM (triforce_amd/csrc/sg_rule.h) evaluated for the cases of tests/gemm_probes.py: reads
// one case per line from stdin — mode M N K and the five knobs (tf_sg_tune keys 0, 2, 3, 4, 5) — and prints what the header
// returns: MT WAVES P ks and the narrow-panel form MT U.  tests/test_gemm_probes_cpu.py compares the lines with the Python
// restatement that labels the cases.
#include <cstdio>
#include "../../triforce_amd/csrc/sg_rule.h"

int main() {
    int mode, M, N, K;
    SgKnobs kn;
    while (std::scanf("%d %d %d %d %d %d %d %d %d", &mode, &M, &N, &K, &kn.p2_rows, &kn.p2_groups, &kn.ksplit_max_groups,
                      &kn.ksplit_force, &kn.few_panels) == 9) {
        const SgForm f = sg_pick_form(mode, false, M, N, K, kn);
        const int ks = sg_pick_ks(N / 16, f.P, K >> 5, f.WAVES, mode, kn);
        const SgN8Form n8 = sg_pick_n8(mode, M, K);
        std::printf("%d %d %d %d %d %d\n", f.MT, f.WAVES, f.P, ks, n8.MT, n8.U);
    }
    return 0;
}
