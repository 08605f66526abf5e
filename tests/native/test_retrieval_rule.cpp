// The launch rules of the retrieval build and the KV row moves (triforce_amd/csrc/retrieval_rule.h) evaluated for the cases of
// tests/retrieval_probes.py: reads one query per line from stdin and prints what the header returns.
//   t C sets   -> form lds mpow2 npow2 raise     (rt_topk_pick)
//   g n H D    -> grid x                         (rt_chunk_grid_x)
//   c n D      -> grid x                         (rt_copy_grid_x)
// tests/test_retrieval_probes_cpu.py compares the lines with the Python restatement that labels the cases.
#include <cstdio>
#include "../../triforce_amd/csrc/retrieval_rule.h"

int main() {
    char op;
    int a, b, c;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 't' && std::scanf("%d %d", &a, &b) == 2) {
            const RtTopkPick p = rt_topk_pick(a, b);
            std::printf("%d %zu %d %d %d\n", p.form, p.lds, p.mpow2, p.npow2, p.raise ? 1 : 0);
        } else if (op == 'g' && std::scanf("%d %d %d", &a, &b, &c) == 3) {
            std::printf("%d\n", rt_chunk_grid_x(a, b, c));
        } else if (op == 'c' && std::scanf("%d %d", &a, &b) == 2) {
            std::printf("%d\n", rt_copy_grid_x(a, b));
        } else {
            return 1;
        }
    }
    return 0;
}
