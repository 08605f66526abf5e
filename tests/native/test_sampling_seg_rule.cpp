// Host-only evaluation of block_sample's slice rule (csrc/sampling.hip) for tests/test_sampling_probes_cpu.py: reads one V per
// line, prints seg and whether the LARGE instance is launched.  The two expressions below are the kernel's, character for
// character; the test also asserts that sampling.hip still holds the same two lines.
#include <cstdio>

#define SAMP_THREADS 1024

int main() {
    int V;
    while (std::scanf("%d", &V) == 1) {
        const int seg = (((V + SAMP_THREADS - 1) / SAMP_THREADS) + 3) & ~3;
        const int large = (V) > SAMP_THREADS * 32;
        std::printf("%d %d\n", seg, large);
    }
    return 0;
}
