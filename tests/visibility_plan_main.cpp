// stand-alone program over nero_amd/csrc/visibility_plan.h (no HIP): the grid arithmetic of the visibility kernels at and around the
// documented limit n * S = 2^31 - 64, built by tests/test_visibility_cpu.py with -fsanitize=undefined.  Prints one line per case.
#include <cstdio>
#include <initializer_list>
#include "../nero_amd/csrc/visibility_plan.h"

int main() {
    using namespace nero_vis;
    const long long limit = AO_MAX_RAYS;
    int bad = 0;
    for (int S = AO_MIN_SAMPLES; S <= AO_MAX_SAMPLES; S *= 2) {
        const int n = (int)(limit / S);                               // the largest chunk of points: what ambient_occlusion passes
        const int total = n * S;
        if (!samples_ok(S) || !total_ok(n, S) || total_ok(n + 1, S) || (1 << log2_of(S)) != S) ++bad;
        for (int threads : {64, 256}) {
            const unsigned blocks = grid_blocks(total, threads);
            const long long covered = (long long)blocks * threads;
            // every item has a thread, no workgroup is empty, and the last thread's index fits an int
            if (covered < total || covered - total >= threads || covered - 1 > 2147483647ll || blocks == 0) ++bad;
            std::printf("%d %d %d %u\n", S, total, threads, blocks);
        }
    }
    if (grid_blocks(2147483647, 256) != 8388608u || grid_blocks(1, 256) != 1u || grid_blocks(256, 256) != 1u || grid_blocks(257, 256) != 2u) ++bad;
    if (samples_ok(0) || samples_ok(7) || samples_ok(12) || samples_ok(2048) || samples_ok(-8) || total_ok(-1, 8)) ++bad;
    return bad;
}
