// stand-alone program over nero_amd/csrc/relight_plan.h (no HIP): the grid and workspace arithmetic of the relighting kernel at and around
// the documented limit P * padded(D) = 2^31 - 64, built by tests/test_relight_cpu.py with -fsanitize=undefined.  One line per case.
#include <cstdio>
#include <initializer_list>
#include "../nero_amd/csrc/relight_plan.h"

int main() {
    using namespace nero_relight;
    int bad = 0;
    const int pairs[][2] = {{1, 1}, {5, 3}, {32, 32}, {33, 32}, {64, 64}, {96, 160}, {512, 256}, {4096, 1}, {4096, 4096}};
    for (const auto& pr : pairs) {
        const int Dd = pr[0], Ds = pr[1];
        const int pad = padded_samples(Dd, Ds, 0), wpp = waves_per_point(Dd, Ds, 0);
        if (!samples_ok(Dd, Ds, 0) || pad % 64 != 0 || pad < Dd + Ds || pad - (Dd + Ds) >= 64 || wpp * 64 != pad) ++bad;
        const int P = (int)(MAX_LANES / pad);                          // the largest chunk of points
        const long long total = total_lanes(P, Dd, Ds, 0);
        if (!total_ok(P, Dd, Ds, 0) || total_ok(P + 1, Dd, Ds, 0) || total % 64 != 0) ++bad;
        // the last wavefront's partial lies inside the workspace, and its index fits an int
        const long long waves = total / 64;
        if ((long long)workspace_bytes(P, Dd, Ds, 0, PARTIAL_DIRECT) != waves * PARTIAL_DIRECT * 4 || waves > 2147483647ll) ++bad;
        for (int threads : {64, 256}) {
            const unsigned blocks = grid_blocks(total, threads);
            const long long covered = (long long)blocks * threads;
            if (covered < total || covered - total >= threads || covered - 1 > 2147483647ll || blocks == 0) ++bad;
            std::printf("%d %d %d %lld %d %u\n", Dd, Ds, P, total, threads, blocks);
        }
    }
    if (samples_ok(0, 1, 0) || samples_ok(1, 0, 0) || samples_ok(4097, 1, 0) || samples_ok(1, 4097, 0) || samples_ok(-1, 8, 0) || total_ok(-1, 8, 8, 0)) ++bad;
    if (total_ok(2147483647, 4096, 4096, 0) || !total_ok(0, 1, 1, 0) || workspace_bytes(0, 1, 1, 0, PARTIAL_DIRECT) != 0) ++bad;
    if (grid_blocks(MAX_LANES, 256) != 8388608u || grid_blocks(1, 64) != 1u || grid_blocks(65, 64) != 2u) ++bad;
    return bad;
}
