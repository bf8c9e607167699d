// stand-alone program over nero_amd/csrc/relight_plan.h (no HIP): the workspace and grid arithmetic of the estimator with one bounce at and
// around the documented limit P * padded(D) = 2^31 - 64, for the two-strategy (Dl = 0) and the MIS primary, built by
// tests/test_relight_bounce_cpu.py with -fsanitize=address,undefined.  One line per case.
#include <cstdio>
#include <initializer_list>
#include "../nero_amd/csrc/relight_plan.h"

int main() {
    using namespace nero_relight;
    int bad = 0;
    const int triples[][3] = {{1, 1, 0}, {3, 2, 0}, {32, 32, 0}, {33, 32, 0}, {96, 160, 0}, {4096, 4096, 0},
                              {1, 1, 1}, {16, 16, 32}, {33, 32, 7}, {4096, 1, 1}, {4096, 4096, 4096}};
    for (const auto& t : triples) {
        const int Dd = t[0], Ds = t[1], Dl = t[2], D = Dd + Ds + Dl;
        const int wpp = waves_per_point(Dd, Ds, Dl), pad = wpp * 64;
        if (!samples_ok(Dd, Ds, Dl) || pad < D || pad - D >= 64) ++bad;
        const int P = (int)(MAX_LANES / pad);                           // the largest chunk of points
        const long long total = total_lanes(P, Dd, Ds, Dl);
        if (!total_ok(P, Dd, Ds, Dl) || total_ok(P + 1, Dd, Ds, Dl) || total % 64 != 0 || total != (long long)P * pad) ++bad;
        const long long waves = total / 64;
        const size_t bytes = workspace_bytes(P, Dd, Ds, Dl, PARTIAL_BOUNCE);
        if ((long long)bytes != waves * PARTIAL_BOUNCE * 4 || bytes != 2 * workspace_bytes(P, Dd, Ds, Dl, PARTIAL_DIRECT)) ++bad;
        if ((long long)P * D > 2147483647ll) ++bad;                     // (the row index of nero_relight_bounce_rays is 64 bits all the same)
        for (int threads : {64, 256}) {
            const unsigned blocks = grid_blocks(total, threads);
            const long long covered = (long long)blocks * threads;
            if (covered < total || covered - total >= threads || covered - 1 > 2147483647ll || blocks == 0) ++bad;
            std::printf("bounce %d %d %d %d %lld %zu %d %u\n", Dd, Ds, Dl, P, total, bytes, threads, blocks);
        }
    }
    if (PARTIAL_BOUNCE != 12 || samples_ok(8, 8, -1) || samples_ok(8, 8, 4097) || samples_ok(0, 8, 0) || samples_ok(8, 4097, 0)) ++bad;
    if (total_ok(-1, 8, 8, 0) || total_ok(2147483647, 4096, 4096, 0) || !total_ok(0, 1, 1, 0) || workspace_bytes(0, 1, 1, 0, PARTIAL_BOUNCE) != 0) ++bad;
    if (workspace_bytes(4, 8, 8, 0, PARTIAL_BOUNCE) != 4 * 12 * 4 || workspace_bytes(3, 60, 4, 1, PARTIAL_BOUNCE) != 3 * 2 * 12 * 4) ++bad;
    return bad;
}
