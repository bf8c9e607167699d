// stand-alone program over nero_amd/csrc/envsample_plan.h and relight_plan.h (no HIP): the limits of the light table, its weight width and
// workspace, and the grid and workspace arithmetic of the MIS estimator at and around the documented limit P * padded(D) = 2^31 - 64, built by
// tests/test_relight_mis_cpu.py with -fsanitize=undefined.  One line per case.
#include <cstdio>
#include <initializer_list>
#include "../nero_amd/csrc/envsample_plan.h"
#include "../nero_amd/csrc/relight_plan.h"

int main() {
    using namespace nero_envsample;
    using namespace nero_relight;
    int bad = 0;
    // the table
    const int maps[][2] = {{1, 1}, {1, 2}, {3, 5}, {16, 32}, {2048, 4096}, {4096, 16384}, {16384, 4096}, {8192, 8192}, {16384, 1}};
    for (const auto& m : maps) {
        const int eh = m[0], ew = m[1];
        const int64_t N = cells(eh, ew);
        const int B = weight_bits(N);
        if (!map_ok(eh, ew) || B < 1 || B > MAX_WEIGHT_BITS) ++bad;
        // N weights of at most 2^B stay at or below 2^62
        if (N > ((int64_t)1 << (TOTAL_BITS - B))) ++bad;
        if (fixed_bytes(N) < HEAD_BYTES + (size_t)N * 12 || fixed_bytes(N) % 256 != 0) ++bad;
        if ((long long)nero_ws::blocks_of(N) * THREADS < N) ++bad;
        std::printf("map %d %d %lld %d %zu\n", eh, ew, (long long)N, B, fixed_bytes(N));
    }
    if (map_ok(0, 8) || map_ok(8, 0) || map_ok(-1, 8) || map_ok(16385, 1) || map_ok(1, 16385) || map_ok(8192, 8193) || map_ok(16384, 16384)) ++bad;
    if (weight_bits(1) != 40 || weight_bits(2) != 40 || weight_bits(MAX_CELLS) != 36 || weight_bits((int64_t)1 << 22) != 40) ++bad;
    // the MIS kernel
    const int triples[][3] = {{1, 1, 1}, {16, 16, 32}, {3, 2, 60}, {40, 24, 1}, {96, 160, 200}, {64, 64, 128}, {4096, 1, 1}, {4096, 4096, 4096}};
    for (const auto& t : triples) {
        const int Dd = t[0], Ds = t[1], Dl = t[2], D = Dd + Ds + Dl;
        const int pad = padded_samples(Dd, Ds, Dl), wpp = waves_per_point(Dd, Ds, Dl);
        if (!mis_samples_ok(Dd, Ds, Dl) || pad % 64 != 0 || pad < D || pad - D >= 64 || wpp * 64 != pad) ++bad;
        const int P = (int)(MAX_LANES / pad);                           // the largest chunk of points
        const long long total = total_lanes(P, Dd, Ds, Dl);
        if (!total_ok(P, Dd, Ds, Dl) || total_ok(P + 1, Dd, Ds, Dl) || total % 64 != 0) ++bad;
        const long long waves = total / 64;
        if ((long long)workspace_bytes(P, Dd, Ds, Dl, PARTIAL_DIRECT) != waves * PARTIAL_DIRECT * 4 || waves > 2147483647ll) ++bad;
        if ((long long)P * D > 2147483647ll) ++bad;                     // the ray index of nero_relight_mis_rays fits an int
        for (int threads : {64, 256}) {
            const unsigned blocks = grid_blocks(total, threads);
            const long long covered = (long long)blocks * threads;
            if (covered < total || covered - total >= threads || covered - 1 > 2147483647ll || blocks == 0) ++bad;
            std::printf("mis %d %d %d %d %lld %d %u\n", Dd, Ds, Dl, P, total, threads, blocks);
        }
    }
    if (mis_samples_ok(8, 8, 0) || mis_samples_ok(8, 8, 4097) || mis_samples_ok(8, 8, -1) || mis_samples_ok(0, 8, 8) || mis_samples_ok(8, 4097, 8)) ++bad;
    if (total_ok(-1, 8, 8, 8) || total_ok(2147483647, 4096, 4096, 4096) || !total_ok(0, 1, 1, 1) || workspace_bytes(0, 1, 1, 1, PARTIAL_DIRECT) != 0) ++bad;
    return bad;
}
