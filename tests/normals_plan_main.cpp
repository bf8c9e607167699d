// stand-alone program over nero_amd/csrc/normals_plan.h (no HIP): the limit, fixed-point-width, launch and workspace arithmetic of the
// vertex-normal kernels at and around T = 2^21 (where the area width leaves 40 bits) and V = T = 2^31 - 2, built by
// tests/test_vertex_normals_cpu.py with -fsanitize=address,undefined.  One line per triangle count: T L B_area B_angle blocks; then one
// line per vertex count: V sums_bytes workspace_bytes.
#include <cstdio>
#include <vector>
#include "../nero_amd/csrc/normals_plan.h"

int main() {
    using namespace nero_normals;
    using namespace nero_ws;
    int bad = 0;
    const std::vector<int64_t> counts = {1, 2, 3, 256, 257, 65537, (1 << 19) + 1, 1 << 21, (1 << 21) + 1, 1 << 22, 12900000, 1ll << 30, (1ll << 30) + 1,
                                         MAX_ITEMS};
    for (const int64_t T : counts) {
        const int L = bit_length(T - 1), Ba = term_bits(T, WEIGHT_AREA), Bg = term_bits(T, WEIGHT_ANGLE);
        if (L > 31 || (T > 1 && (1ll << (L - 1)) >= T) || (1ll << L) < T) ++bad;
        if (Ba < 1 || Ba > MAX_TERM_BITS || L + Ba > AREA_SUM_BITS || Bg < 1 || Bg > MAX_TERM_BITS || L + Bg > ANGLE_SUM_BITS) ++bad;
        // T terms of magnitude <= 2^B (area), < 2^(B + 2) (angle): within 2^61, so a sum and every partial sum fit an int64
        const unsigned long long area_most = (unsigned long long)T << Ba, angle_most = (unsigned long long)T << (Bg + 2);
        if (area_most > (1ull << 61) || angle_most > (1ull << 61)) ++bad;
        const unsigned blocks = blocks_of(T);
        const int64_t covered = (int64_t)blocks * THREADS;
        if (blocks == 0 || covered < T || covered - T >= THREADS) ++bad;
        const int64_t last_corner = 3 * (T - 1) + 2;                   // the last index read of tris
        if (last_corner < 0 || last_corner != 3 * T - 1) ++bad;
        std::printf("T %lld %d %d %d %u\n", (long long)T, L, Ba, Bg, blocks);
    }
    for (const int64_t V : counts) {
        const size_t sb = sums_bytes(V), wb = workspace_bytes(V);
        if (sb % 256 != 0 || sb < (size_t)V * 24 || sb - (size_t)V * 24 >= 256 || wb != sb + HEAD_BYTES) ++bad;
        const int64_t last_sum = 3 * (V - 1) + 2;                      // the last int64 of the sums, the last float of the normals
        if ((size_t)last_sum * 8 + 8 > sb || last_sum != 3 * V - 1) ++bad;
        const unsigned blocks = blocks_of(V);
        if ((int64_t)blocks * THREADS < V) ++bad;
        std::printf("V %lld %zu %zu\n", (long long)V, sb, wb);
    }
    if (!sizes_ok(1, 1) || !sizes_ok(MAX_ITEMS, MAX_ITEMS) || sizes_ok(0, 1) || sizes_ok(1, 0) || sizes_ok(MAX_ITEMS + 1, 1) ||
        sizes_ok(1, MAX_ITEMS + 1) || sizes_ok(-1, 5) || sizes_ok(1ll << 40, 1) || sizes_ok(8, (1ll << 33) + 7))
        ++bad;
    if (!weight_ok(0) || !weight_ok(1) || weight_ok(2) || weight_ok(-1)) ++bad;
    if (term_bits(1, WEIGHT_AREA) != 40 || term_bits(1 << 21, WEIGHT_AREA) != 40 || term_bits((1 << 21) + 1, WEIGHT_AREA) != 39 ||
        term_bits(MAX_ITEMS, WEIGHT_AREA) != 30)
        ++bad;
    if (term_bits(1, WEIGHT_ANGLE) != 40 || term_bits(1 << 19, WEIGHT_ANGLE) != 40 || term_bits((1 << 19) + 1, WEIGHT_ANGLE) != 39 ||
        term_bits(1 << 21, WEIGHT_ANGLE) != 38 || term_bits((1 << 21) + 1, WEIGHT_ANGLE) != 37 || term_bits(MAX_ITEMS, WEIGHT_ANGLE) != 28)
        ++bad;
    std::printf("bad %d\n", bad);
    return bad;
}
