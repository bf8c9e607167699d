// stand-alone program over nero_amd/csrc/surface_plan.h (no HIP): the limit, weight-width and launch arithmetic of the surface sampler at
// and around n = 2^31 - 1 samples and T = 2^31 - 2 triangles, built by tests/test_surface_sample_cpu.py with -fsanitize=undefined.  One
// line per triangle count: T L B blocks weights_bytes.
#include <cstdio>
#include "../nero_amd/csrc/surface_plan.h"

int main() {
    using namespace nero_surface;
    using namespace nero_ws;
    int bad = 0;
    const int64_t counts[] = {1, 2, 3, 64, 65, 320, (1 << 20) + 3, 1 << 22, (1 << 22) + 1, 1 << 23, 12900000, 1ll << 30, (1ll << 30) + 1, MAX_ITEMS};
    for (const int64_t T : counts) {
        const int L = bit_length(T - 1), B = weight_bits(T);
        // T <= 2^L, so T weights below 2^B sum to at most T (2^B - 1) < 2^62: the total fits an int64 with room to spare
        if (L > 31 || (T > 1 && (1ll << (L - 1)) >= T) || (1ll << L) < T) ++bad;
        if (B < 1 || B > MAX_WEIGHT_BITS || B != (TOTAL_BITS - L < MAX_WEIGHT_BITS ? TOTAL_BITS - L : MAX_WEIGHT_BITS) || L + B > TOTAL_BITS) ++bad;
        const unsigned long long most = (unsigned long long)T * ((1ull << B) - 1ull);        // (31 + 40 bits would not fit: L + B <= 62 does)
        if (most >= (1ull << TOTAL_BITS)) ++bad;
        if ((B < MAX_WEIGHT_BITS) != (L > TOTAL_BITS - MAX_WEIGHT_BITS)) ++bad;
        const unsigned blocks = blocks_of(T);
        const int64_t covered = (int64_t)blocks * THREADS;
        if (blocks == 0 || covered < T || covered - T >= THREADS) ++bad;
        const size_t wb = weights_bytes(T);
        if (wb % 256 != 0 || wb < (size_t)T * 8 || wb - (size_t)T * 8 >= 256) ++bad;
        // the last corner index and the last cdf byte of the mesh
        const int64_t last_corner = 3 * (T - 1) + 2;
        const size_t last_cdf_byte = (size_t)T * 8 - 1;
        if (last_corner < 0 || last_cdf_byte + 1 != (size_t)T * 8) ++bad;
        std::printf("%lld %d %d %u %zu\n", (long long)T, L, B, blocks, wb);
    }
    // a call of the most samples: the grid covers them, the last lane index and the last output element stay in range
    const int64_t n = MAX_SAMPLES;
    const unsigned blocks = blocks_of(n);
    const int64_t last_lane = (int64_t)blocks * THREADS - 1, last_float = 3 * (n - 1) + 2;
    if (blocks != 8388608u || last_lane < n - 1 || last_lane - (n - 1) >= THREADS || last_float != 6442450940ll) ++bad;
    if ((size_t)last_float * sizeof(float) != 25769803760ull) ++bad;
    if (blocks_of(1) != 1u || blocks_of(256) != 1u || blocks_of(257) != 2u) ++bad;
    // limits
    if (!sizes_ok(1, 1) || !sizes_ok(MAX_ITEMS, MAX_ITEMS) || sizes_ok(0, 1) || sizes_ok(1, 0) || sizes_ok(MAX_ITEMS + 1, 1) ||
        sizes_ok(1, MAX_ITEMS + 1) || sizes_ok(-1, 5) || sizes_ok(1ll << 40, 1))
        ++bad;
    if (!range_ok(0, 0, 0) || !range_ok(0, n, n) || !range_ok(n, 0, n) || !range_ok(n - 1, 1, n) || !range_ok(5, 3, 8)) ++bad;
    if (range_ok(-1, 1, 8) || range_ok(0, -1, 8) || range_ok(0, 9, 8) || range_ok(5, 4, 8) || range_ok(9, 0, 8) || range_ok(0, 1, n + 1) ||
        range_ok(0, 1, -1) || range_ok(1, INT64_MAX, n) || range_ok(INT64_MAX, 1, n) || range_ok(INT64_MAX, INT64_MAX, INT64_MAX))
        ++bad;
    if (weight_bits(1) != 40 || weight_bits((1 << 22) + 0) != 40 || weight_bits((1 << 22) + 1) != 39 || weight_bits(MAX_ITEMS) != 31) ++bad;
    std::printf("bad %d\n", bad);
    return bad;
}
