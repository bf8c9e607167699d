// stand-alone program over nero_amd/csrc/tex_fetch_plan.h (no HIP): the level counts, sizes and offsets of the mip pyramid at the sizes
// its tests run and at the limits, and the argument checks at their edges, built by tests/test_tex_fetch_cpu.py with
// -fsanitize=address,undefined.  The levels of a pyramid are marked into a byte per record: they tile it without gap or overlap (the
// 16384 x 16384 pyramid, 358 M records, is checked by its offsets alone).  One line per size: P h w levels records bytes; one per level:
// V h w k h_k w_k offset.
#include <cstdio>
#include <utility>
#include <vector>
#include "../nero_amd/csrc/tex_fetch_plan.h"

int main() {
    using namespace nero_texfetch;
    int bad = 0;
    const std::vector<std::pair<int64_t, int64_t>> sizes = {{1, 1},   {2, 2},   {4, 2},       {6, 10},      {8, 8},         {64, 64},
                                                            {96, 80}, {3, 16384}, {1000, 1000}, {2048, 2048}, {16384, 8192}, {16384, 16384}};
    for (const auto& s : sizes) {
        const int64_t h = s.first, w = s.second;
        Plan P;
        if (!make_plan(h, w, &P)) ++bad;
        if (P.L != levels(h, w) || P.L < 1 || P.L > MAX_LEVELS) ++bad;
        // the levels lie back to back, level 0 first, each half the one below on both sides, and the one above the last would not exist
        int64_t at = 0;
        for (int k = 0; k < P.L; ++k) {
            if (P.off[k] != at || P.h[k] != (h >> k) || P.w[k] != (w >> k) || P.h[k] < 1 || P.w[k] < 1) ++bad;
            if (k > 0 && (P.h[k - 1] != 2 * P.h[k] || P.w[k - 1] != 2 * P.w[k])) ++bad;
            at += (int64_t)P.h[k] * P.w[k];
            std::printf("V %lld %lld %d %d %d %lld\n", (long long)h, (long long)w, k, P.h[k], P.w[k], (long long)P.off[k]);
        }
        if (P.records != at || pyramid_bytes(h, w) != (size_t)at * RECORD_BYTES) ++bad;
        if (P.L < MAX_LEVELS && P.h[P.L - 1] % 2 == 0 && P.w[P.L - 1] % 2 == 0) ++bad;
        if (P.records >= MAX_COUNT) ++bad;                                  // a record index fits an int32
        // the last record a clamped tap can name in every level is the level's last, and lies inside the pyramid
        for (int k = 0; k < P.L; ++k) {
            const int64_t last = P.off[k] + (int64_t)(P.h[k] - 1) * P.w[k] + (P.w[k] - 1);
            if (last != (k + 1 < P.L ? P.off[k + 1] : P.records) - 1) ++bad;
        }
        if (P.records <= (1 << 24)) {                                       // mark every record of every level: once each, none left
            std::vector<unsigned char> seen((size_t)P.records, 0);
            for (int k = 0; k < P.L; ++k)
                for (int64_t y = 0; y < P.h[k]; ++y)
                    for (int64_t x = 0; x < P.w[k]; ++x) {
                        const int64_t r = P.off[k] + y * P.w[k] + x;
                        if (r < 0 || r >= P.records || seen[(size_t)r]++) ++bad;
                    }
            for (unsigned char c : seen)
                if (c != 1) ++bad;
        }
        if ((uint64_t)blocks_of((int64_t)P.h[0] * P.w[0]) * THREADS < (uint64_t)P.h[0] * P.w[0]) ++bad;
        std::printf("P %lld %lld %d %lld %zu\n", (long long)h, (long long)w, P.L, (long long)P.records, pyramid_bytes(h, w));
    }
    Plan P;
    if (size_ok(0, 1) || size_ok(1, 0) || size_ok(-1, 5) || size_ok(5, -1) || size_ok(16385, 1) || size_ok(1, 16385) || size_ok(1ll << 40, 4) ||
        !size_ok(1, 1) || !size_ok(16384, 16384))
        ++bad;
    if (levels(0, 8) != 0 || levels(8, 0) != 0 || levels(16385, 8) != 0 || levels(-2, -2) != 0 || pyramid_bytes(0, 8) != 0 ||
        pyramid_bytes(8, 16385) != 0 || make_plan(0, 0, &P) || make_plan(32768, 32768, &P))
        ++bad;
    if (!count_ok(0) || !count_ok(MAX_COUNT - 1) || count_ok(-1) || count_ok(MAX_COUNT) || count_ok(1ll << 40)) ++bad;
    if (!corners_ok(0) || !corners_ok(MAX_COUNT / 3 - 1) || corners_ok(MAX_COUNT / 3) || corners_ok(-1)) ++bad;
    if (3 * (MAX_COUNT / 3 - 1) + 2 >= (int64_t)NO_OWNER) ++bad;            // the largest corner number stays below the sentinel
    if (blocks_of(1) != 1 || blocks_of(256) != 1 || blocks_of(257) != 2 || blocks_of(MAX_COUNT - 1) != (1u << 23)) ++bad;
    alignas(8) unsigned char buf[16];
    if (!aligned(buf, 8) || aligned(buf + 4, 8) || aligned(buf + 1, 8) || !aligned(buf + 8, 8)) ++bad;
    std::printf("bad %d\n", bad);
    return bad;
}
