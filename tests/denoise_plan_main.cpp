// stand-alone program over nero_amd/csrc/denoise_plan.h (no HIP): the argument checks and the tile and grid arithmetic of the denoiser at
// the shapes its tests run, at 800 x 800 and 1600 x 1600, and at the limits (h w = 2^31 - 1 as one row, one column and a near-square), built
// by tests/test_denoise_cpu.py with -fsanitize=address,undefined.  One line per shape: S h w tiles_x tiles_y tiles grid; one per region
// staged in LDS: L stride (0: the variance window) records bytes(G = 0) bytes(G = 4).
#include <cstdio>
#include <limits>
#include <utility>
#include <vector>
#include "../nero_amd/csrc/denoise_plan.h"

int main() {
    using namespace nero_denoise;
    int bad = 0;
    const std::vector<std::pair<int64_t, int64_t>> shapes = {{1, 1},     {1, 7},       {7, 1},       {5, 3},          {17, 33},         {40, 48},        {64, 64},
                                                             {8, 32},    {9, 33},      {800, 800},   {1600, 1600},    {MAX_PIXELS, 1},  {1, MAX_PIXELS}, {46340, 46340},
                                                             {65536, 32767}};
    for (const auto& s : shapes) {
        const int64_t h = s.first, w = s.second;
        if (!shape_ok(h, w)) ++bad;
        const int64_t tx = tiles_x(w), ty = tiles_y(h), t = tiles(h, w);
        const unsigned grid = grid_of(h, w);
        if (tx * TILE_W < w || tx * TILE_W - w >= TILE_W || ty * TILE_H < h || ty * TILE_H - h >= TILE_H || t != tx * ty) ++bad;
        if (t < 1 || t > MAX_PIXELS || grid < 1 || grid > MAX_GRID || (int64_t)grid > t || (t <= (int64_t)MAX_GRID && (int64_t)grid != t)) ++bad;
        if ((uint64_t)grid * THREADS >= (1ull << 32)) ++bad;                                  // a dispatch counts its work-items in 32 bits
        // the last tile's last thread: its pixel lies past the image or is the last one; the farthest tap's coordinates fit an int64
        const int64_t last_y = (ty - 1) * TILE_H + (TILE_H - 1), last_x = (tx - 1) * TILE_W + (TILE_W - 1);
        if (last_y < h - 1 || last_x < w - 1) ++bad;
        const int64_t far_y = (h - 1) + (int64_t)ATROUS_RADIUS * MAX_STEP, far_x = -(int64_t)ATROUS_RADIUS * MAX_STEP;
        if (far_y <= h - 1 || far_x >= 0) ++bad;
        const int64_t last_pixel = (h - 1) * w + (w - 1);
        if (last_pixel != h * w - 1 || last_pixel >= MAX_PIXELS) ++bad;
        // bytes of the records: a size_t holds them
        const size_t guide_bytes = (size_t)(h * w) * 48, signal_bytes = (size_t)(h * w) * 16;
        if (guide_bytes / 48 != (size_t)(h * w) || signal_bytes / 16 != (size_t)(h * w)) ++bad;
        std::printf("S %lld %lld %lld %lld %lld %u\n", (long long)h, (long long)w, (long long)tx, (long long)ty, (long long)t, grid);
    }
    if (shape_ok(0, 1) || shape_ok(1, 0) || shape_ok(-1, 5) || shape_ok(5, -1) || shape_ok(1ll << 31, 1) || shape_ok(1, 1ll << 31) ||
        shape_ok(46341, 46341) || shape_ok(65536, 32768) || shape_ok(1ll << 40, 1ll << 40) || shape_ok(MAX_PIXELS, 2))
        ++bad;
    if (!guide_ok(0) || !guide_ok(4) || guide_ok(1) || guide_ok(8) || guide_ok(-4) || guide_quads(0) != 2 || guide_quads(4) != 3) ++bad;
    if (!step_ok(1) || !step_ok(16) || !step_ok(MAX_STEP) || step_ok(0) || step_ok(-1) || step_ok(MAX_STEP + 1) ||
        step_ok(std::numeric_limits<int>::max()))
        ++bad;
    // the strides whose tile and halo are staged in LDS: the region covers the farthest tap of every pixel of the tile and fits a workgroup
    if (!staged(1) || !staged(2) || staged(0) || staged(3) || staged(4) || staged(MAX_STEP)) ++bad;
    for (int step = 1; step <= MAX_STAGED_STEP; ++step) {
        const int R = ATROUS_RADIUS * step, RW = TILE_W + 2 * R, RH = TILE_H + 2 * R;
        const int first = 0 * RW + 0 + (-R) * RW + (-R) + (R * RW + R), last = (TILE_H - 1 + R) * RW + (TILE_W - 1 + R) + R * RW + R;
        if (staged_records(step) != RW * RH || first != 0 || last != RW * RH - 1) ++bad;
        if (staged_lds_bytes(0, step) != (size_t)RW * RH * 48 || staged_lds_bytes(4, step) != (size_t)RW * RH * 64 ||
            staged_lds_bytes(4, step) > MAX_STATIC_LDS)
            ++bad;
        std::printf("L %d %d %zu %zu\n", step, staged_records(step), staged_lds_bytes(0, step), staged_lds_bytes(4, step));
    }
    {                                                                 // the variance window's region: 38 x 14 records
        const int R = VAR_RADIUS, RW = TILE_W + 2 * R, RH = TILE_H + 2 * R;
        const int last = (TILE_H - 1 + R) * RW + (TILE_W - 1 + R) + R * RW + R;
        if (region_records(R) != RW * RH || last != RW * RH - 1 || region_lds_bytes(4, R) != (size_t)RW * RH * 64 ||
            region_lds_bytes(0, R) != (size_t)RW * RH * 48 || region_lds_bytes(4, R) > MAX_STATIC_LDS)
            ++bad;
        std::printf("L 0 %d %zu %zu\n", region_records(R), region_lds_bytes(0, R), region_lds_bytes(4, R));
    }
    if (!k_ok(0) || !k_ok(6) || !k_ok(10) || k_ok(-1) || k_ok(11)) ++bad;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    if (!sigma_ok(1e-30f) || !sigma_ok(4.0f) || sigma_ok(0.0f) || sigma_ok(-0.0f) || sigma_ok(-1.0f) || sigma_ok(inf) || sigma_ok(-inf) ||
        sigma_ok(nan))
        ++bad;
    std::printf("bad %d\n", bad);
    return bad;
}
