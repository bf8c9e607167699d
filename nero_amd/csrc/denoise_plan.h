// denoise_plan.h -- the argument checks and the tile and grid arithmetic of denoise.hip, free of HIP calls: tests/denoise_plan_main.cpp is a
// stand-alone program over it that the CPU tests build with the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace nero_denoise {

constexpr int TILE_W = 32, TILE_H = 8;                         // one workgroup owns a TILE_W x TILE_H tile, one thread per pixel
constexpr int THREADS = TILE_W * TILE_H;                       // 256: a wave is two rows of 32 pixels, 512 contiguous bytes of signal each
constexpr int64_t MAX_PIXELS = 2147483647ll;                   // h w < 2^31: a pixel index fits an int32 with room for the sign
constexpr int MAX_STEP = 1 << 20;                              // the farthest tap lies 2 MAX_STEP pixels away: coordinates are int64
constexpr int MAX_K = 10;                                      // w_n = max(0, n_p . n_q)^(2^k), k squarings
constexpr unsigned MAX_GRID = 1u << 20;                        // workgroups of one launch (2^28 work-items, below the 2^32 of a dispatch);
                                                               // a workgroup strides over the tiles beyond that
constexpr int VAR_RADIUS = 3, ATROUS_RADIUS = 2;               // the 7 x 7 variance window, the 5 x 5 taps

// What is staged in LDS: a tile and the halo its taps reach, where the taps of a tile share one (measured to pay there) --
// the variance window (halo VAR_RADIUS) and the a-trous strides up to MAX_STAGED_STEP (halo ATROUS_RADIUS step).  The largest region, G = 4
// at stride 2, is 40 x 16 records of 64 bytes = 40 KiB of the 64 KiB a workgroup may hold.
constexpr int MAX_STAGED_STEP = 2;
constexpr size_t MAX_STATIC_LDS = 65536;
constexpr bool staged(int step) { return step >= 1 && step <= MAX_STAGED_STEP; }
constexpr int region_records(int halo) { return (TILE_W + 2 * halo) * (TILE_H + 2 * halo); }
constexpr int staged_records(int step) { return region_records(ATROUS_RADIUS * step); }
constexpr size_t region_lds_bytes(int G, int halo) { return (size_t)region_records(halo) * 16 * ((G == 4 ? 3 : 2) + 1); }
constexpr size_t staged_lds_bytes(int G, int step) { return region_lds_bytes(G, ATROUS_RADIUS * step); }
static_assert(staged_lds_bytes(4, MAX_STAGED_STEP) <= MAX_STATIC_LDS && region_lds_bytes(4, VAR_RADIUS) <= MAX_STATIC_LDS,
              "a staged region does not fit a workgroup's LDS");

inline bool guide_ok(int G) { return G == 0 || G == 4; }
inline int guide_quads(int G) { return G == 4 ? 3 : 2; }       // 16-byte loads per guide record: [n,8] or [n,12] fp32
inline bool shape_ok(int64_t h, int64_t w) { return h >= 1 && w >= 1 && h <= MAX_PIXELS && w <= MAX_PIXELS && h * w <= MAX_PIXELS; }
inline bool step_ok(int step) { return step >= 1 && step <= MAX_STEP; }
inline bool k_ok(int k) { return k >= 0 && k <= MAX_K; }
inline bool sigma_ok(float s) { return isfinite(s) && s > 0.0f; }

inline int64_t tiles_x(int64_t w) { return (w + TILE_W - 1) / TILE_W; }
inline int64_t tiles_y(int64_t h) { return (h + TILE_H - 1) / TILE_H; }
inline int64_t tiles(int64_t h, int64_t w) { return tiles_x(w) * tiles_y(h); }       // <= h w / 256 + h / 8 + w / 32 + 1 < 2^31
inline unsigned grid_of(int64_t h, int64_t w) {
    const int64_t t = tiles(h, w);
    return (unsigned)(t < (int64_t)MAX_GRID ? t : (int64_t)MAX_GRID);
}

}  // namespace nero_denoise
