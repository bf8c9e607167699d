// relight_plan.h -- the lane, launch and workspace arithmetic of the relighter's estimator kernel (relight_estimator.hip) and ray exports
// (relight.hip), free of HIP calls: tests/relight_plan_main.cpp, tests/envsample_plan_main.cpp and tests/relight_bounce_plan_main.cpp are
// stand-alone programs over it that the CPU tests build with the address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>

namespace nero_relight {

constexpr int MIN_SAMPLES = 1, MAX_SAMPLES = 4096;            // each of Dd, Ds, and of Dl where there are light samples
constexpr long long MAX_LANES = 2147483647ll - 63ll;          // P * padded(D) of one call: 2^31 - 64, a multiple of 64 -- the last lane index
                                                              // of a grid of 64- or 256-thread workgroups over it stays below 2^31
constexpr int PARTIAL_DIRECT = 6;                             // floats per wavefront: diffuse rgb, specular rgb
constexpr int PARTIAL_BOUNCE = 12;                            // with one bounce: the same of the indirect terms behind them

// Dl == 0: the two-strategy estimator (Dd, Ds), else the MIS estimator (Dd, Ds, Dl), which takes at least one light sample
inline bool samples_ok(int Dd, int Ds, int Dl) {
    return Dd >= MIN_SAMPLES && Dd <= MAX_SAMPLES && Ds >= MIN_SAMPLES && Ds <= MAX_SAMPLES && Dl >= 0 && Dl <= MAX_SAMPLES;
}
inline bool mis_samples_ok(int Dd, int Ds, int Dl) { return Dl >= MIN_SAMPLES && samples_ok(Dd, Ds, Dl); }
// a point's D = Dd + Ds + Dl samples padded to whole wavefronts: a wavefront belongs to one point
inline int waves_per_point(int Dd, int Ds, int Dl) { return (Dd + Ds + Dl + 63) / 64; }
inline int padded_samples(int Dd, int Ds, int Dl) { return waves_per_point(Dd, Ds, Dl) * 64; }
inline long long total_lanes(int P, int Dd, int Ds, int Dl) { return (long long)P * (long long)padded_samples(Dd, Ds, Dl); }
inline bool total_ok(int P, int Dd, int Ds, int Dl) { return P >= 0 && total_lanes(P, Dd, Ds, Dl) <= MAX_LANES; }
// at most (2^31 - 64) / 64 wavefronts of 48 bytes each: 1.6e9 bytes, far inside size_t
inline size_t workspace_bytes(int P, int Dd, int Ds, int Dl, int partial_floats) {
    return (size_t)P * (size_t)waves_per_point(Dd, Ds, Dl) * (size_t)partial_floats * sizeof(float);
}
// workgroups of `threads` threads that cover `total` items, in 64 bits: total + threads - 1 does not fit an int near 2^31
inline unsigned grid_blocks(long long total, int threads) { return (unsigned)((total + threads - 1) / threads); }

}  // namespace nero_relight
