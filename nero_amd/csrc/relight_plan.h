// relight_plan.h -- the launch and workspace arithmetic of relight.hip, free of HIP calls: tests/relight_plan_main.cpp is a stand-alone
// program over it that the CPU tests build with the undefined-behaviour sanitizer.
#pragma once
#include <cstddef>

namespace nero_relight {

constexpr int MIN_SAMPLES = 1, MAX_SAMPLES = 4096;            // each of Dd, Ds
constexpr long long MAX_LANES = 2147483647ll - 63ll;          // P * padded(D) of one call: 2^31 - 64, a multiple of 64 -- the last lane index
                                                              // of a grid of 64- or 256-thread workgroups over it stays below 2^31
constexpr int PARTIAL_FLOATS = 6;                             // per wavefront: diffuse rgb, specular rgb

inline bool samples_ok(int Dd, int Ds) { return Dd >= MIN_SAMPLES && Dd <= MAX_SAMPLES && Ds >= MIN_SAMPLES && Ds <= MAX_SAMPLES; }
// a point's Dd + Ds samples padded to whole wavefronts: a wavefront belongs to one point
inline int waves_per_point(int Dd, int Ds) { return (Dd + Ds + 63) / 64; }
inline int padded_samples(int Dd, int Ds) { return waves_per_point(Dd, Ds) * 64; }
inline long long total_lanes(int P, int Dd, int Ds) { return (long long)P * (long long)padded_samples(Dd, Ds); }
inline bool total_ok(int P, int Dd, int Ds) { return P >= 0 && total_lanes(P, Dd, Ds) <= MAX_LANES; }
inline size_t workspace_bytes(int P, int Dd, int Ds) {
    return (size_t)P * (size_t)waves_per_point(Dd, Ds) * (size_t)PARTIAL_FLOATS * sizeof(float);
}
// workgroups of `threads` threads that cover `total` items, in 64 bits: total + threads - 1 does not fit an int near 2^31
inline unsigned grid_blocks(long long total, int threads) { return (unsigned)((total + threads - 1) / threads); }

}  // namespace nero_relight
