// visibility_plan.h -- the launch arithmetic of visibility.hip, free of HIP calls: tests/visibility_plan_main.cpp is a stand-alone program
// over it that the CPU tests build with the undefined-behaviour sanitizer.
#pragma once

namespace nero_vis {

constexpr long long AO_MAX_RAYS = 2147483647ll - 63ll;        // n * S of one call: 2^31 - 64, so that the last ray index of a grid of
                                                              // 64- or 256-thread workgroups (a multiple of 64 below 2^31) fits an int
constexpr int AO_MIN_SAMPLES = 8, AO_MAX_SAMPLES = 1024;

inline bool samples_ok(int S) { return S >= AO_MIN_SAMPLES && S <= AO_MAX_SAMPLES && (S & (S - 1)) == 0; }
inline bool total_ok(int n, int S) { return n >= 0 && (long long)n * (long long)S <= AO_MAX_RAYS; }
inline int log2_of(int S) { int l = 0; while ((1 << l) < S) ++l; return l; }

// workgroups of `threads` threads that cover `total` items, in 64 bits: total + threads - 1 does not fit an int near 2^31
inline unsigned grid_blocks(int total, int threads) { return (unsigned)(((long long)total + threads - 1) / threads); }

}  // namespace nero_vis
