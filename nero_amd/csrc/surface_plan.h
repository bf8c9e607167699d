// surface_plan.h -- the limit, weight-width and workspace arithmetic of surface_sample.hip, free of HIP calls: tests/surface_plan_main.cpp is
// a stand-alone program over it that the CPU tests build with the undefined-behaviour sanitizer.  Launches are nero_ws::blocks_of workgroups
// of 256 threads.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ws_plan.h"

namespace nero_surface {

constexpr int64_t MAX_ITEMS = 2147483646ll;                    // V and T: 2^31 - 2, int32 ids and an int item count for hipCUB
constexpr int64_t MAX_SAMPLES = 2147483647ll;                  // n_total: 2^31 - 1, a sample index fits the 32-bit hash key
constexpr int THREADS = 256;                                   // (what nero_ws::blocks_of divides by)
constexpr int MAX_WEIGHT_BITS = 40, TOTAL_BITS = 62;           // w[t] < 2^B with B <= 40, and the sum of all T of them stays <= 2^62

inline bool sizes_ok(int64_t V, int64_t T) { return V >= 1 && V <= MAX_ITEMS && T >= 1 && T <= MAX_ITEMS; }
// the call covers the samples [first, first + n) of n_total
inline bool range_ok(int64_t first, int64_t n, int64_t n_total) {
    return first >= 0 && n >= 0 && n_total >= 0 && n_total <= MAX_SAMPLES && first <= n_total && n <= n_total - first;
}
// B: T <= 2^L with L the bit length of T - 1, so T weights below 2^B sum to less than 2^(L + B) <= 2^62
inline int weight_bits(int64_t T) {
    const int L = nero_ws::bit_length(T - 1);
    return TOTAL_BITS - L < MAX_WEIGHT_BITS ? TOTAL_BITS - L : MAX_WEIGHT_BITS;
}
// the fixed part of the cdf workspace, ahead of the scan's scratch: 256 bytes (the bit pattern of the largest doubled area), then one
// 8-byte word per triangle (its doubled area, overwritten by its weight), rounded up to 256 bytes
constexpr size_t HEAD_BYTES = 256;
inline size_t weights_bytes(int64_t T) { return nero_ws::align256((size_t)T * 8); }

}  // namespace nero_surface
