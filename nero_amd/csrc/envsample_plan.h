// envsample_plan.h -- the limits, weight-width and workspace arithmetic of the light table (envsample.hip), free of HIP calls:
// tests/envsample_plan_main.cpp is a stand-alone program over it that the CPU tests build with the undefined-behaviour sanitizer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ws_plan.h"

namespace nero_envsample {

constexpr int MAX_SIDE = 16384;                               // eh and ew, as nero_env_lookup
constexpr int64_t MAX_CELLS = (int64_t)1 << 26;               // eh * ew: the table is 8 bytes per cell (512 MB here)
constexpr int MAX_WEIGHT_BITS = 40, TOTAL_BITS = 62;          // w < 2^B (<= 2^B in the fallback) with B <= 40; the sum stays <= 2^62
constexpr int INFO_WORDS = 5;                                 // total, zero-weight cells, e, B, fallback taken
constexpr int THREADS = 256;                                  // (what nero_ws::blocks_of divides by)

inline bool map_ok(int eh, int ew) {
    return eh >= 1 && ew >= 1 && eh <= MAX_SIDE && ew <= MAX_SIDE && (int64_t)eh * (int64_t)ew <= MAX_CELLS;
}
inline int64_t cells(int eh, int ew) { return (int64_t)eh * (int64_t)ew; }
// B: N <= 2^L cells with L the bit length of N - 1, so N weights of at most 2^B sum to at most 2^(L + B) <= 2^62
inline int weight_bits(int64_t N) {
    const int L = nero_ws::bit_length(N - 1);
    return TOTAL_BITS - L < MAX_WEIGHT_BITS ? TOTAL_BITS - L : MAX_WEIGHT_BITS;
}
// the fixed part of the table's workspace, ahead of the scan's scratch: 256 bytes (the bit pattern of the largest float weight), the float
// weights and the 8-byte integer weights, each rounded up to 256 bytes
constexpr size_t HEAD_BYTES = 256;
inline size_t float_bytes(int64_t N) { return nero_ws::align256((size_t)N * 4); }
inline size_t weight_bytes(int64_t N) { return nero_ws::align256((size_t)N * 8); }
inline size_t fixed_bytes(int64_t N) { return HEAD_BYTES + float_bytes(N) + weight_bytes(N); }

}  // namespace nero_envsample
