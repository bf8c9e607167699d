// normals_plan.h -- the limit, fixed-point-width and workspace arithmetic of mesh_normals.hip, free of HIP calls: tests/normals_plan_main.cpp
// is a stand-alone program over it that the CPU tests build with the address and undefined-behaviour sanitizers.  Launches are
// nero_ws::blocks_of workgroups of 256 threads.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "ws_plan.h"

namespace nero_normals {

constexpr int64_t MAX_ITEMS = 2147483646ll;                    // V and T: 2^31 - 2, int32 ids
constexpr int THREADS = 256;                                   // (what nero_ws::blocks_of divides by)
constexpr int WEIGHT_AREA = 0, WEIGHT_ANGLE = 1;
constexpr int MAX_TERM_BITS = 40;                              // a fixed-point term carries at most 40 fractional bits
constexpr int AREA_SUM_BITS = 61, ANGLE_SUM_BITS = 59;         // |q| <= 2^B (area), < 2^(B + 2) (angle): T of them stay within 2^61

inline bool sizes_ok(int64_t V, int64_t T) { return V >= 1 && V <= MAX_ITEMS && T >= 1 && T <= MAX_ITEMS; }
inline bool weight_ok(int weight) { return weight == WEIGHT_AREA || weight == WEIGHT_ANGLE; }
// B: a vertex lies in at most T <= 2^L faces (L the bit length of T - 1), each adding one term per component
//   area   |c_k| <= mx < 2^e, so |llrint(ldexp(c_k, B - e))| <= 2^B and a sum stays within 2^(L + B) <= 2^61
//   angle  |theta n_k| <= pi < 4, so |llrint(ldexp(theta n_k, B))| < 2^(B + 2) and a sum stays below 2^(L + B + 2) <= 2^61
inline int term_bits(int64_t T, int weight) {
    const int room = (weight == WEIGHT_ANGLE ? ANGLE_SUM_BITS : AREA_SUM_BITS) - nero_ws::bit_length(T - 1);
    return room < MAX_TERM_BITS ? room : MAX_TERM_BITS;
}
// workspace: 256 bytes (the bit pattern of the largest |c_k|), then three int64 sums per vertex, rounded up to 256 bytes
constexpr size_t HEAD_BYTES = 256;
inline size_t sums_bytes(int64_t V) { return nero_ws::align256((size_t)V * 24); }
inline size_t workspace_bytes(int64_t V) { return HEAD_BYTES + sums_bytes(V); }

}  // namespace nero_normals
