// relight_bounce_plan.h -- the workspace arithmetic of relight_bounce.hip, free of HIP calls: tests/relight_bounce_plan_main.cpp is a
// stand-alone program over it that the CPU tests build with the address and undefined-behaviour sanitizers.  Lane layout, sample limits and
// the lane total are those of relight_plan.h / envsample_plan.h; only the partial is wider.
#pragma once
#include <cstddef>
#include "envsample_plan.h"
#include "relight_plan.h"

namespace nero_bounce {

constexpr int PARTIAL_FLOATS = 12;                            // per wavefront: direct diffuse, direct specular, indirect diffuse, indirect
                                                              // specular, rgb each
// Dl == 0: the two-strategy primary (Dd, Ds), else the MIS primary (Dd, Ds, Dl)
inline bool samples_ok(int Dd, int Ds, int Dl) { return Dl == 0 ? nero_relight::samples_ok(Dd, Ds) : nero_envsample::samples_ok(Dd, Ds, Dl); }
inline int waves_per_point(int Dd, int Ds, int Dl) { return nero_envsample::waves_per_point(Dd, Ds, Dl); }
inline long long total_lanes(int P, int Dd, int Ds, int Dl) { return nero_envsample::total_lanes(P, Dd, Ds, Dl); }
inline bool total_ok(int P, int Dd, int Ds, int Dl) { return nero_envsample::total_ok(P, Dd, Ds, Dl); }
// at most (2^31 - 64) / 64 wavefronts of 48 bytes each: 1.6e9 bytes, far inside size_t
inline size_t workspace_bytes(int P, int Dd, int Ds, int Dl) {
    return (size_t)P * (size_t)waves_per_point(Dd, Ds, Dl) * (size_t)PARTIAL_FLOATS * sizeof(float);
}
using nero_relight::grid_blocks;

}  // namespace nero_bounce
