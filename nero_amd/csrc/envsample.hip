// envsample.hip -- the light table of the relighter's third strategy (include/nero_hip_envsample.h):
//   nero_env_cdf           the map as a sampling table: one luminance x cos(elevation) weight per cell of an equirectangular grid in world
//                          directions, read through relight_dev.h's env_sample (rotation, convention and cap honoured, nothing inverted),
//                          turned into INTEGER weights on the scale of the largest and summed by hipCUB's integer scan -- the recipe of
//                          surface_sample.hip, so the running sum does not depend on how the scan is partitioned.
// What reads the table is elsewhere: env_draw / env_pdf, the piecewise-constant 2-D inversion and the density per steradian, in
// envsample_dev.h; nero_relight_mis_rays in relight.hip; nero_bvh_relight_mis in relight_estimator.hip.
// The file is compiled without floating-point contraction: every operation is the one the header and the numpy restatement write.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nero_hip.h"
#include "../../include/nero_hip_envsample.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "cub_calls.h"
#include "envsample_plan.h"
#include "relight_dev.h"
#include "envsample_dev.h"                   // the grid's directions (grid_dir) and the check of the table's size

#pragma clang fp contract(off)

namespace {

using namespace nero_bvh;
using namespace nero_cub;
using namespace nero_envsample;            // the table's sizes (envsample_plan.h), grid_dir
using nero_relight::EnvMap; using nero_relight::env_sample; using nero_relight::check_env;

// ---- the grid (grid_dir: envsample_dev.h) ------------------------------------------------------------------------------------------------
// max(ce, 0) of the centre of a cell of row r, and the centre's direction
__device__ __forceinline__ float cell_centre(int r, int c, int gh, int gw, float* d) {
    const float u = ((float)c + 0.5f) / (float)gw;
    const float v = 1.0f - ((float)r + 0.5f) / (float)gh;
    return fmaxf(grid_dir(u, v, d), 0.f);
}

__device__ __forceinline__ unsigned wave_max32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// a[k], and the largest of them in *mx_bits (zeroed by the caller): non-negative floats order as their bit patterns do
__global__ __launch_bounds__(THREADS) void env_weight_kernel(EnvMap E, int gh, int gw, int64_t N, float* __restrict__ a, unsigned* mx_bits) {
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    float v = 0.f;
    if (k < N) {
        const int r = (int)(k / gw), c = (int)(k - (int64_t)r * gw);
        float d[3], L[3];
        const float ce = cell_centre(r, c, gh, gw, d);
        // the largest luminance at the cell's corners, edge midpoints and centre: the lookup is bilinear, so a bright texel spills into the
        // cells around it, and a weight read at the centre alone would leave that energy to the BRDF strategies' chance
        float best = 0.f;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const float u = ((float)c + 0.5f * (float)s) / (float)gw;
                const float vv = 1.0f - ((float)r + 0.5f * (float)t) / (float)gh;
                (void)grid_dir(u, vv, d);
                env_sample(E, d, L);
                const float y = (0.2126f * L[0] + 0.7152f * L[1]) + 0.0722f * L[2];
                if (isfinite(y) && y > best) best = y;
            }
        }
        const float y = best * ce;
        if (isfinite(y) && y > 0.f) v = y;
        a[k] = v;
    }
    const unsigned m = wave_max32(__float_as_uint(v));                // (lanes past N hold +0)
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(mx_bits, m);
}

// w[k] = floor(a[k] 2^(B - e)), a[k] the fallback's when no cell has a weight; info = {., zero weights, e, B, fallback} (info zeroed by the
// caller, info[0] filled after the scan)
__global__ __launch_bounds__(THREADS) void env_intweight_kernel(const float* __restrict__ a, int gh, int gw, int64_t N,
                                                                const unsigned* __restrict__ mx_bits, int B, u64* __restrict__ w,
                                                                int64_t* info, float* __restrict__ weights) {
    const int64_t k = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const float mx = __uint_as_float(*mx_bits);
    const bool fallback = !(mx > 0.f);
    int e = 0;
    if (!fallback) (void)frexp((double)mx, &e);
    bool zero = false;
    if (k < N) {
        float ak = a[k];
        if (fallback) {
            const int r = (int)(k / gw);
            float d[3];
            ak = cell_centre(r, (int)(k - (int64_t)r * gw), gh, gw, d);
        }
        const u64 wt = (u64)floor(ldexp((double)ak, B - e));           // ak <= mx < 2^e (fallback: ak <= 1 = 2^e): at most 2^B, exact
        w[k] = wt;
        zero = wt == 0;
        if (weights) weights[k] = ak;
    }
    const int zeros = __popcll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd((u64*)(info + 1), (u64)zeros);
    if (k == 0) {
        info[2] = e;
        info[3] = B;
        info[4] = fallback ? 1 : 0;
    }
}

// ---- argument checks (check_table_size: envsample_dev.h) -------------------------------------------------------------------------------------
int cdf_layout(int64_t N, size_t* temp_bytes) {
    if (scan_temp<u64>(N, temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_env_cdf: the scratch-size query of the weight scan failed");
    return NERO_OK;
}

}  // namespace

extern "C" {

size_t nero_env_cdf_workspace_bytes(int eh, int ew) {
    if (!map_ok(eh, ew)) return no_workspace("nero_env_cdf_workspace_bytes: eh and ew must be in [1, 16384] and eh * ew at most 2^26");
    size_t temp = 0;
    if (cdf_layout(cells(eh, ew), &temp) != NERO_OK) return 0;
    return fixed_bytes(cells(eh, ew)) + temp;
}

int nero_env_cdf(const float* env, int eh, int ew, int convention, const float* rot, float clamp_max, void* ws, int64_t* cdf, int64_t* info,
                 float* weights, void* stream) {
    EnvMap E;
    if (check_env("nero_env_cdf", env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (check_table_size("nero_env_cdf", eh, ew) != NERO_OK) return NERO_ERR_ARG;
    if (!ws || !cdf || !info) return nero_fail(NERO_ERR_ARG, "nero_env_cdf: null pointer");
    if (((uintptr_t)ws & 255u) != 0) return nero_fail(NERO_ERR_ARG, "nero_env_cdf: the workspace is not 256-byte aligned");
    const int64_t N = cells(eh, ew);
    size_t temp_bytes = 0;
    if (int rc = cdf_layout(N, &temp_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    unsigned* mx_bits = (unsigned*)b;
    float* a = (float*)(b + HEAD_BYTES);
    u64* w = (u64*)(b + HEAD_BYTES + float_bytes(N));
    void* temp = b + fixed_bytes(N);
    if (hipMemsetAsync(mx_bits, 0, sizeof(u64), s) != hipSuccess || hipMemsetAsync(info, 0, INFO_WORDS * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_env_cdf: hipMemsetAsync failed");
    hipLaunchKernelGGL(env_weight_kernel, dim3(nero_ws::blocks_of(N)), dim3(THREADS), 0, s, E, eh, ew, N, a, mx_bits);
    if (int rc = nero_check_launch("nero_env_cdf: weight pass")) return rc;
    hipLaunchKernelGGL(env_intweight_kernel, dim3(nero_ws::blocks_of(N)), dim3(THREADS), 0, s, (const float*)a, eh, ew, N,
                       (const unsigned*)mx_bits, weight_bits(N), w, info, weights);
    if (int rc = nero_check_launch("nero_env_cdf: integer-weight pass")) return rc;
    if (int rc = inclusive_sum(temp, temp_bytes, (const u64*)w, (u64*)cdf, N, s, "nero_env_cdf: the weight scan failed")) return rc;
    if (hipMemcpyAsync(info, cdf + (N - 1), sizeof(int64_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_env_cdf: the copy of the total failed");
    return NERO_OK;
}

}  // extern "C"
