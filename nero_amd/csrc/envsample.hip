// envsample.hip -- importance sampling of the environment map in the relighter (include/nero_hip_envsample.h):
//   nero_env_cdf           the map as a sampling table: one luminance x cos(elevation) weight per cell of an equirectangular grid in world
//                          directions, read through relight_dev.h's env_sample (rotation, convention and cap honoured, nothing inverted),
//                          turned into INTEGER weights on the scale of the largest and summed by hipCUB's integer scan -- the recipe of
//                          surface_sample.hip, so the running sum does not depend on how the scan is partitioned;
//   env_draw / env_pdf     the piecewise-constant 2-D inversion (row marginal, then the row's cells, both read from the one running sum by
//                          binary search, the residuals placing the sample inside its cell) and the density per steradian;
//   nero_relight_mis_rays  the sample set of the three strategies, made by mis_ray() -- relight_ray() for the first Dd + Ds samples;
//   nero_bvh_relight_mis   the same rays walked as shadow rays without being stored, every sample weighed by the balance-heuristic mixture
//                          of the three densities, reduced as relight_kernel reduces (butterfly, one partial per wavefront, a finishing pass
//                          in index order).  No float atomics.
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
#include "envsample_dev.h"                   // the grid, the light draw, the density, mis_ray, mis_weight, mis_terms: shared with
                                             // relight_bounce.hip, which draws and weighs a bounce's one sample by them

#pragma clang fp contract(off)

namespace {

using namespace nero_bvh;
using namespace nero_cub;
using namespace nero_envsample;            // the MIS overloads of samples_ok .. workspace_bytes, the table's sizes (envsample_plan.h)
using nero_relight::EnvMap; using nero_relight::env_sample; using nero_relight::relight_ray; using nero_relight::dotp;
using nero_relight::check_env; using nero_relight::MISS_DEPTH;
using nero_shade::PI_F; using nero_shade::TWO_PI; using nero_shade::sat;

constexpr int PRIV_THREADS = 256;          // workgroup of the private-stack kernels (as relight_kernel)

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

// ---- the sample set (env_draw, env_pdf, mis_ray: envsample_dev.h) ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mis_rays_kernel(const float* __restrict__ pt, const float* __restrict__ tab_d,
                                                       const float* __restrict__ tab_s, const float* __restrict__ tab_l,
                                                       const float* __restrict__ rand_l, int total, int Dd, int Ds, int Dl, int geom,
                                                       const int64_t* __restrict__ cdf, const int64_t* __restrict__ info, int gh, int gw,
                                                       float* __restrict__ ro, float* __restrict__ rd, unsigned char* __restrict__ dead,
                                                       int* __restrict__ cell, float* __restrict__ pdf_l) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;             // ray p D + j
    if (row >= total) return;
    const int D = Dd + Ds + Dl;
    const int p = row / D, j = row - p * D;
    const float* q = pt + (size_t)p * 32;
    const LightTab T = {cdf, gh, gw, (u64)info[0]};
    float w[3], o[3], pdf;
    int k;
    const bool dd = mis_ray(q, tab_d, tab_s, tab_l, rand_l ? rand_l + (size_t)p * 2 : nullptr, j, Dd, Ds, geom, T, w, o, k, pdf);
    const size_t at = (size_t)row * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ro[at + c] = o[c]; rd[at + c] = w[c]; }
    if (dead) dead[row] = dd ? 1 : 0;
    if (cell) cell[row] = k;
    if (pdf_l) pdf_l[row] = pdf;
}

// ---- the estimator (mis_weight, mis_terms: envsample_dev.h) ---------------------------------------------------------------------------------
// The lane layout of relight_kernel: wavefront W of the grid is chunk W % wpp of point W / wpp, lane l its sample (W % wpp) 64 + l; samples
// at or past D are padding.  partial [P wpp, 6]: the wavefront's sums of the diffuse and the specular terms, added by a shuffle butterfly.
template <bool OVERLAP>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void relight_mis_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, int root, const float* __restrict__ pt, const float* __restrict__ tab_d,
    const float* __restrict__ tab_s, const float* __restrict__ tab_l, const float* __restrict__ rand_l, int P_, int Dd, int Ds, int Dl, int wpp,
    int geom, EnvMap E, const int64_t* __restrict__ cdf, const int64_t* __restrict__ info, float* __restrict__ partial) {
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    (void)st;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // below 2^31 (envsample_plan.h)
    const int wave = g >> 6, lane = threadIdx.x & 63;
    const int p = wave / wpp;
    if (p >= P_) return;                                               // a whole wavefront of the last workgroup
    const int D = Dd + Ds + Dl;
    const int j = (wave - p * wpp) * 64 + lane;
    const float* q = pt + (size_t)p * 32;
    float diff[3] = {0.f, 0.f, 0.f}, spec[3] = {0.f, 0.f, 0.f};
    if (j < D) {
        const LightTab T = {cdf, E.h, E.w, (u64)info[0]};
        float d[3], o[3], pl;
        int cell;
        const bool dead = mis_ray(q, tab_d, tab_s, tab_l, rand_l ? rand_l + (size_t)p * 2 : nullptr, j, Dd, Ds, geom, T, d, o, cell, pl);
        NERO_RELIGHT_ANY_HIT(blocked, MISS_DEPTH, dead ? NONE : root)
        if (!dead && !blocked) {
            float L[3];
            env_sample(E, d, L);
            mis_terms(q, d, pl, Dd, Ds, Dl, geom, L, diff, spec);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            diff[c] += __shfl_xor(diff[c], off);
            spec[c] += __shfl_xor(spec[c], off);
        }
    }
    if (lane == 0) {
        float* out = partial + (size_t)wave * nero_relight::PARTIAL_FLOATS;
#pragma unroll
        for (int c = 0; c < 3; ++c) { out[c] = diff[c]; out[3 + c] = spec[c]; }
    }
}

// a point's partials added in index order; both means are over all D samples
__global__ __launch_bounds__(256) void relight_mis_finish_kernel(const float* __restrict__ partial, int P_, int wpp, int D,
                                                                 float* __restrict__ rgb_lin, float* __restrict__ diffuse_lin,
                                                                 float* __restrict__ spec_lin) {
    constexpr int PF = nero_relight::PARTIAL_FLOATS;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P_) return;
    float s[PF] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < wpp; ++k) {
        const float* in = partial + ((size_t)p * wpp + k) * PF;
#pragma unroll
        for (int c = 0; c < PF; ++c) s[c] += in[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float df = s[c] / (float)D, sp = s[3 + c] / (float)D;
        rgb_lin[(size_t)p * 3 + c] = df + sp;
        if (diffuse_lin) diffuse_lin[(size_t)p * 3 + c] = df;
        if (spec_lin) spec_lin[(size_t)p * 3 + c] = sp;
    }
}

// ---- argument checks (check_table_size, check_mis_samples: envsample_dev.h) -----------------------------------------------------------------
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

int nero_relight_mis_rays(const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l, int P, int Dd, int Ds,
                          int Dl, int geometry_type, const int64_t* cdf, const int64_t* info, int gh, int gw, float* rays_o, float* rays_d,
                          unsigned char* dead, int* cell, float* pdf_l, void* stream) {
    if (!pt || !tab_d || !tab_s || !tab_l || !cdf || !info || !rays_o || !rays_d) return nero_fail(NERO_ERR_ARG, "nero_relight_mis_rays: null pointer");
    if (check_mis_samples("nero_relight_mis_rays", P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    if (!map_ok(gh, gw)) return nero_fail(NERO_ERR_ARG, "nero_relight_mis_rays: gh and gw must be in [1, 16384] and gh * gw at most 2^26");
    if (P == 0) return NERO_OK;
    const int total = P * (Dd + Ds + Dl);                              // at most P * padded(D)
    hipLaunchKernelGGL(mis_rays_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, pt, tab_d, tab_s, tab_l, rand_l, total,
                       Dd, Ds, Dl, geometry_type, cdf, info, gh, gw, rays_o, rays_d, dead, cell, pdf_l);
    return nero_check_launch("nero_relight_mis_rays");
}

size_t nero_relight_mis_workspace_bytes(int P, int Dd, int Ds, int Dl) {
    if (!samples_ok(Dd, Ds, Dl) || !total_ok(P, Dd, Ds, Dl)) return 0;
    return workspace_bytes(P, Dd, Ds, Dl);
}

int nero_bvh_relight_mis(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l, int P,
                         int Dd, int Ds, int Dl, int geometry_type, const float* env, int eh, int ew, int convention, const float* rot,
                         float clamp_max, const int64_t* cdf, const int64_t* info, float* rgb_lin, float* diffuse_lin, float* spec_lin, void* ws,
                         size_t ws_bytes, void* stream) {
    if (!handle || !pt || !tab_d || !tab_s || !tab_l || !cdf || !info || !rgb_lin)
        return nero_fail(NERO_ERR_ARG, "nero_bvh_relight_mis: null handle or pointer");
    if (check_mis_samples("nero_bvh_relight_mis", P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env("nero_bvh_relight_mis", env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (check_table_size("nero_bvh_relight_mis", eh, ew) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    if (!ws || ((uintptr_t)ws & 3u) != 0 || ws_bytes < workspace_bytes(P, Dd, Ds, Dl))
        return nero_fail(NERO_ERR_ARG, "nero_bvh_relight_mis: workspace missing, misaligned or smaller than nero_relight_mis_workspace_bytes");
    Handle* h = (Handle*)handle;
    const int wpp = waves_per_point(Dd, Ds, Dl);
    const long long total = total_lanes(P, Dd, Ds, Dl);
    float* partial = (float*)ws;
    if (h->mode == 0)
        hipLaunchKernelGGL(relight_mis_kernel<false>, dim3(grid_blocks(total, PRIV_THREADS)), dim3(PRIV_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pt, tab_d, tab_s, tab_l, rand_l, P, Dd, Ds, Dl, wpp, geometry_type, E, cdf, info,
                           partial);
    else
        hipLaunchKernelGGL(relight_mis_kernel<true>, dim3(grid_blocks(total, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pt, tab_d, tab_s, tab_l, rand_l, P, Dd, Ds, Dl, wpp, geometry_type, E, cdf, info,
                           partial);
    if (nero_check_launch("nero_bvh_relight_mis") != NERO_OK) return NERO_ERR_LAUNCH;
    hipLaunchKernelGGL(relight_mis_finish_kernel, dim3(grid_blocks(P, 256)), dim3(256), 0, (hipStream_t)stream, partial, P, wpp, Dd + Ds + Dl,
                       rgb_lin, diffuse_lin, spec_lin);
    return nero_check_launch("nero_bvh_relight_mis (finish)");
}

}  // extern "C"
