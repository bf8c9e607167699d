// relight.hip -- relighting the Stage-II mesh under a lat-long environment map (include/nero_hip_relight.h).  Replaces what the reference
// hands to Blender Cycles in relight.py with direct lighting and shadows on the mesh tracer's BVH.  Here, what surrounds the estimator:
//   * nero_bvh_export_faces / nero_bvh_trace_faces: the closest-hit walks of bvh_walk.h expanded once more (ANY = false), reporting WHICH
//     triangle was hit (through the builders' leaf-order table, Bvh::d_face) and where on it (the u, v of tri_test's own arithmetic);
//   * nero_env_lookup: bilinear radiance of a lat-long map, in this project's own grid (the inverse of nero_env_encode's directions) or in
//     the equirectangular mapping an .hdr made for the reference's relight.py --hdr assumes;
//   * nero_relight_rays / nero_relight_mis_rays (include/nero_hip_envsample.h): the sample set -- relight_ray() of relight_dev.h IS the
//     definition: the directions of sample_diffuse_directions / sample_specular_directions (field.py:768-810) as mc_shade.hip forms them,
//     with every product and sum rounded on its own; mis_ray() of envsample_dev.h is relight_ray() for the first Dd + Ds samples and the
//     light draws behind them.  The estimator (relight_estimator.hip) forms its rays by the same two functions and never stores them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nero_hip.h"
#include "../../include/nero_hip_relight.h"
#include "../../include/nero_hip_envsample.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "relight_plan.h"
#include "relight_dev.h"                     // env_sample, relight_ray, hit_bary, the choice of the walk and the argument checks
#include "envsample_dev.h"                   // mis_ray and the checks of the MIS sample counts

namespace {

using namespace nero_bvh;
using namespace nero_relight;              // relight_plan.h (grid_blocks), relight_dev.h
using nero_envsample::LightTab; using nero_envsample::u64; using nero_envsample::mis_ray; using nero_envsample::check_mis_samples;
using nero_envsample::map_ok;

// ---- closest hit with the face (hit_bary: relight_dev.h) --------------------------------------------------------------------------------
// OVERLAP: PL_THREADS threads and the LDS stack (trees no deeper than PL_STACK), else PRIV_THREADS threads and the private stack
template <bool OVERLAP>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void trace_faces_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, const int* __restrict__ face_of, int root, const float* __restrict__ ro,
    const float* __restrict__ rd, int n, float* __restrict__ depth, int* __restrict__ face, float* __restrict__ bary) {
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float o[3] = {ro[r * 3], ro[r * 3 + 1], ro[r * 3 + 2]};
    const float d[3] = {rd[r * 3], rd[r * 3 + 1], rd[r * 3 + 2]};
    float inv[3];
    ray_inverse(d, inv);
    float t_hit;
    int slot;
    if constexpr (OVERLAP) {
        NERO_WALK_OVERLAP(false, MISS_DEPTH, root)
        t_hit = tbest; slot = best;
    } else {
        (void)st;
        NERO_WALK_PRIVATE(false, MISS_DEPTH, root)
        t_hit = tbest; slot = best;
    }
    float u = 0.f, v = 0.f;
    if (slot >= 0) hit_bary(tris, slot, o, d, u, v);
    depth[r] = t_hit;
    face[r] = slot >= 0 ? face_of[slot] : -1;
    bary[(size_t)r * 2] = u;
    bary[(size_t)r * 2 + 1] = v;
}

// ---- the environment map (env_sample: relight_dev.h) ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void env_lookup_kernel(EnvMap E, const float* __restrict__ dirs, int64_t n, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]};
    float L[3];
    env_sample(E, d, L);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = L[k];
}

// ---- the sample set (relight_ray: relight_dev.h; mis_ray: envsample_dev.h) ---------------------------------------------------------------
// MIS: the three strategies' D = Dd + Ds + Dl samples with their cell and density, else the two BRDF strategies' (Dl = 0; tab_l .. gw, cell
// and pdf_l unread)
template <bool MIS>
__global__ __launch_bounds__(256) void rays_kernel(const float* __restrict__ pt, const float* __restrict__ tab_d, const float* __restrict__ tab_s,
                                                   const float* __restrict__ tab_l, const float* __restrict__ rand_l, int total, int Dd, int Ds,
                                                   int Dl, int geom, const int64_t* __restrict__ cdf, const int64_t* __restrict__ info, int gh,
                                                   int gw, float* __restrict__ ro, float* __restrict__ rd, unsigned char* __restrict__ dead,
                                                   int* __restrict__ cell, float* __restrict__ pdf_l) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;             // ray p D + j
    if (row >= total) return;
    const int D = Dd + Ds + Dl;
    const int p = row / D, j = row - p * D;
    const float* q = pt + (size_t)p * 32;
    float w[3], o[3], pdf = 0.f;
    int k = -1;
    bool dd;
    if constexpr (MIS) {
        const LightTab T = {cdf, gh, gw, (u64)info[0]};
        dd = mis_ray(q, tab_d, tab_s, tab_l, rand_l ? rand_l + (size_t)p * 2 : nullptr, j, Dd, Ds, geom, T, w, o, k, pdf);
    } else {
        dd = relight_ray(q, tab_d, tab_s, j, Dd, geom, w, o);
    }
    const size_t at = (size_t)row * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ro[at + c] = o[c]; rd[at + c] = w[c]; }
    if (dead) dead[row] = dd ? 1 : 0;
    if constexpr (MIS) {
        if (cell) cell[row] = k;
        if (pdf_l) pdf_l[row] = pdf;
    }
}

}  // namespace

extern "C" {

int nero_bvh_export_faces(void* handle, int* faces_host) {
    if (!handle || !faces_host) return nero_fail(NERO_ERR_ARG, "nero_bvh_export_faces: bad argument");
    const Handle* h = (const Handle*)handle;
    // hipMemcpy orders itself behind the work of the null stream only: wait for every stream, the build's included
    if (hipDeviceSynchronize() != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_export_faces: hipDeviceSynchronize failed");
    if (hipMemcpy(faces_host, h->b.d_face, (size_t)h->b.n_tris * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_export_faces: hipMemcpy failed");
    return NERO_OK;
}

int nero_bvh_trace_faces(void* handle, const float* rays_o, const float* rays_d, int n, float* depth, int* face, float* bary, void* stream) {
    if (!handle || !rays_o || !rays_d || !depth || !face || !bary || n < 0) return nero_fail(NERO_ERR_ARG, "nero_bvh_trace_faces: bad argument");
    if ((long long)n > 2147483647ll / 3) return nero_fail(NERO_ERR_ARG, "nero_bvh_trace_faces: more than (2^31 - 1) / 3 rays: call in chunks");
    if (n == 0) return NERO_OK;
    Handle* h = (Handle*)handle;
    with_walk(h, [&](auto overlap, int threads) {
        hipLaunchKernelGGL(trace_faces_kernel<decltype(overlap)::value>, dim3(grid_blocks(n, threads)), dim3(threads), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->b.d_face, h->root, rays_o, rays_d, n, depth, face, bary);
    });
    return nero_check_launch("nero_bvh_trace_faces");
}

int nero_env_lookup(const float* env, int h, int w, int convention, const float* rot, const float* dirs, int64_t n, float clamp_max,
                    float* rgb, void* stream) {
    EnvMap E;
    if (check_env("nero_env_lookup", env, h, w, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (!dirs || !rgb) return nero_fail(NERO_ERR_ARG, "nero_env_lookup: null pointer");
    if (n < 0 || n > 2147483647ll) return nero_fail(NERO_ERR_ARG, "nero_env_lookup: n must lie in [0, 2^31 - 1]: call in chunks");
    if (n == 0) return NERO_OK;
    hipLaunchKernelGGL(env_lookup_kernel, dim3(grid_blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, E, dirs, n, rgb);
    return nero_check_launch("nero_env_lookup");
}

int nero_relight_rays(const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type, float* rays_o,
                      float* rays_d, unsigned char* dead, void* stream) {
    if (!pt || !tab_d || !tab_s || !rays_o || !rays_d) return nero_fail(NERO_ERR_ARG, "nero_relight_rays: null pointer");
    if (check_samples("nero_relight_rays", P, Dd, Ds, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const int total = P * (Dd + Ds);                                   // at most P * padded(D)
    hipLaunchKernelGGL(rays_kernel<false>, dim3(grid_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, pt, tab_d, tab_s, nullptr, nullptr,
                       total, Dd, Ds, 0, geometry_type, nullptr, nullptr, 1, 1, rays_o, rays_d, dead, nullptr, nullptr);
    return nero_check_launch("nero_relight_rays");
}

int nero_relight_mis_rays(const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l, int P, int Dd, int Ds,
                          int Dl, int geometry_type, const int64_t* cdf, const int64_t* info, int gh, int gw, float* rays_o, float* rays_d,
                          unsigned char* dead, int* cell, float* pdf_l, void* stream) {
    if (!pt || !tab_d || !tab_s || !tab_l || !cdf || !info || !rays_o || !rays_d) return nero_fail(NERO_ERR_ARG, "nero_relight_mis_rays: null pointer");
    if (check_mis_samples("nero_relight_mis_rays", P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    if (!map_ok(gh, gw)) return nero_fail(NERO_ERR_ARG, "nero_relight_mis_rays: gh and gw must be in [1, 16384] and gh * gw at most 2^26");
    if (P == 0) return NERO_OK;
    const int total = P * (Dd + Ds + Dl);                              // at most P * padded(D)
    hipLaunchKernelGGL(rays_kernel<true>, dim3(grid_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, pt, tab_d, tab_s, tab_l, rand_l, total,
                       Dd, Ds, Dl, geometry_type, cdf, info, gh, gw, rays_o, rays_d, dead, cell, pdf_l);
    return nero_check_launch("nero_relight_mis_rays");
}

}  // extern "C"
