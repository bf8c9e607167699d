// relight.hip -- relighting the Stage-II mesh under a lat-long environment map (include/nero_hip_relight.h).  Replaces what the reference
// hands to Blender Cycles in relight.py with direct lighting and shadows on the mesh tracer's BVH:
//   * nero_bvh_export_faces / nero_bvh_trace_faces: the closest-hit walks of bvh_walk.h expanded once more (ANY = false), reporting WHICH
//     triangle was hit (through the builders' leaf-order table, Bvh::d_face) and where on it (the u, v of tri_test's own arithmetic);
//   * nero_env_lookup: bilinear radiance of a lat-long map, in this project's own grid (the inverse of nero_env_encode's directions) or in
//     the equirectangular mapping an .hdr made for the reference's relight.py --hdr assumes;
//   * nero_relight_rays: the sample set -- relight_ray() of relight_dev.h IS the definition: the directions of sample_diffuse_directions /
//     sample_specular_directions (field.py:768-810) as mc_shade.hip forms them, restated here with every product and sum rounded on its own
//     so that the two kernels that expand it agree bit for bit;
//   * nero_bvh_relight: the same rays from the same function, walked as shadow rays (any hit within the miss distance) without ever being
//     stored, the environment looked up for the free ones, weighed by the estimator of shade_mixed (field.py:950-998) and reduced per point
//     in a fixed order: shuffle butterfly inside the wavefront, one partial per wavefront, a finishing pass in index order.  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nero_hip.h"
#include "../../include/nero_hip_relight.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "relight_plan.h"
#include "relight_dev.h"                     // env_sample, relight_ray, brdf_weight, the any-hit walk and the argument checks: shared with
                                             // envsample.hip, which expands the same sample set and reads the same radiance

namespace {

using namespace nero_bvh;
using namespace nero_relight;              // relight_plan.h (samples_ok, total_ok, waves_per_point, workspace_bytes, grid_blocks), relight_dev.h
constexpr int PRIV_THREADS = 256;          // workgroup of the private-stack kernels (as trace_kernel)

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

// ---- the sample set (relight_ray: relight_dev.h) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relight_rays_kernel(const float* __restrict__ pt, const float* __restrict__ tab_d,
                                                           const float* __restrict__ tab_s, int total, int Dd, int Ds, int geom,
                                                           float* __restrict__ ro, float* __restrict__ rd, unsigned char* __restrict__ dead) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;             // ray p D + j
    if (row >= total) return;
    const int D = Dd + Ds;
    const int p = row / D, j = row - p * D;
    const float* q = pt + (size_t)p * 32;
    float w[3], o[3];
    const bool dd = relight_ray(q, tab_d, tab_s, j, Dd, geom, w, o);
    const size_t at = (size_t)row * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ro[at + c] = o[c]; rd[at + c] = w[c]; }
    if (dead) dead[row] = dd ? 1 : 0;
}

// ---- the estimator (brdf_weight, two_strategy_terms, the any-hit walk: relight_dev.h) -----------------------------------------------------------------------
// One lane per (point, sample): wavefront W of the grid is chunk W % wpp of point W / wpp, lane l its sample (W % wpp) 64 + l; samples at or
// past D are padding.  partial [P wpp, 6]: the wavefront's sums of the diffuse and the specular terms, added by a shuffle butterfly (the same
// order on every run).
template <bool OVERLAP>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void relight_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, int root, const float* __restrict__ pt, const float* __restrict__ tab_d,
    const float* __restrict__ tab_s, int P_, int Dd, int Ds, int wpp, int geom, EnvMap E, float* __restrict__ partial) {
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    (void)st;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // below 2^31 (relight_plan.h)
    const int wave = g >> 6, lane = threadIdx.x & 63;
    const int p = wave / wpp;
    if (p >= P_) return;                                               // a whole wavefront of the last workgroup
    const int D = Dd + Ds;
    const int j = (wave - p * wpp) * 64 + lane;
    const float* q = pt + (size_t)p * 32;
    float diff[3] = {0.f, 0.f, 0.f}, spec[3] = {0.f, 0.f, 0.f};
    if (j < D) {
        float d[3], o[3];
        const bool dead = relight_ray(q, tab_d, tab_s, j, Dd, geom, d, o);
        NERO_RELIGHT_ANY_HIT(blocked, MISS_DEPTH, dead ? NONE : root)
        if (!dead && !blocked) {
            float L[3];
            env_sample(E, d, L);
            two_strategy_terms(q, d, j, Dd, Ds, geom, L, diff, spec);
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
        float* out = partial + (size_t)wave * PARTIAL_FLOATS;
#pragma unroll
        for (int c = 0; c < 3; ++c) { out[c] = diff[c]; out[3 + c] = spec[c]; }
    }
}

// a point's partials added in index order
__global__ __launch_bounds__(256) void relight_finish_kernel(const float* __restrict__ partial, int P_, int wpp, int Dd, int Ds,
                                                             float* __restrict__ rgb_lin, float* __restrict__ diffuse_lin,
                                                             float* __restrict__ spec_lin) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P_) return;
    float s[PARTIAL_FLOATS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < wpp; ++k) {
        const float* in = partial + ((size_t)p * wpp + k) * PARTIAL_FLOATS;
#pragma unroll
        for (int c = 0; c < PARTIAL_FLOATS; ++c) s[c] += in[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float df = s[c] / (float)Dd, sp = s[3 + c] / (float)(Dd + Ds);
        rgb_lin[(size_t)p * 3 + c] = df + sp;
        if (diffuse_lin) diffuse_lin[(size_t)p * 3 + c] = df;
        if (spec_lin) spec_lin[(size_t)p * 3 + c] = sp;
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
    if (h->mode == 0)
        hipLaunchKernelGGL(trace_faces_kernel<false>, dim3(grid_blocks(n, PRIV_THREADS)), dim3(PRIV_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->b.d_face, h->root, rays_o, rays_d, n, depth, face, bary);
    else
        hipLaunchKernelGGL(trace_faces_kernel<true>, dim3(grid_blocks(n, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->b.d_face, h->root, rays_o, rays_d, n, depth, face, bary);
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
    hipLaunchKernelGGL(relight_rays_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, pt, tab_d, tab_s, total, Dd, Ds,
                       geometry_type, rays_o, rays_d, dead);
    return nero_check_launch("nero_relight_rays");
}

size_t nero_relight_workspace_bytes(int P, int Dd, int Ds) {
    if (!samples_ok(Dd, Ds) || !total_ok(P, Dd, Ds)) return 0;
    return workspace_bytes(P, Dd, Ds);
}

int nero_bvh_relight(void* handle, const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                     const float* env, int eh, int ew, int convention, const float* rot, float clamp_max, float* rgb_lin, float* diffuse_lin,
                     float* spec_lin, void* ws, size_t ws_bytes, void* stream) {
    if (!handle || !pt || !tab_d || !tab_s || !rgb_lin) return nero_fail(NERO_ERR_ARG, "nero_bvh_relight: null handle or pointer");
    if (check_samples("nero_bvh_relight", P, Dd, Ds, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env("nero_bvh_relight", env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    if (!ws || ((uintptr_t)ws & 3u) != 0 || ws_bytes < workspace_bytes(P, Dd, Ds))
        return nero_fail(NERO_ERR_ARG, "nero_bvh_relight: workspace missing, misaligned or smaller than nero_relight_workspace_bytes");
    Handle* h = (Handle*)handle;
    const int wpp = waves_per_point(Dd, Ds);
    const long long total = total_lanes(P, Dd, Ds);
    float* partial = (float*)ws;
    if (h->mode == 0)
        hipLaunchKernelGGL(relight_kernel<false>, dim3(grid_blocks(total, PRIV_THREADS)), dim3(PRIV_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pt, tab_d, tab_s, P, Dd, Ds, wpp, geometry_type, E, partial);
    else
        hipLaunchKernelGGL(relight_kernel<true>, dim3(grid_blocks(total, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pt, tab_d, tab_s, P, Dd, Ds, wpp, geometry_type, E, partial);
    if (nero_check_launch("nero_bvh_relight") != NERO_OK) return NERO_ERR_LAUNCH;
    hipLaunchKernelGGL(relight_finish_kernel, dim3(grid_blocks(P, 256)), dim3(256), 0, (hipStream_t)stream, partial, P, wpp, Dd, Ds, rgb_lin,
                       diffuse_lin, spec_lin);
    return nero_check_launch("nero_bvh_relight (finish)");
}

}  // extern "C"
