// relight.hip -- relighting the Stage-II mesh under a lat-long environment map (include/nero_hip_relight.h).  Replaces what the reference
// hands to Blender Cycles in relight.py with direct lighting and shadows on the mesh tracer's BVH:
//   * nero_bvh_export_faces / nero_bvh_trace_faces: the closest-hit walks of bvh_walk.h expanded once more (ANY = false), reporting WHICH
//     triangle was hit (through the builders' leaf-order table, Bvh::d_face) and where on it (the u, v of tri_test's own arithmetic);
//   * nero_env_lookup: bilinear radiance of a lat-long map, in this project's own grid (the inverse of nero_env_encode's directions) or in
//     the equirectangular mapping an .hdr made for the reference's relight.py --hdr assumes;
//   * nero_relight_rays: the sample set -- relight_ray() below IS the definition: the directions of sample_diffuse_directions /
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
#include "shade_math.h"                      // PI_F, TWO_PI, HALF_PI, sat -- and nothing else: the header says why

namespace {

using namespace nero_bvh;
using nero_shade::PI_F; using nero_shade::TWO_PI; using nero_shade::HALF_PI; using nero_shade::sat;
using namespace nero_relight;              // samples_ok, total_ok, waves_per_point, workspace_bytes, grid_blocks (relight_plan.h)
constexpr float MISS_DEPTH = 10.0f;        // the tracer's miss distance
constexpr int PRIV_THREADS = 256;          // workgroup of the private-stack kernels (as trace_kernel)
constexpr int ENV_MAX_SIZE = 16384;

// ---- closest hit with the face ----------------------------------------------------------------------------------------------------------
// (u, v) of tri_test on triangle `best`: the same operations in the same order
__device__ __forceinline__ void hit_bary(const Tri* __restrict__ tris, int best, const float* o, const float* d, float& u, float& v) {
#pragma clang fp contract(off)
    const TriQ q = load_tri(tris, best);
    const float v0[3] = {q.a.x, q.a.y, q.a.z}, e1[3] = {q.a.w, q.b.x, q.b.y}, e2[3] = {q.b.z, q.b.w, q.c.x};
    const float px = cross_c(d[1], e2[2], d[2], e2[1]), py = cross_c(d[2], e2[0], d[0], e2[2]), pz = cross_c(d[0], e2[1], d[1], e2[0]);
    const float det = dot3(e1[0], e1[1], e1[2], px, py, pz);
    const float inv = 1.0f / det;
    const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
    u = dot3(tx, ty, tz, px, py, pz) * inv;
    const float qx = cross_c(ty, e1[2], tz, e1[1]), qy = cross_c(tz, e1[0], tx, e1[2]), qz = cross_c(tx, e1[1], ty, e1[0]);
    v = dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
}

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

// ---- the environment map ----------------------------------------------------------------------------------------------------------------
struct EnvMap { const float* tex; int h, w, conv, has_rot; float R[9]; float clamp_max; };

// radiance of the map in direction d0 (any non-zero length): header, nero_env_lookup.  Texel coordinates are clamped as floats before they
// become integers (fmaxf / fminf drop a NaN), so every read lies inside the map whatever the direction holds.
__device__ __forceinline__ void env_sample(const EnvMap& E, const float* d0, float* rgb) {
#pragma clang fp contract(off)
    float d[3] = {d0[0], d0[1], d0[2]};
    if (E.has_rot) {
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = E.R[3 * k] * d0[0] + E.R[3 * k + 1] * d0[1] + E.R[3 * k + 2] * d0[2];
    }
    const int h = E.h, w = E.w;
    float fx, fy;
    int c0, c1;
    if (E.conv == 2) {
        const float u = atan2f(d[1], -d[0]) / TWO_PI + 0.5f;
        const float v = atan2f(d[2], sqrtf(d[0] * d[0] + d[1] * d[1])) / PI_F + 0.5f;
        const float x = fminf(fmaxf(u * (float)w - 0.5f, -0.5f), (float)w - 0.5f);
        fy = fminf(fmaxf((1.0f - v) * (float)h - 0.5f, 0.f), (float)(h - 1));
        const float xf = floorf(x);
        fx = x - xf;
        const int x0 = (int)xf;                               // -1 .. w - 1
        c0 = x0 < 0 ? w - 1 : x0;
        c1 = x0 + 1 >= w ? 0 : x0 + 1;
    } else {
        float az, el;
        if (E.conv == 1) { az = atan2f(d[1], d[0]); el = atan2f(d[2], sqrtf(d[0] * d[0] + d[1] * d[1])); }
        else             { az = atan2f(d[0], d[2]); el = atan2f(d[1], sqrtf(d[0] * d[0] + d[2] * d[2])); }
        float t = (az + HALF_PI) / TWO_PI;
        t = t - floorf(t);                                    // [0, 1): column (1 - t) (w - 1)
        const float x = fminf(fmaxf((1.0f - t) * (float)(w - 1), 0.f), (float)(w - 1));
        fy = fminf(fmaxf((1.0f - el / HALF_PI) * 0.5f * (float)(h - 1), 0.f), (float)(h - 1));
        const float xf = floorf(x);
        fx = x - xf;
        c0 = (int)xf;
        c1 = c0 + 1 > w - 1 ? w - 1 : c0 + 1;
    }
    const float yf = floorf(fy);
    const float gy = fy - yf;
    const int r0 = (int)yf;
    const int r1 = r0 + 1 > h - 1 ? h - 1 : r0 + 1;
    const float* a = E.tex + ((size_t)r0 * w + c0) * 3;
    const float* b = E.tex + ((size_t)r0 * w + c1) * 3;
    const float* c = E.tex + ((size_t)r1 * w + c0) * 3;
    const float* e = E.tex + ((size_t)r1 * w + c1) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float top = (1.0f - fx) * a[k] + fx * b[k];
        const float bot = (1.0f - fx) * c[k] + fx * e[k];
        float L = (1.0f - gy) * top + gy * bot;
        if (E.clamp_max > 0.f) L = fminf(L, E.clamp_max);
        rgb[k] = L;
    }
}

__global__ __launch_bounds__(256) void env_lookup_kernel(EnvMap E, const float* __restrict__ dirs, int64_t n, float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d[3] = {dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2]};
    float L[3];
    env_sample(E, d, L);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[i * 3 + k] = L[k];
}

// ---- the sample set ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dotp(const float* a, const float* b) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// Sample j of the point record q (mc_shade.hip, top: 3-5 n, 6-8 reflection, 10 alpha, 15-26 the two frames, 27 / 28 azimuth rotations,
// 29-31 p): direction w (j < Dd: cosine-weighted around n, field.py:768-787; else GGX around the reflection, :789-810), origin o = p + 1e-5 w
// (:859-860), dead = the rule of nero_mc_dead_rays.  Every product and sum rounded on its own, in the order written.
__device__ __forceinline__ bool relight_ray(const float* q, const float* __restrict__ tab_d, const float* __restrict__ tab_s, int j, int Dd,
                                            int geom, float* w, float* o) {
#pragma clang fp contract(off)
    if (j < Dd) {
        const float az_t = tab_d[2 * j], el = tab_d[2 * j + 1];
        float az = az_t * TWO_PI;
        if (q[27] >= 0.f) az = fmodf(az + q[27], TWO_PI);
        const float es = sqrtf(el + 1e-7f), cz = sqrtf(1.f - el + 1e-7f);
        const float cx = es * cosf(az), cy = es * sinf(az);
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = cx * q[15 + c] + cy * q[18 + c] + cz * q[3 + c];
    } else {
        const float az_t = tab_s[2 * (j - Dd)], el = tab_s[2 * (j - Dd) + 1];
        const float a = q[10];
        const float cost = sqrtf((1.0f - el + 1e-6f) / (1.0f + (a * a - 1.0f) * el + 1e-6f) + 1e-6f);
        const float sint = sqrtf(1.f - cost * cost + 1e-6f);
        float phi = TWO_PI * az_t;
        if (q[28] >= 0.f) phi = fmodf(phi + q[28], TWO_PI);
        const float cphi = cosf(phi), sphi = sinf(phi);
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = cphi * sint * q[21 + c] + sphi * sint * q[24 + c] + cost * q[6 + c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = q[29 + c] + w[c] * 1e-5f;
    return geom == 0 && j >= Dd && dotp(q + 3, w) < -1e-6f;
}

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

// ---- the estimator ----------------------------------------------------------------------------------------------------------------------
// W = D_ggx G / (4 NoV p + 1e-5) and the Fresnel factor fc = (1 - HoV)^5 of direction w at the point q (shade_mixed, field.py:950-998, as
// brdf_terms of mc_shade.hip states it): geom 0 = Schlick-GGX product (:892-903), 1 = height-correlated Smith (:905-913); p = the pdf of
// the strategy that drew the sample, weighted by its share wd = Dd / D or ws = Ds / D of the samples
__device__ __forceinline__ void brdf_weight(const float* q, const float* w, bool diffuse, float wd, float ws, int geom, float& W, float& fc) {
    const float* v = q;
    const float* n = q + 3;
    const float r = q[10], nov = q[14];
    const float hraw[3] = {v[0] + w[0], v[1] + w[1], v[2] + w[2]};
    const float hlen = fmaxf(sqrtf(dotp(hraw, hraw)), 1e-12f);
    const float H[3] = {hraw[0] / hlen, hraw[1] / hlen, hraw[2] / hlen};
    const float hov = sat(dotp(H, v)), nol = sat(dotp(n, w)), noh = sat(dotp(n, H));
    const float cc = sat(1.f - hov);
    fc = cc * cc * cc * cc * cc;
    const float a2 = r * r;
    float G;
    if (geom == 0) {
        const float k = r * 0.5f;
        const float gv = nov / (nov * (1.f - k) + k + 1e-5f), gl = nol / (nol * (1.f - k) + k + 1e-5f);
        G = gv * gl;
    } else {
        const float cv2 = nov * nov, cl2 = nol * nol;
        const float sv = sqrtf(1.f + a2 * ((1.f - cv2) / (cv2 + 1e-7f))), sl = sqrtf(1.f + a2 * ((1.f - cl2) / (cl2 + 1e-7f)));
        G = 2.f / (sv + sl);
    }
    const float t = noh * noh * (a2 - 1.f) + 1.f;
    const float dg = a2 / (PI_F * t * t + 1e-4f);
    const float prob = diffuse ? nol / PI_F * wd : dg * noh / (4.f * hov + 1e-5f) * ws;
    W = dg * G / (4.f * nov * prob + 1e-5f);
}

// bool HIT = does the ray (o, d) meet a triangle nearer than TMAX: the any-hit expansion of the walk that the kernel's OVERLAP selects (the
// pattern of visibility.hip).  In scope: nodes, tris, o, d, st.
#define NERO_RELIGHT_ANY_HIT(HIT, TMAX, CUR0)                                \
    bool HIT;                                                                \
    {                                                                        \
        float inv[3];                                                        \
        ray_inverse(d, inv);                                                 \
        if constexpr (OVERLAP) {                                             \
            NERO_WALK_OVERLAP(true, TMAX, CUR0)                              \
            HIT = best >= 0;                                                 \
        } else {                                                             \
            NERO_WALK_PRIVATE(true, TMAX, CUR0)                              \
            HIT = best >= 0;                                                 \
        }                                                                    \
    }

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
            float L[3], W, fc;
            env_sample(E, d, L);
            brdf_weight(q, d, j < Dd, (float)Dd / (float)D, (float)Ds / (float)D, geom, W, fc);
            const float m = q[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float F0 = 0.04f * (1.f - m) + m * q[11 + c];
                const float Fr = F0 + (1.f - F0) * fc;
                spec[c] = Fr * L[c] * W;
                if (j < Dd) diff[c] = q[11 + c] * (1.f - m) * L[c];
            }
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

int check_env(const char* who, const float* env, int h, int w, int convention, const float* rot, float clamp_max, EnvMap* E) {
    char msg[160];
    if (!env) { snprintf(msg, sizeof(msg), "%s: null environment map", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (h < 1 || w < 1 || h > ENV_MAX_SIZE || w > ENV_MAX_SIZE) {
        snprintf(msg, sizeof(msg), "%s: map of %d x %d texels: both sizes must be in [1, %d]", who, h, w, ENV_MAX_SIZE);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (convention < 0 || convention > 2) {
        snprintf(msg, sizeof(msg), "%s: convention %d: 0, 1 (the project's grid, is_real = 0 / 1) or 2 (equirectangular)", who, convention);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    E->tex = env; E->h = h; E->w = w; E->conv = convention; E->has_rot = rot != nullptr; E->clamp_max = clamp_max;
    for (int i = 0; i < 9; ++i) E->R[i] = rot ? rot[i] : (i % 4 == 0 ? 1.f : 0.f);
    return NERO_OK;
}

int check_samples(const char* who, int P, int Dd, int Ds, int geometry_type) {
    char msg[160];
    if (P < 0) { snprintf(msg, sizeof(msg), "%s: P must be >= 0", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!samples_ok(Dd, Ds)) { snprintf(msg, sizeof(msg), "%s: Dd and Ds must lie in [1, 4096]", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (geometry_type < 0 || geometry_type > 1) { snprintf(msg, sizeof(msg), "%s: geometry_type must be 0 or 1", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!total_ok(P, Dd, Ds)) {
        snprintf(msg, sizeof(msg), "%s: P * (Dd + Ds padded to 64) must be at most 2^31 - 64: call in chunks", who);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
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
