// relight_dev.h -- the device functions and argument checks that relight.hip, relight_estimator.hip and envsample.hip share: the environment
// lookup (env_sample), the sample set of the two BRDF strategies (relight_ray), the estimator's weight (brdf_weight) and per-sample terms
// (two_strategy_terms), the hit's (u, v) (hit_bary), the any-hit expansion of the BVH walks and the host's choice between the walks.
// One definition each, so that the ray exports and every estimator form the same directions and read the same radiance bit for bit.
// Include after bvh_walk.h, common.h, relight_plan.h and shade_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <type_traits>
#include "../../include/nero_hip.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "relight_plan.h"
#include "shade_math.h"                      // PI_F, TWO_PI, HALF_PI, sat -- and nothing else: the header says why

namespace nero_relight {

using nero_shade::PI_F; using nero_shade::TWO_PI; using nero_shade::HALF_PI; using nero_shade::sat;
constexpr float MISS_DEPTH = 10.0f;        // the tracer's miss distance
constexpr int ENV_MAX_SIZE = 16384;

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

// one sample's diffuse and specular terms for the radiance L it fetched: what relight_kernel adds up (a cosine sample alone carries a
// diffuse term).  Not under a contraction pragma, as the kernel's body never was.
__device__ __forceinline__ void two_strategy_terms(const float* q, const float* d, int j, int Dd, int Ds, int geom, const float* L, float* diff,
                                                   float* spec) {
    const int D = Dd + Ds;
    float W, fc;
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

// ---- closest hit with the face ----------------------------------------------------------------------------------------------------------
// (u, v) of tri_test on triangle `best`: the same operations in the same order
__device__ __forceinline__ void hit_bary(const nero_bvh::Tri* __restrict__ tris, int best, const float* o, const float* d, float& u, float& v) {
#pragma clang fp contract(off)
    using nero_bvh::cross_c; using nero_bvh::dot3;
    const nero_bvh::TriQ q = nero_bvh::load_tri(tris, best);
    const float v0[3] = {q.a.x, q.a.y, q.a.z}, e1[3] = {q.a.w, q.b.x, q.b.y}, e2[3] = {q.b.z, q.b.w, q.c.x};
    const float px = cross_c(d[1], e2[2], d[2], e2[1]), py = cross_c(d[2], e2[0], d[0], e2[2]), pz = cross_c(d[0], e2[1], d[1], e2[0]);
    const float det = dot3(e1[0], e1[1], e1[2], px, py, pz);
    const float inv = 1.0f / det;
    const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
    u = dot3(tx, ty, tz, px, py, pz) * inv;
    const float qx = cross_c(ty, e1[2], tz, e1[1]), qy = cross_c(tz, e1[0], tx, e1[2]), qz = cross_c(tx, e1[1], ty, e1[0]);
    v = dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
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

// ---- the walk of a tree -----------------------------------------------------------------------------------------------------------------
constexpr int PRIV_THREADS = 256;          // workgroup of the private-stack kernels (as trace_kernel)
// launch(OVERLAP as a std::bool_constant, threads per workgroup): PL_THREADS threads and the LDS stack where the tree is no deeper than
// PL_STACK (mode != 0), else PRIV_THREADS threads and the private stack
template <class Launch>
inline void with_walk(const nero_bvh::Handle* h, Launch&& launch) {
    if (h->mode == 0) launch(std::false_type{}, PRIV_THREADS);
    else launch(std::true_type{}, nero_bvh::PL_THREADS);
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
inline int check_env(const char* who, const float* env, int h, int w, int convention, const float* rot, float clamp_max, EnvMap* E) {
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

inline int check_samples(const char* who, int P, int Dd, int Ds, int geometry_type) {
    char msg[160];
    if (P < 0) { snprintf(msg, sizeof(msg), "%s: P must be >= 0", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!samples_ok(Dd, Ds, 0)) { snprintf(msg, sizeof(msg), "%s: Dd and Ds must lie in [1, 4096]", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (geometry_type < 0 || geometry_type > 1) { snprintf(msg, sizeof(msg), "%s: geometry_type must be 0 or 1", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!total_ok(P, Dd, Ds, 0)) {
        snprintf(msg, sizeof(msg), "%s: P * (Dd + Ds padded to 64) must be at most 2^31 - 64: call in chunks", who);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
}

}  // namespace nero_relight
