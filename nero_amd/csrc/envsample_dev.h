// envsample_dev.h -- the device functions that envsample.hip (the light table), relight.hip (the ray export) and relight_estimator.hip (the
// estimator) share: the grid's directions, the light draw (env_draw), the density (env_pdf, env_lookup_cell), the sample set of the three
// strategies (mis_ray) and the MIS per-sample terms (mis_weight, mis_terms), and the host checks of the MIS sample counts and the table's
// size.  One definition each, so that the export, the primary estimator and a bounce's one sample draw the same directions and weigh them
// by the same mixture bit for bit.  Every function switches floating-point contraction off for its own body: every operation is the one
// include/nero_hip_envsample.h writes.
// Include after relight_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "envsample_plan.h"
#include "relight_dev.h"

namespace nero_envsample {

using nero_relight::EnvMap; using nero_relight::relight_ray; using nero_relight::dotp;
using nero_shade::PI_F; using nero_shade::TWO_PI; using nero_shade::sat;

typedef unsigned long long u64;
constexpr float ONE_BELOW = 0x1.fffffep-1f;  // 1 - 2^-24
// S, the scale of the specular integrand.  The two-strategy kernel divides each sample by its own strategy's density times that strategy's
// share (brdf_weight), so its specular mean over all D samples is the SUM of two complete estimates of f = F L D_ggx G / (4 NoV), and the
// Stage-II materials were fitted under that sum.  The cosine half is Int f: p_d is the density its samples have.  The GGX half is NOT: it
// divides by p_code = D_ggx NoH / (4 HoV + 1e-5), the half-vector density, while the sampler lays its GGX lobe around the reflection r
// itself, which gives the direction the density p_act = D(w.r) w.r -- so that half's expectation is Int f p_act / p_code.  Quadrature
// (tests/test_relight_mis_cpu.py) puts the sum at 2.03 Int f for alpha = 0.09 but at 1.5 .. 1.7 Int f for alpha = 0.36 and 0.81: no constant
// serves.  The balance heuristic estimates an integral once, so it is given the integrand whose integral IS that sum, f S(w) with
//   S(w) = SPEC_COSINE_HALF + p_act / (p_code + 1e-5),
// and its mixture takes p_act, the density the GGX samples have: samples = (Dd, Ds) and samples = (Dd, Ds, Dl) converge to the same picture.
constexpr float SPEC_COSINE_HALF = 1.0f;   // the cosine half's share of S: Int f, once

// ---- the grid ---------------------------------------------------------------------------------------------------------------------------
// direction of (u, v), and the cosine of its elevation
__device__ __forceinline__ float grid_dir(float u, float v, float* d) {
#pragma clang fp contract(off)
    const float el = (v - 0.5f) * PI_F, phi = (u - 0.5f) * TWO_PI;
    const float ce = cosf(el);
    d[0] = -(ce * cosf(phi));
    d[1] = ce * sinf(phi);
    d[2] = sinf(el);
    return ce;
}

// ---- drawing, density -------------------------------------------------------------------------------------------------------------------
struct LightTab { const int64_t* cdf; int gh, gw; u64 total; };

__device__ __forceinline__ float clamp_unit(double x) { return (float)fmin(fmax(x, 0.0), (double)ONE_BELOW); }

// p_l of cell k for a direction of grid coordinate v (header, DENSITY)
__device__ __forceinline__ float env_pdf(const LightTab& T, int64_t k, float v) {
#pragma clang fp contract(off)
    const u64 prev = k > 0 ? (u64)T.cdf[k - 1] : 0ull;
    const u64 wc = (u64)T.cdf[k] - prev;
    const float pc = T.total > 0 ? (float)((double)wc / (double)T.total) : 0.f;
    const float ce = fmaxf(cosf((v - 0.5f) * PI_F), 1e-6f);
    return (pc * ((float)T.gh * (float)T.gw)) / ((TWO_PI * PI_F) * ce);
}

// the light sample of the variates (u1, u2) (header, A LIGHT SAMPLE): direction w, its cell, its density.  Every read of the running sum
// lies in [0, gh gw - 1] whatever the array holds.
__device__ __forceinline__ void env_draw(const LightTab& T, float u1, float u2, float* w, int& cell, float& pdf) {
#pragma clang fp contract(off)
    const int gh = T.gh, gw = T.gw;
    const u64 total = T.total;
    int row = 0, col = 0;
    float x1 = 0.5f, x2 = 0.5f;
    if (total > 0) {
        const double s1 = (double)u1 * (double)total;
        u64 t1 = (u64)s1;
        if (t1 > total - 1) t1 = total - 1;
        int lo = 0, hi = gh - 1;                                       // R_{gh-1} = total > t1: the answer lies in [lo, hi]
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((u64)T.cdf[(int64_t)mid * gw + (gw - 1)] > t1) hi = mid; else lo = mid + 1;
        }
        row = lo;
        const u64 base = row > 0 ? (u64)T.cdf[(int64_t)row * gw - 1] : 0ull;
        const u64 rowtot = (u64)T.cdf[(int64_t)row * gw + (gw - 1)] - base;
        x1 = clamp_unit((s1 - (double)base) / (double)rowtot);
        const double s2 = (double)u2 * (double)rowtot;
        u64 r2 = (u64)s2;
        if (rowtot > 0 && r2 > rowtot - 1) r2 = rowtot - 1;
        const u64 t2 = base + r2;
        const int64_t at = (int64_t)row * gw;
        lo = 0; hi = gw - 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((u64)T.cdf[at + mid] > t2) hi = mid; else lo = mid + 1;
        }
        col = lo;
        const int64_t k = at + col;
        const u64 prev = k > 0 ? (u64)T.cdf[k - 1] : 0ull;
        const u64 wc = (u64)T.cdf[k] - prev;
        x2 = clamp_unit((s2 - (double)(prev - base)) / (double)wc);
    }
    const float u = ((float)col + x2) / (float)gw;
    const float v = 1.0f - ((float)row + x1) / (float)gh;
    (void)grid_dir(u, v, w);
    cell = row * gw + col;
    pdf = env_pdf(T, (int64_t)cell, v);
}

// the cell and the density of a direction another strategy drew (header: (u, v) of a direction, cell of a direction)
__device__ __forceinline__ void env_lookup_cell(const LightTab& T, const float* d, int& cell, float& pdf) {
#pragma clang fp contract(off)
    const float u = atan2f(d[1], -d[0]) / TWO_PI + 0.5f;
    const float v = atan2f(d[2], sqrtf(d[0] * d[0] + d[1] * d[1])) / PI_F + 0.5f;
    const int row = (int)fminf(fmaxf(floorf((1.0f - v) * (float)T.gh), 0.f), (float)(T.gh - 1));     // (fmaxf / fminf drop a NaN)
    const int col = (int)fminf(fmaxf(floorf(u * (float)T.gw), 0.f), (float)(T.gw - 1));
    cell = row * T.gw + col;
    pdf = env_pdf(T, (int64_t)cell, v);
}

__device__ __forceinline__ float frac_shift(float t, float shift) {
#pragma clang fp contract(off)
    const float s = t + shift;
    return fminf(fmaxf(s - floorf(s), 0.f), ONE_BELOW);
}

// Sample j of D = Dd + Ds + Dl of the point record q: relight_ray() below Dd + Ds, then the light samples.  -> dead
__device__ __forceinline__ bool mis_ray(const float* q, const float* __restrict__ tab_d, const float* __restrict__ tab_s,
                                        const float* __restrict__ tab_l, const float* shift, int j, int Dd, int Ds, int geom, const LightTab& T,
                                        float* w, float* o, int& cell, float& pdf) {
#pragma clang fp contract(off)
    if (j < Dd + Ds) {
        const bool dead = relight_ray(q, tab_d, tab_s, j, Dd, geom, w, o);
        env_lookup_cell(T, w, cell, pdf);
        return dead;
    }
    const int l = j - (Dd + Ds);
    const float u1 = frac_shift(tab_l[2 * l], shift ? shift[0] : 0.f), u2 = frac_shift(tab_l[2 * l + 1], shift ? shift[1] : 0.f);
    env_draw(T, u1, u2, w, cell, pdf);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = q[29 + c] + w[c] * 1e-5f;
    return geom == 0 && dotp(q + 3, w) < -1e-6f;
}

// ---- the estimator ----------------------------------------------------------------------------------------------------------------------
// of direction w at the point q, with the saturations, D_ggx and G of brdf_weight: dterm = (NoL / pi) / p_mix (0 where p_mix or NoL is 0),
// W = S(w) D_ggx G / (4 NoV p_mix + 1e-5), fc = (1 - HoV)^5; p_mix = (Dd p_d + Ds p_act + Dl p_l) / D
__device__ __forceinline__ void mis_weight(const float* q, const float* w, float pl, int Dd, int Ds, int Dl, int geom, float& dterm, float& W,
                                           float& fc) {
#pragma clang fp contract(off)
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
    const float pd = nol / PI_F, pcode = dg * noh / (4.f * hov + 1e-5f);
    const float cr = sat(dotp(q + 6, w));
    const float tr = cr * cr * (a2 - 1.f) + 1.f;
    const float pact = a2 / fmaxf(PI_F * tr * tr, 1e-30f) * cr;
    const float pmix = (((float)Dd * pd + (float)Ds * pact) + (float)Dl * pl) / (float)(Dd + Ds + Dl);
    dterm = (nol > 0.f && pmix > 0.f) ? pd / pmix : 0.f;
    const float S = SPEC_COSINE_HALF + pact / (pcode + 1e-5f);
    W = S * dg * G / (4.f * nov * pmix + 1e-5f);
}

// one sample's diffuse and specular terms under the mixture, for the radiance L it fetched: what relight_kernel<MIS> adds up
__device__ __forceinline__ void mis_terms(const float* q, const float* w, float pl, int Dd, int Ds, int Dl, int geom, const float* L, float* diff,
                                          float* spec) {
#pragma clang fp contract(off)
    float dterm, W, fc;
    mis_weight(q, w, pl, Dd, Ds, Dl, geom, dterm, W, fc);
    const float m = q[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float F0 = 0.04f * (1.f - m) + m * q[11 + c];
        const float Fr = F0 + (1.f - F0) * fc;
        spec[c] = Fr * L[c] * W;
        diff[c] = q[11 + c] * (1.f - m) * L[c] * dterm;
    }
}

// ---- argument checks --------------------------------------------------------------------------------------------------------------------
inline int check_table_size(const char* who, int eh, int ew) {
    char msg[200];
    if (eh >= 1 && ew >= 1 && eh <= MAX_SIDE && ew <= MAX_SIDE && !map_ok(eh, ew)) {
        snprintf(msg, sizeof(msg), "%s: map of %d x %d texels: a light table holds at most 2^26 cells (nero_bvh_relight serves larger maps)", who,
                 eh, ew);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
}

inline int check_mis_samples(const char* who, int P, int Dd, int Ds, int Dl, int geometry_type) {
    char msg[160];
    if (P < 0) { snprintf(msg, sizeof(msg), "%s: P must be >= 0", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!nero_relight::mis_samples_ok(Dd, Ds, Dl)) { snprintf(msg, sizeof(msg), "%s: Dd, Ds and Dl must lie in [1, 4096]", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (geometry_type < 0 || geometry_type > 1) { snprintf(msg, sizeof(msg), "%s: geometry_type must be 0 or 1", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (!nero_relight::total_ok(P, Dd, Ds, Dl)) {
        snprintf(msg, sizeof(msg), "%s: P * (Dd + Ds + Dl padded to 64) must be at most 2^31 - 64: call in chunks", who);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
}

}  // namespace nero_envsample
