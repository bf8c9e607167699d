// tex_lod.h -- the level-of-detail rule and the texel addressing that every mip-mapped lookup of the library shares (tex_fetch.hip: the
// material records of include/nero_hip_texfetch.h; detail_transfer.hip: the normal-map records of include/nero_transfer.h).  Device code
// only; the pyramid's sizes and offsets are tex_fetch_plan.h's Plan, whatever a record holds.
// Compiled without floating-point contraction: every fp32 operation is the one the numpy restatements of the tests perform.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "tex_fetch_plan.h"

#pragma clang fp contract(off)

namespace nero_texfetch {

__device__ __forceinline__ bool in_range(int j, int64_t n) { return j >= 0 && (int64_t)j < n; }

__device__ __forceinline__ float lerp(float p, float q, float f) { return p + f * (q - p); }

// where a coordinate falls in a level n texels wide: c = fminf(fmaxf(u n - 0.5, -1), n) (NaN -> -1), i0 = floorf(c) in [-1, n], f = c - i0
struct Axis {
    int i0;
    float f;
};

__device__ __forceinline__ Axis axis_of(float u, int n) {
    const float nf = (float)n;
    const float c = fminf(fmaxf(u * nf - 0.5f, -1.0f), nf);                 // fmaxf and fminf return the other operand for a NaN
    const float fl = floorf(c);
    Axis a;
    a.i0 = (int)fl;
    a.f = c - fl;
    return a;
}

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// the four taps of the bilinear fetch at (u, v) in level k, as record numbers inside the pyramid: off[k] + y w_k + x with y and x clamped to
// the level, so below off[k] + h_k w_k <= records whatever the coordinates are
struct Taps {
    int64_t r00, r01, r10, r11;
    Axis ax, ay;
};

__device__ __forceinline__ Taps taps_of(const Plan& P, int k, float u, float v) {
    const int wk = P.w[k], hk = P.h[k];
    Taps t;
    t.ax = axis_of(u, wk);
    t.ay = axis_of(v, hk);
    const int x0 = clamp_index(t.ax.i0, wk), x1 = clamp_index(t.ax.i0 + 1, wk);  // in [0, w_k - 1]
    const int y0 = clamp_index(t.ay.i0, hk), y1 = clamp_index(t.ay.i0 + 1, hk);  // in [0, h_k - 1]
    const int64_t r0 = P.off[k] + (int64_t)y0 * wk, r1 = P.off[k] + (int64_t)y1 * wk;
    t.r00 = r0 + x0;
    t.r01 = r0 + x1;
    t.r10 = r1 + x0;
    t.r11 = r1 + x1;
    return t;
}

// the level of a footprint: s = fmaxf(((depth spread) scale) lod_scale, 1) (a NaN gives 1), l = min(exponent of s, L - 1), t = s 2^-l - 1 in
// [0, 1) below the top level (exact), 0 at it
struct Lod {
    int l;
    float t;
};

__device__ __forceinline__ Lod lod_of(float depth, float spread, float scale, float lod_scale, int L) {
    const float s = fmaxf(((depth * spread) * scale) * lod_scale, 1.0f);              // >= 1, or +inf; a NaN gives 1
    const int e = (int)((__float_as_uint(s) >> 23) & 255u) - 127;                     // in [0, 128]
    Lod o;
    o.l = e < L - 1 ? e : L - 1;
    o.t = o.l < L - 1 ? s * __uint_as_float((uint32_t)(127 - o.l) << 23) - 1.0f : 0.0f;   // l == e there: s 2^-l in [1, 2), exact
    return o;
}

// the UV of a hit: a(X) = (((1 - u) - v) X[j0] + u X[j1]) + v X[j2] over vt [Vt,2]
__device__ __forceinline__ void hit_uv(const float* __restrict__ vt, int j0, int j1, int j2, float bu, float bv, float* u, float* v) {
    const float w0 = (1.0f - bu) - bv;
    *u = (w0 * vt[2 * (int64_t)j0] + bu * vt[2 * (int64_t)j1]) + bv * vt[2 * (int64_t)j2];
    *v = (w0 * vt[2 * (int64_t)j0 + 1] + bu * vt[2 * (int64_t)j1 + 1]) + bv * vt[2 * (int64_t)j2 + 1];
}

}  // namespace nero_texfetch
