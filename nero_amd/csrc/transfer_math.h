// transfer_math.h -- the arithmetic of detail_transfer.hip that more than one kernel performs: THE FRAME and THE BYTES of
// include/nero_transfer.h.  fp32, one operation at a time, in the order the header states and tests/transfer_ref.py restates.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace nero_transfer {

__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ bool finite3(const float* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

struct Frame {
    float n[3], t[3], b[3];                                     // unit normal, T', B
    float len;                                                  // |N|
    bool ok;                                                    // |N| finite and not zero
};

__device__ __forceinline__ void project(const float* T, const float* n, float* p) {
    const float d = dot3(T, n);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = T[k] - d * n[k];
}

__device__ __forceinline__ Frame frame_of(const float* N, const float* T, int sign) {
    Frame F;
    F.len = sqrtf(dot3(N, N));
    F.ok = isfinite(F.len) && F.len != 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) F.n[k] = N[k] / F.len;
    float p[3];
    project(T, F.n, p);
    float pp = dot3(p, p);
    if (!(pp > 1e-12f * dot3(T, T))) {                          // no direction: the axis of smallest |n_k|, the lowest k among equals
        const float a0 = fabsf(F.n[0]), a1 = fabsf(F.n[1]), a2 = fabsf(F.n[2]);
        const int k = (a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2);
        const float d = k == 0 ? F.n[0] : (k == 1 ? F.n[1] : F.n[2]);    // dot(axis, n): the products with 0 and 1 are exact
        p[0] = (k == 0 ? 1.0f : 0.0f) - d * F.n[0];
        p[1] = (k == 1 ? 1.0f : 0.0f) - d * F.n[1];
        p[2] = (k == 2 ? 1.0f : 0.0f) - d * F.n[2];
        pp = dot3(p, p);
    }
    const float pl = sqrtf(pp);
#pragma unroll
    for (int k = 0; k < 3; ++k) F.t[k] = p[k] / pl;
    const float s = sign < 0 ? -1.0f : 1.0f;
    F.b[0] = s * (F.n[1] * F.t[2] - F.n[2] * F.t[1]);
    F.b[1] = s * (F.n[2] * F.t[0] - F.n[0] * F.t[2]);
    F.b[2] = s * (F.n[0] * F.t[1] - F.n[1] * F.t[0]);
    return F;
}

// x / |x|; false where the length is zero or not finite
__device__ __forceinline__ bool unit3(const float* x, float* out) {
    const float l = sqrtf(dot3(x, x));
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = x[k] / l;
    return isfinite(l) && l != 0.0f;
}

// clamp(lrintf(127 x) + 128, 1, 255) of a component in [-1, 1] (anything finite is clamped)
__device__ __forceinline__ uint32_t nmap_byte(float x) {
    const float r = rintf(127.0f * x) + 128.0f;                 // round to nearest even, as lrintf; exact in fp32 for |x| <= 1
    return (uint32_t)fminf(fmaxf(r, 1.0f), 255.0f);
}

__device__ __forceinline__ float nmap_decode(uint32_t b) { return ((float)b - 128.0f) / 127.0f; }

}  // namespace nero_transfer
