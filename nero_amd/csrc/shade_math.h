// shade_math.h -- the elementwise arithmetic that the shading units share: constants, clamps and sign, the sigmoid, sRGB and
// exp-clamp heads, the positional encoding of a 3-vector, the human-light plane test and the input row of the inner-light MLP.
// Included by shade.hip (Stage I), mc_shade.hip and mat_loss.hip (Stage II), step_glue.hip, envlight.hip, sampler.hip and relight.hip;
// device inline functions and constexpr only, so a unit that uses one piece pays for nothing else.
//
// Deliberately NOT here, each for a reason that sharing would break:
//   * srgb_grad.  shade.hip tests `x >= SRGB_EPS` and returns 0 otherwise, mat_loss.hip clamps with fmaxf: equal for every finite input,
//     different for NaN, and the fmaxf form changes the instructions of shade_combine_bwd_kernel and nerf_head_bwd_kernel.  Each file
//     keeps its own form (docs/experiments.md: an unmeasured lead).
//   * the softplus of the three MLP engines (mlp_engine.hip, mlp_split.hip, mlp_f16_util.h): different formulas on purpose.
//   * relight.hip's relight_ray, brdf_weight and dotp.  They restate mc_shade.hip's sampling and BRDF under `#pragma clang fp contract(off)`
//     so that two kernels agree bit for bit; the pragma does not reach an inlined callee, so one shared body would change one side's bits.
//   * sphere_dir (shade.hip) against sphere_exit (mc_shade.hip), and reg_points_kernel's frame (mat_loss.hip) against ortho3 (mc_shade.hip):
//     alike to the eye, different arithmetic.
//   * image_metrics.hip's templated block_sum: a wave butterfly first, not the tree of device_prims.h's block_tree_sum.
#pragma once
#include <hip/hip_runtime.h>
#include "rows.h"                                    // rows_put / rows_zero / rows_flush: put_inner_row's coalesced row stores

namespace nero_shade {

constexpr float PI_F = 3.14159265358979f, TWO_PI = 6.283185307179586f, HALF_PI = 1.5707963267948966f;

__device__ __forceinline__ float sat(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
// sign(0) = 0: the sub-gradient of |x| the ATen kernels of the reference use
__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// linear_to_srgb (utils/raw_utils.py:4-10)
constexpr float SRGB_EPS = 1.1920928955078125e-07f;     // torch.finfo(float32).eps
__device__ __forceinline__ float srgb_f(float x) {
    return x <= 0.0031308f ? (323.f / 25.f) * x : (211.f * powf(fmaxf(x, SRGB_EPS), 5.f / 12.f) - 11.f) / 200.f;
}

// the light head, ExpActivation (network/field.py:302-308): exp(min(raw, emax)); the clamp passes the gradient where exp_head_gate holds
// (the gate returns int on purpose: with bool the compare reaches the selects of shade_combine_bwd_kernel in the inverted form and the
//  kernel comes out with two register pairs swapped -- profiles/shared_shading_math_isa.txt)
__device__ __forceinline__ float exp_head(float raw, float emax) { return expf(fminf(raw, emax)); }
__device__ __forceinline__ int exp_head_gate(float raw, float emax) { return raw <= emax; }

// positional encoding of a 3-vector (Embedder / get_embedder, network/field.py:14-58): out[3 + 6 N_FREQ] = p, then sin(2^k p), cos(2^k p) for k < N_FREQ
template <int N_FREQ>
__device__ __forceinline__ void pe3(const float* p, float* out) {      // (unrolled: `out` stays in registers)
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = p[c];
    float f = 1.f;
#pragma unroll
    for (int k = 0; k < N_FREQ; ++k) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 + 6 * k + c] = sinf(p[c] * f);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[3 + 6 * k + 3 + c] = cosf(p[c] * f);
        f *= 2.f;
    }
}

// human ("photo capturer") light: intersection of the ray (p, rf) with the z = 0 plane of the human frame `pose` [3,4]
// (get_camera_plane_intersection, network/field.py:348-367); h = 1 when the ray reaches the photographer's region of that plane
// (predict_human_light, :536-542; get_human_light, :820-825: hits & |0.3 inter_xy| < 1.5 & dist > 0), else 0
struct HumanGeom { float px, py, pz, dx, dy, dz, dzp, dist, ix, iy, h; bool hits0; };
__device__ __forceinline__ HumanGeom human_geom(const float* __restrict__ pose, const float* p, const float* rf) {
    HumanGeom g;
    g.px = pose[0] * p[0] + pose[1] * p[1] + pose[2] * p[2] + pose[3];
    g.py = pose[4] * p[0] + pose[5] * p[1] + pose[6] * p[2] + pose[7];
    g.pz = pose[8] * p[0] + pose[9] * p[1] + pose[10] * p[2] + pose[11];
    g.dx = pose[0] * rf[0] + pose[1] * rf[1] + pose[2] * rf[2];
    g.dy = pose[4] * rf[0] + pose[5] * rf[1] + pose[6] * rf[2];
    g.dz = pose[8] * rf[0] + pose[9] * rf[1] + pose[10] * rf[2];
    g.hits0 = fabsf(g.dz) > 1e-4f;
    g.dzp = g.hits0 ? g.dz : 1e-4f;
    g.dist = -g.pz / g.dzp;
    g.ix = g.px + g.dist * g.dx;
    g.iy = g.py + g.dist * g.dy;
    const float mx = g.ix * 0.3f, my = g.iy * 0.3f;
    g.h = (g.hits0 && sqrtf(mx * mx + my * my) < 1.5f && g.dist > 0.f) ? 1.f : 0.f;
    return g;
}

// input row of the inner-light MLP (predict_specular_lights, network/field.py:557, 569; get_inner_lights, :812-818):
// X row = [PE-8(p) 51 | IDE(refl, rough) 72 | 0 x 5], ld 128, staged as columns 0..63 and 64..127.  All ROW_BLOCK threads of the block
// call it (rows_flush holds the barriers); z = 0 makes the thread's row a zero row.
__device__ __forceinline__ void put_inner_row(float* __restrict__ stage, const float (&pe)[51], const float (&e)[72], float z,
                                              float* __restrict__ X, int row0, int n_pad) {
    rows_put<64, 0, 51>(stage, pe, z);
    {
        float h[13];
#pragma unroll
        for (int c = 0; c < 13; ++c) h[c] = e[c];
        rows_put<64, 51, 13>(stage, h, z);
    }
    rows_flush<64>(stage, X, 128, 0, row0, n_pad);
    {
        float h[59];
#pragma unroll
        for (int c = 0; c < 59; ++c) h[c] = e[13 + c];
        rows_put<64, 0, 59>(stage, h, z);
    }
    rows_zero<64, 59, 5>(stage);
    rows_flush<64>(stage, X, 128, 64, row0, n_pad);
}

}  // namespace nero_shade
