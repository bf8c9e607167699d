// denoise.hip -- the edge-aware denoiser of the relighter's pictures (include/nero_hip_denoise.h): a variance pass over a
// 7 x 7 window and an a-trous pass of 25 taps at a stride, both steered by the guide weight of normals, tangent-plane distance and, for
// G = 4, four more guide channels.
//   A workgroup owns a TILE_W x TILE_H tile (denoise_plan.h) and one thread one output pixel; a workgroup strides over tiles where an
//   image has more than MAX_GRID of them.  Records are read with 16-byte loads (the taps of neighbouring lanes are neighbouring records,
//   so a wave's load is a run of contiguous bytes per row).  What bounds a pass is the latency of its loads, not their bytes: the loads of
//   one row of taps are issued together, ahead of their arithmetic, and where the taps of a tile share a halo -- the variance window, the
//   strides 1 and 2 -- the tile and its halo are staged in LDS first (DESIGN.md 9.12.3 has the measurements behind both).  Sums run in
//   row-major tap order in registers: no atomics, the same bits on every run, and the same bits from the staged and the direct form.
// The file is compiled without floating-point contraction: every fp32 operation is the one the numpy restatement of the tests performs
// (expf's last place excepted).  Wide LOADS only: all arithmetic is written per component (tests/test_no_packed_fp32.py).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip_denoise.h"
#include "common.h"
#include "denoise_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_denoise;

struct Params {
    int k;                                                        // squarings of the normal weight
    float sigma_l, sigma_p, sg2;                                  // sg2 = sigma_g sigma_g (unused for G = 0)
};

__device__ __forceinline__ float lum_of(const float4& s) { return (0.2126f * s.x + 0.7152f * s.y) + 0.0722f * s.z; }

// a guide record: (nx, ny, nz, valid), (px, py, pz, 0) and, for G = 4, (g0..g3)
template <int G>
struct Guide {
    float4 n, p, g;
};

template <int G>
__device__ __forceinline__ Guide<G> load_guide(const float4* __restrict__ guide, int64_t i) {
    Guide<G> r;
    const float4* at = guide + i * (G == 4 ? 3 : 2);
    r.n = at[0];
    r.p = at[1];
    if (G == 4) r.g = at[2];
    return r;
}

// one tap: the records of a pixel; a tap outside the image carries valid = 0
template <int G>
struct Tap {
    Guide<G> g;
    float4 s;
};

// the tap at (qy, qx) from memory.  Outside the image the nearest pixel inside is read and marked invalid: a tap's loads wait for no test,
// so the loads of a whole row of taps are in flight together
template <int G>
__device__ __forceinline__ Tap<G> load_tap(const float4* __restrict__ guide, const float4* __restrict__ sig, int64_t qy, int64_t qx, int64_t h,
                                           int64_t w) {
    Tap<G> t;
    const bool inside = qy >= 0 && qy < h && qx >= 0 && qx < w;
    const int64_t cy = qy < 0 ? 0 : (qy >= h ? h - 1 : qy), cx = qx < 0 ? 0 : (qx >= w ? w - 1 : qx);
    const int64_t q = cy * w + cx;
    t.g = load_guide<G>(guide, q);
    t.s = sig[q];
    if (!inside) t.g.n.w = 0.0f;
    return t;
}

// the guide weight of the valid pixel a against the tap t; 0 for an invalid one
template <int G>
__device__ __forceinline__ float guide_weight(const Guide<G>& a, const Tap<G>& t, const Params& P) {
    const Guide<G>& b = t.g;
    float wn = fmaxf((a.n.x * b.n.x + a.n.y * b.n.y) + a.n.z * b.n.z, 0.0f);
    for (int s = 0; s < P.k; ++s) wn = wn * wn;
    const float dx = b.p.x - a.p.x, dy = b.p.y - a.p.y, dz = b.p.z - a.p.z;
    const float plane = (a.n.x * dx + a.n.y * dy) + a.n.z * dz;
    float wt = wn * expf(-(fabsf(plane) / P.sigma_p));
    if (G == 4) {
        const float e0 = a.g.x - b.g.x, e1 = a.g.y - b.g.y, e2 = a.g.z - b.g.z, e3 = a.g.w - b.g.w;
        const float d2 = ((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3;
        wt = wt * expf(-(d2 / P.sg2));
    }
    return b.n.w != 0.0f ? wt : 0.0f;
}

// the pixel (y, x) of tile t that this thread owns; false past the image's edge
__device__ __forceinline__ bool own_pixel(int64_t t, int64_t tx_count, int64_t h, int64_t w, int64_t* y, int64_t* x) {
    const int64_t ty = t / tx_count, tx = t - ty * tx_count;
    *y = ty * TILE_H + (int)(threadIdx.x / TILE_W);
    *x = tx * TILE_W + (int)(threadIdx.x % TILE_W);
    return *y < h && *x < w;
}

// ---- a tile and its halo of R pixels in LDS -----------------------------------------------------------------------------------------------
// RH x RW records (RW = TILE_W + 2 R, RH = TILE_H + 2 R) from the pixel (y0, x0) on, a pixel outside the image as an invalid one
template <int G, int R>
__device__ __forceinline__ void stage_tile(float4* l_n, float4* l_p, float4* l_g, float4* l_s, const float4* __restrict__ guide,
                                           const float4* __restrict__ sig, int64_t y0, int64_t x0, int64_t h, int64_t w) {
    constexpr int RW = TILE_W + 2 * R, RH = TILE_H + 2 * R;
    for (int j = (int)threadIdx.x; j < RH * RW; j += THREADS) {
        const Tap<G> b = load_tap<G>(guide, sig, y0 + j / RW, x0 + j % RW, h, w);
        l_n[j] = b.g.n;
        l_p[j] = b.g.p;
        if (G == 4) l_g[j] = b.g.g;
        l_s[j] = b.s;
    }
}

template <int G>
__device__ __forceinline__ Tap<G> staged_tap(const float4* l_n, const float4* l_p, const float4* l_g, const float4* l_s, int q) {
    Tap<G> t;
    t.g.n = l_n[q];
    t.g.p = l_p[q];
    if (G == 4) t.g.g = l_g[q];
    t.s = l_s[q];
    return t;
}

// ---- the variance pass -----------------------------------------------------------------------------------------------------------------------
// the tile and its halo of VAR_RADIUS pixels staged in LDS; a tile without a valid pixel of its own stages nothing
template <int G>
__global__ __launch_bounds__(THREADS) void denoise_variance_kernel(const float4* __restrict__ guide, const float4* __restrict__ sig_in, int64_t h,
                                                                   int64_t w, int64_t n_tiles, Params P, float4* __restrict__ sig_out) {
    constexpr int R = VAR_RADIUS, RW = TILE_W + 2 * R, RH = TILE_H + 2 * R;
    static_assert(RW * RH == region_records(R), "denoise_plan.h sizes this kernel's LDS");
    __shared__ float4 l_n[RH * RW], l_p[RH * RW], l_s[RH * RW], l_g[G == 4 ? RH * RW : 1];
    const int64_t tx_count = (w + TILE_W - 1) / TILE_W;           // (tiles_x of denoise_plan.h, a host function)
    const int ly = (int)(threadIdx.x / TILE_W), lx = (int)(threadIdx.x % TILE_W);
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int64_t y, x;
        const bool own = own_pixel(t, tx_count, h, w, &y, &x);
        const int64_t i = own ? y * w + x : 0;
        float4 out = sig_in[i];
        const Guide<G> a = load_guide<G>(guide, i);
        const bool work = own && a.n.w != 0.0f;
        if (!__syncthreads_or(work)) {                                // one answer for the workgroup; also the barrier between two tiles' LDS
            if (own) sig_out[i] = out;
            continue;
        }
        stage_tile<G, R>(l_n, l_p, l_g, l_s, guide, sig_in, y - ly - R, x - lx - R, h, w);
        __syncthreads();
        if (work) {
            const int c = (ly + R) * RW + (lx + R);                   // every tap lies within [0, RH RW): |offset| <= R rows and R columns
            const float lum_p = lum_of(out);
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int oy = -R; oy <= R; ++oy)
#pragma unroll
                for (int ox = -R; ox <= R; ++ox) {
                    const Tap<G> tap = staged_tap<G>(l_n, l_p, l_g, l_s, c + oy * RW + ox);
                    const float wt = guide_weight<G>(a, tap, P);
                    if (wt == 0.0f) continue;
                    const float d = lum_of(tap.s) - lum_p;
                    s0 = s0 + wt;
                    s1 = s1 + wt * d;
                    s2 = s2 + wt * (d * d);
                }
            if (s0 > 0.0f) {
                const float m1 = s1 / s0, m2 = s2 / s0;
                out.w = fmaxf(m2 - m1 * m1, 0.0f);
            }
        }
        if (own) sig_out[i] = out;
    }
}

// ---- the a-trous pass: what the direct and the staged kernel share ----------------------------------------------------------------------------
__device__ __constant__ const float C5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
__device__ __constant__ const float C3[3] = {0.25f, 0.5f, 0.25f};

// den = sigma_l sqrtf(gvar) + 1e-6 from the nine (valid, var) pairs around a valid p, row-major (p itself counts: the divisor is >= 1/4)
__device__ __forceinline__ float luminance_scale(const float* valid, const float* var, float sigma_l) {
    float va = 0.0f, vb = 0.0f;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        if (valid[j] == 0.0f) continue;
        const float c = C3[j / 3] * C3[j % 3];
        va = va + c * var[j];
        vb = vb + c;
    }
    return sigma_l * sqrtf(va / vb) + 1e-6f;
}

struct Sums {
    float w = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f, v = 0.0f;
};

template <int G>
__device__ __forceinline__ void add_tap(Sums& S, const Guide<G>& a, const Tap<G>& t, float c, float lum_p, float den, const Params& P) {
    const float gw = guide_weight<G>(a, t, P);
    if (gw == 0.0f) return;                                       // (adding the zeros would change no bit)
    const float wl = expf(-(fabsf(lum_p - lum_of(t.s)) / den));
    const float wt = (c * gw) * wl;
    S.w = S.w + wt;
    S.r = S.r + wt * t.s.x;
    S.g = S.g + wt * t.s.y;
    S.b = S.b + wt * t.s.z;
    S.v = S.v + (wt * wt) * t.s.w;
}

__device__ __forceinline__ void finish(const Sums& S, float4& out) {
    if (S.w > 0.0f) {
        out.x = S.r / S.w;
        out.y = S.g / S.w;
        out.z = S.b / S.w;
        const float w2 = S.w * S.w;
        if (w2 > 0.0f) out.w = S.v / w2;
    }
}

// any stride (used above MAX_STAGED_STEP): the taps straight from memory, one row of five in flight at a time
template <int G>
__global__ __launch_bounds__(THREADS) void denoise_atrous_kernel(const float4* __restrict__ guide, const float4* __restrict__ sig_in, int64_t h,
                                                                 int64_t w, int64_t n_tiles, int step, Params P, float4* __restrict__ sig_out) {
    const int64_t tx_count = (w + TILE_W - 1) / TILE_W;
    constexpr int N = 2 * ATROUS_RADIUS + 1;
    const float* gf = (const float*)guide;
    const float* sf = (const float*)sig_in;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int64_t y, x;
        if (!own_pixel(t, tx_count, h, w, &y, &x)) continue;
        const int64_t i = y * w + x;
        float4 out = sig_in[i];
        const Guide<G> a = load_guide<G>(guide, i);
        if (a.n.w != 0.0f) {
            float valid[9], var[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int64_t qy = y + (j / 3 - 1), qx = x + (j % 3 - 1);
                const bool inside = qy >= 0 && qy < h && qx >= 0 && qx < w;
                const int64_t q = inside ? qy * w + qx : i;
                valid[j] = inside ? gf[q * (G == 4 ? 12 : 8) + 3] : 0.0f;
                var[j] = sf[q * 4 + 3];
            }
            const float den = luminance_scale(valid, var, P.sigma_l), lum_p = lum_of(out);
            Sums S;
            for (int ty = 0; ty < N; ++ty) {
                Tap<G> row[N];
#pragma unroll
                for (int tx = 0; tx < N; ++tx)
                    row[tx] = load_tap<G>(guide, sig_in, y + (int64_t)(ty - ATROUS_RADIUS) * step, x + (int64_t)(tx - ATROUS_RADIUS) * step, h, w);
#pragma unroll
                for (int tx = 0; tx < N; ++tx) add_tap<G>(S, a, row[tx], C5[ty] * C5[tx], lum_p, den, P);
            }
            finish(S, out);
        }
        sig_out[i] = out;
    }
}

// STEP 1 or 2: the tile and its halo of 2 STEP pixels staged in LDS, a pixel outside the image as an invalid one; a tile without a valid
// pixel of its own stages nothing.  The arithmetic is denoise_atrous_kernel's, tap for tap.
template <int G, int STEP>
__global__ __launch_bounds__(THREADS) void denoise_atrous_staged_kernel(const float4* __restrict__ guide, const float4* __restrict__ sig_in,
                                                                        int64_t h, int64_t w, int64_t n_tiles, Params P,
                                                                        float4* __restrict__ sig_out) {
    constexpr int R = ATROUS_RADIUS * STEP, RW = TILE_W + 2 * R, RH = TILE_H + 2 * R, N = 2 * ATROUS_RADIUS + 1;
    static_assert(STEP >= 1 && STEP <= MAX_STAGED_STEP && RW * RH == staged_records(STEP), "denoise_plan.h sizes this kernel's LDS");
    __shared__ float4 l_n[RH * RW], l_p[RH * RW], l_s[RH * RW], l_g[G == 4 ? RH * RW : 1];
    const int64_t tx_count = (w + TILE_W - 1) / TILE_W;
    const int ly = (int)(threadIdx.x / TILE_W), lx = (int)(threadIdx.x % TILE_W);
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int64_t y, x;
        const bool own = own_pixel(t, tx_count, h, w, &y, &x);
        const int64_t i = own ? y * w + x : 0;
        float4 out = sig_in[i];
        const Guide<G> a = load_guide<G>(guide, i);
        const bool work = own && a.n.w != 0.0f;
        if (!__syncthreads_or(work)) {                                // one answer for the workgroup; also the barrier between two tiles' LDS
            if (own) sig_out[i] = out;
            continue;
        }
        stage_tile<G, R>(l_n, l_p, l_g, l_s, guide, sig_in, y - ly - R, x - lx - R, h, w);
        __syncthreads();
        if (work) {
            const int c = (ly + R) * RW + (lx + R);                   // every tap lies within [0, RH RW): |offset| <= R rows and R columns
            float valid[9], var[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const int q = c + (j / 3 - 1) * RW + (j % 3 - 1);
                valid[j] = l_n[q].w;
                var[j] = l_s[q].w;
            }
            const float den = luminance_scale(valid, var, P.sigma_l), lum_p = lum_of(out);
            Sums S;
#pragma unroll
            for (int ty = 0; ty < N; ++ty)
#pragma unroll
                for (int tx = 0; tx < N; ++tx) {
                    const int q = c + (ty - ATROUS_RADIUS) * STEP * RW + (tx - ATROUS_RADIUS) * STEP;
                    add_tap<G>(S, a, staged_tap<G>(l_n, l_p, l_g, l_s, q), C5[ty] * C5[tx], lum_p, den, P);
                }
            finish(S, out);
        }
        if (own) sig_out[i] = out;
    }
}

const char* check_common(const float* guide, int G, const float* sig_in, int64_t h, int64_t w, int k, float sigma_p, float sigma_g,
                         const float* sig_out) {
    if (!guide || !sig_in || !sig_out) return "null pointer";
    if (!shape_ok(h, w)) return "h and w must be at least 1 and h w below 2^31";
    if (!guide_ok(G)) return "G must be 0 or 4";
    if (!k_ok(k)) return "k must be in [0, 10]";
    if (!sigma_ok(sigma_p)) return "sigma_p must be finite and positive";
    if (G == 4 && !sigma_ok(sigma_g)) return "sigma_g must be finite and positive";
    if (sig_in == sig_out) return "sig_in and sig_out must not be the same buffer";
    if ((((uintptr_t)guide | (uintptr_t)sig_in | (uintptr_t)sig_out) & 15u) != 0) return "the records are not 16-byte aligned";
    return nullptr;
}

int refuse(const char* fn, const char* why) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", fn, why);
    return nero_fail(NERO_ERR_ARG, msg);
}

}  // namespace

int64_t nero_denoise_max_pixels(void) { return MAX_PIXELS; }

int nero_denoise_variance(const float* guide, int G, const float* sig_in, int64_t h, int64_t w, int k, float sigma_p, float sigma_g,
                          float* sig_out, void* stream) {
    if (const char* why = check_common(guide, G, sig_in, h, w, k, sigma_p, sigma_g, sig_out)) return refuse("nero_denoise_variance", why);
    const Params P = {k, 1.0f, sigma_p, G == 4 ? sigma_g * sigma_g : 1.0f};
    const float4 *g4 = (const float4*)guide, *s4 = (const float4*)sig_in;
    const dim3 grid(grid_of(h, w)), block(THREADS);
    if (G == 4)
        hipLaunchKernelGGL(denoise_variance_kernel<4>, grid, block, 0, (hipStream_t)stream, g4, s4, h, w, tiles(h, w), P, (float4*)sig_out);
    else
        hipLaunchKernelGGL(denoise_variance_kernel<0>, grid, block, 0, (hipStream_t)stream, g4, s4, h, w, tiles(h, w), P, (float4*)sig_out);
    return nero_check_launch("nero_denoise_variance");
}

int nero_denoise_atrous(const float* guide, int G, const float* sig_in, int64_t h, int64_t w, int step, int k, float sigma_l, float sigma_p,
                        float sigma_g, float* sig_out, void* stream) {
    if (const char* why = check_common(guide, G, sig_in, h, w, k, sigma_p, sigma_g, sig_out)) return refuse("nero_denoise_atrous", why);
    if (!step_ok(step)) return refuse("nero_denoise_atrous", "step must be in [1, 2^20]");
    if (!sigma_ok(sigma_l)) return refuse("nero_denoise_atrous", "sigma_l must be finite and positive");
    const Params P = {k, sigma_l, sigma_p, G == 4 ? sigma_g * sigma_g : 1.0f};
    const float4 *g4 = (const float4*)guide, *s4 = (const float4*)sig_in;
    float4* o4 = (float4*)sig_out;
    const dim3 grid(grid_of(h, w)), block(THREADS);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = tiles(h, w);
    if (staged(step) && G == 4 && step == 1)
        hipLaunchKernelGGL((denoise_atrous_staged_kernel<4, 1>), grid, block, 0, s, g4, s4, h, w, n_tiles, P, o4);
    else if (staged(step) && G == 4)
        hipLaunchKernelGGL((denoise_atrous_staged_kernel<4, 2>), grid, block, 0, s, g4, s4, h, w, n_tiles, P, o4);
    else if (staged(step) && step == 1)
        hipLaunchKernelGGL((denoise_atrous_staged_kernel<0, 1>), grid, block, 0, s, g4, s4, h, w, n_tiles, P, o4);
    else if (staged(step))
        hipLaunchKernelGGL((denoise_atrous_staged_kernel<0, 2>), grid, block, 0, s, g4, s4, h, w, n_tiles, P, o4);
    else if (G == 4)
        hipLaunchKernelGGL(denoise_atrous_kernel<4>, grid, block, 0, s, g4, s4, h, w, n_tiles, step, P, o4);
    else
        hipLaunchKernelGGL(denoise_atrous_kernel<0>, grid, block, 0, s, g4, s4, h, w, n_tiles, step, P, o4);
    return nero_check_launch("nero_denoise_atrous");
}
