// envlight.hip -- the learned environment light as a lat-long (equirectangular) panorama (include/nero_hip.h, nero_env_*).
//
// Replaces the device arithmetic of the reference's MCShadingNetwork.env_light / get_env_light (network/field.py:1020-1059):
//   nero_env_encode       the linspace / meshgrid / cos / sin direction grid (:1021-1034) and sph_enc(pts, 0) of predict_outer_lights_pts
//                         (:1049-1055), for a window of pixels, straight into the row layout the chain engine reads
//   nero_env_encode_dirs  the same encoding of given directions (get_env_light's light_pts, :1058-1059)
//   nero_env_finish       the ExpActivation of the outer_light predictor (exp(min(x, exp_max))) and linear_to_srgb (:1043-1044)
//   nero_env_rgbe         Radiance RGBE bytes of a linear image (the reference has no HDR writer; relight.py reads such files)
// The four-layer predictor itself runs on the MLP-chain engine between nero_env_encode and nero_env_finish (nero_amd/envlight.py).
// A pixel's direction is a function of its index alone, so any chunking of the panorama gives the same bits.  The angles are formed in
// float64 in units of pi and go through sincospi, so the grid's exact points are exact: the first and the last column coincide, the poles
// have cos(el) = 0, and a direction on the z axis gets the finite limit of the IDE (ide.h: (x + iy)^0 = 1), where the reference's complex
// power returns NaN.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/nero_hip.h"
#include "common.h"
#include "ide.h"                                     // IDE_N, ide_forward and the table check, rows_put / rows_flush (rows.h)
#include "shade_math.h"                              // exp_head, srgb_f

namespace {

using namespace nero_shade;

constexpr int ENV_MAX_SIZE = 16384;

// pixel p = row r, column c of an h x w panorama: az = linspace(1, 0, w)[c] 2 pi - pi / 2, el = linspace(1, -1, h)[r] pi / 2
// (a one-element linspace is its start value)
__device__ __forceinline__ void env_direction(int64_t p, int h, int w, int is_real, float* d) {
    const int r = (int)(p / w), c = (int)(p - (int64_t)r * w);
    const double t = w > 1 ? (double)(w - 1 - c) / (double)(w - 1) : 1.0;
    const double s = h > 1 ? (double)(h - 1 - 2 * r) / (double)(h - 1) : 1.0;
    double sa, ca, se, ce;
    sincospi(2.0 * t - 0.5, &sa, &ca);
    sincospi(0.5 * s, &se, &ce);
    if (is_real) { d[0] = (float)(ce * ca); d[1] = (float)(ce * sa); d[2] = (float)se; }
    else         { d[0] = (float)(ce * sa); d[1] = (float)se;        d[2] = (float)(ce * ca); }
}

// One thread per row, ROW_BLOCK rows per workgroup; the rows leave through LDS so that a wave writes whole rows coalesced
// (mc_encode_miss_kernel's store pattern).  src == NULL: row k is pixel first + k of the panorama; else its direction is src[k].
// X [n_pad, 72 (sphere: 144)]: IDE(d, roughness), with sphere the same 72 columns again; rows n .. n_pad - 1 are zero rows.
__global__ __launch_bounds__(ROW_BLOCK) void env_encode_kernel(const float* __restrict__ src, int h, int w, int64_t first, int n, int n_pad,
                                                                int is_real, int sphere, float roughness, float* __restrict__ X,
                                                                float* __restrict__ dirs) {
    __shared__ float stage[ROW_BLOCK * 73];
    const int row0 = blockIdx.x * ROW_BLOCK;
    const int k = row0 + threadIdx.x;
    const bool live = k < n;
    float d[3];
    if (src) {
        const float* q = src + (size_t)(live ? k : 0) * 3;
        d[0] = q[0]; d[1] = q[1]; d[2] = q[2];
    } else {
        env_direction(first + (live ? k : 0), h, w, is_real, d);
    }
    if (dirs && live) { dirs[(size_t)k * 3] = d[0]; dirs[(size_t)k * 3 + 1] = d[1]; dirs[(size_t)k * 3 + 2] = d[2]; }
    if (!X) return;                                   // (uniform over the grid)
    float e[72];
    ide_forward<true>(d[0], d[1], d[2], roughness, e);        // roughness 0: every attenuation is expf(-0) = 1
    rows_put<72, 0, 72>(stage, e, live ? 1.f : 0.f);
    const int ld = sphere ? 144 : 72;
    rows_flush<72>(stage, X, ld, 0, row0, n_pad);
    if (sphere) rows_flush<72>(stage, X, ld, 72, row0, n_pad);
}

// raw [rows, 4] (the head of the chain: 3 of 4 columns) -> rgb [n, 3]
__global__ __launch_bounds__(256) void env_finish_kernel(const float* __restrict__ raw, int64_t n3, float exp_max, int gamma,
                                                         float* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n3) return;
    const int64_t r = i / 3;
    const int c = (int)(i - r * 3);
    const float v = exp_head(raw[r * 4 + c], exp_max);
    rgb[i] = gamma ? srgb_f(v) : v;
}

// Radiance RGBE: v = max(r, g, b) = m 2^e, m in [0.5, 1); byte = trunc(c 2^(8 - e)), fourth byte e + 128.  The scale is a power of two, so
// every product is exact.  Negative (and NaN) channels count as 0; v < 1e-32 gives (0, 0, 0, 0); v >= 2^127 saturates at e = 127.
__global__ __launch_bounds__(256) void env_rgbe_kernel(const float* __restrict__ rgb, int64_t n, unsigned char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float ch[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float x = rgb[i * 3 + c];
        ch[c] = x > 0.f ? x : 0.f;
    }
    const float v = fmaxf(ch[0], fmaxf(ch[1], ch[2]));
    uchar4 o = make_uchar4(0, 0, 0, 0);
    if (v >= 1e-32f) {
        int e;
        (void)frexpf(v, &e);
        if (!(v < INFINITY) || e > 127) e = 127;
        const float scale = ldexpf(1.f, 8 - e);
        o.x = (unsigned char)(int)fminf(nero_mul_rn(ch[0], scale), 255.f);
        o.y = (unsigned char)(int)fminf(nero_mul_rn(ch[1], scale), 255.f);
        o.z = (unsigned char)(int)fminf(nero_mul_rn(ch[2], scale), 255.f);
        o.w = (unsigned char)(e + 128);
    }
    reinterpret_cast<uchar4*>(out)[i] = o;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

int launch_encode(const char* fn, const float* src, int h, int w, int64_t first, int n, int is_real, int sphere, float roughness, float* X,
                  float* dirs, void* stream) {
    if (n == 0) return NERO_OK;
    if (X) NERO_CHECK_IDE();
    const int n_pad = NERO_ROW_PAD(n);
    hipLaunchKernelGGL(env_encode_kernel, dim3((unsigned)(n_pad / ROW_BLOCK)), dim3(ROW_BLOCK), 0, (hipStream_t)stream, src, h, w, first, n, n_pad,
                       is_real, sphere, roughness, X, dirs);
    return nero_check_launch(fn);
}

}  // namespace

int nero_env_encode(int h, int w, int64_t first, int n, int is_real, int sphere, float roughness, float* X, float* dirs, void* stream) {
    if (h < 1 || h > ENV_MAX_SIZE || w < 1 || w > ENV_MAX_SIZE) return nero_fail(NERO_ERR_ARG, "nero_env_encode: h and w must be in [1, 16384]");
    if (first < 0 || n < 0 || first + (int64_t)n > (int64_t)h * w || n > INT32_MAX - 64)
        return nero_fail(NERO_ERR_ARG, "nero_env_encode: the window [first, first + n) leaves the panorama");
    if (!(roughness >= 0.f)) return nero_fail(NERO_ERR_ARG, "nero_env_encode: roughness must be >= 0");
    if (n > 0 && !X && !dirs) return nero_fail(NERO_ERR_ARG, "nero_env_encode: null pointer");
    return launch_encode("nero_env_encode", nullptr, h, w, first, n, is_real != 0, sphere != 0, roughness, X, dirs, stream);
}

int nero_env_encode_dirs(const float* src, int n, int sphere, float roughness, float* X, void* stream) {
    if (n < 0 || n > INT32_MAX - 64) return nero_fail(NERO_ERR_ARG, "nero_env_encode_dirs: n out of range");
    if (!(roughness >= 0.f)) return nero_fail(NERO_ERR_ARG, "nero_env_encode_dirs: roughness must be >= 0");
    if (n > 0 && (!src || !X)) return nero_fail(NERO_ERR_ARG, "nero_env_encode_dirs: null pointer");
    return launch_encode("nero_env_encode_dirs", src, 1, 1, 0, n, 0, sphere != 0, roughness, X, nullptr, stream);
}

int nero_env_finish(const float* raw, int64_t n, float exp_max, int gamma, float* rgb, void* stream) {
    if (n < 0 || n > ((int64_t)1 << 30)) return nero_fail(NERO_ERR_ARG, "nero_env_finish: n out of range");
    if (n == 0) return NERO_OK;
    if (!raw || !rgb) return nero_fail(NERO_ERR_ARG, "nero_env_finish: null pointer");
    hipLaunchKernelGGL(env_finish_kernel, dim3(blocks_of(3 * n)), dim3(256), 0, (hipStream_t)stream, raw, 3 * n, exp_max, gamma != 0, rgb);
    return nero_check_launch("nero_env_finish");
}

int nero_env_rgbe(const float* rgb, int64_t n, unsigned char* out, void* stream) {
    if (n < 0 || n > ((int64_t)1 << 30)) return nero_fail(NERO_ERR_ARG, "nero_env_rgbe: n out of range");
    if (n == 0) return NERO_OK;
    if (!rgb || !out) return nero_fail(NERO_ERR_ARG, "nero_env_rgbe: null pointer");
    hipLaunchKernelGGL(env_rgbe_kernel, dim3(blocks_of(n)), dim3(256), 0, (hipStream_t)stream, rgb, n, out);
    return nero_check_launch("nero_env_rgbe");
}
