// image_metrics.hip -- the validation metrics on 8-bit images (include/nero_hip.h, nero_img_*).
//
// Replaces, for images that already live on the device:
//   nero_img_quantize   color_map_backward: rgb * 255, clip to [0, 255], astype(uint8)                    (utils/base_utils.py:453-456)
//   nero_img_metrics    compute_psnr                                                                       (network/metrics.py:11-17)
//                       structural_similarity(gt, pr, win_size=11, channel_axis=2, data_range=255)         (network/metrics.py:50, 85)
// The reference copies every float image to the host, quantises it there and lets skimage filter it in float64.  Here the 8-bit images stay on
// the device and every window sum is an integer: with x, y <= 255 the 121-tap sums of x, y, x^2, y^2, x y are at most 121 * 65025 < 2^23, the
// covariance numerators 121 sxx - sx^2 are below 2^30, so nothing rounds before the per-window ratio S, which is formed in float64.
//
// im_tile_kernel: one workgroup per IM_T x IM_T tile of window positions of one image.  It stages the (IM_T + 10)^2 pixels of both images into
//   LDS with byte loads that are contiguous along a row (rows of w C bytes have no alignment to rely on), de-interleaving the channels; takes the
//   five horizontal 11-tap sums (int32, LDS), then the five vertical ones, both by sliding the window (integers: add the entering sample,
//   subtract the leaving one, still exact); adds S over the tile's windows that exist, in a fixed order (per thread four consecutive rows
//   rising, across the wave by a shuffle tree, across the four waves by rising wave); and writes one float64 partial per channel.
//   The squared differences are added in integers over the pixels the tile OWNS: pixel (y, x) belongs to tile (min(y / IM_T, nty - 1),
//   min(x / IM_T, ntx - 1)), so every pixel is counted once -- the last tile of a row or column takes the 10-pixel rim.
// im_final_kernel: one workgroup per image adds the partials (thread t takes tiles t, t + 256, ... by rising index, then the same tree) and
//   writes sse, ssim_c, psnr and ssim.
// No atomics at all; every partial of the workspace is written before it is read, so what the workspace held before does not matter, and the
// result is bit-identical run to run.  fp32 arithmetic: one multiply per element in the quantiser (no packed VALU code, common.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip.h"
#include "common.h"
#include "ws_plan.h"

namespace {

using nero_ws::align256;

constexpr int IM_WIN = 11;                          // skimage's win_size as the reference passes it
constexpr int IM_HALO = IM_WIN - 1;
constexpr int IM_T = 32;                            // window positions per tile side
constexpr int IM_S = IM_T + IM_HALO;                // pixels per staged tile side
constexpr int IM_LD = 44;                           // LDS row pitch of the staged bytes
constexpr int IM_MIN_SIZE = IM_WIN;
constexpr int IM_MAX_SIZE = 16384;
constexpr int IM_MAX_B = 65535;                     // gridDim.y
constexpr int IM_MAX_C = 4;
constexpr int IM_THREADS = 256;
constexpr int IM_SEG = 8;                           // outputs of a row one thread of the horizontal pass slides over
constexpr int IM_VROWS = IM_T * IM_T / IM_THREADS;  // windows of a column one thread of the vertical pass slides over (4)
static_assert(IM_S * (IM_T / IM_SEG) <= IM_THREADS && IM_T % IM_SEG == 0, "the horizontal pass is one round of the workgroup");
constexpr double IM_C1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double IM_C2 = (0.03 * 255.0) * (0.03 * 255.0);
constexpr double IM_INV_NP2 = 1.0 / (121.0 * 121.0);            // means: sums / 121, products of two means
constexpr double IM_INV_COV = 1.0 / (121.0 * 120.0);            // sample covariance: (121 sxy - sx sy) / (121 * 120)

__host__ __device__ inline int tiles_of(int n) { return (n - IM_HALO + IM_T - 1) / IM_T; }      // n >= 11: at least one

// sum over the workgroup in a fixed order; the total is valid in thread 0.  `red`: one slot per wave
template <typename V>
__device__ __forceinline__ V block_sum(V v, V* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();                                // the previous use of `red` has been read
    if (lane == 0) red[wave] = v;
    __syncthreads();
    V total = red[0];
#pragma unroll
    for (int k = 1; k < IM_THREADS / 64; ++k) total += red[k];
    return total;
}

__device__ __forceinline__ unsigned char quantize_one(float x) {
    asm volatile("" : "+v"(x));                     // a value of its own: two elements of a float4 load are never multiplied as a packed pair
    const float v = nero_mul_rn(x, 255.0f);
    if (!(v > 0.0f)) return 0;                      // negatives, -0, -inf and NaN
    if (v >= 255.0f) return 255;
    return (unsigned char)(int)v;                   // truncation towards zero
}

// S of one window from its five integer sums (include/nero_hip.h): integers up to the four terms, float64 from there
__device__ __forceinline__ double ssim_window(int sx, int sy, int sxx, int syy, int sxy) {
    const int64_t mxy = (int64_t)sx * sy;
    const int64_t mxx = (int64_t)sx * sx, myy = (int64_t)sy * sy;
    const int64_t cxy = 121 * (int64_t)sxy - mxy;
    const int64_t cxx = 121 * (int64_t)sxx - mxx, cyy = 121 * (int64_t)syy - myy;
    const double a1 = (double)(2 * mxy) * IM_INV_NP2 + IM_C1;
    const double a2 = (double)(2 * cxy) * IM_INV_COV + IM_C2;
    const double b1 = (double)(mxx + myy) * IM_INV_NP2 + IM_C1;
    const double b2 = (double)(cxx + cyy) * IM_INV_COV + IM_C2;
    return (a1 * a2) / (b1 * b2);
}

// four elements per thread: one 16-byte load, one 4-byte store; the last n % 4 elements one by one
__global__ __launch_bounds__(IM_THREADS) void im_quantize4_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * IM_THREADS + threadIdx.x) * 4;
    if (i + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(in + i);
        const unsigned q = (unsigned)quantize_one(v.x) | ((unsigned)quantize_one(v.y) << 8) | ((unsigned)quantize_one(v.z) << 16) |
                           ((unsigned)quantize_one(v.w) << 24);
        *reinterpret_cast<unsigned*>(out + i) = q;
    } else {
        for (int64_t k = i; k < n; ++k) out[k] = quantize_one(in[k]);
    }
}

__global__ __launch_bounds__(IM_THREADS) void im_quantize1_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * IM_THREADS + threadIdx.x;
    if (i < n) out[i] = quantize_one(in[i]);
}

template <int C>
__global__ __launch_bounds__(IM_THREADS) void im_tile_kernel(const unsigned char* __restrict__ gt, const unsigned char* __restrict__ pr, int h, int w,
                                                             int ntx, int nty, double* __restrict__ ws_ssim,
                                                             unsigned long long* __restrict__ ws_sse) {
    __shared__ unsigned char sg[C][IM_S][IM_LD], sp[C][IM_S][IM_LD];
    __shared__ int hs[5][IM_S][IM_T + 1];           // (+ 1: the horizontal pass writes IM_SEG words apart)
    __shared__ double red_d[IM_THREADS / 64];
    __shared__ unsigned long long red_u[IM_THREADS / 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int ntiles = ntx * nty;
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * IM_T, x0 = tx * IM_T;
    const bool last_y = ty == nty - 1, last_x = tx == ntx - 1;
    const size_t img = (size_t)b * h * w * C;

    // stage both images, channels de-interleaved; pixels outside the image read as zero (only windows that do not exist touch them)
    unsigned long long sse = 0;
    constexpr int ROW = IM_S * C;
    for (int i = tid; i < IM_S * ROW; i += IM_THREADS) {
        const int ly = i / ROW, j = i - ly * ROW;
        const int lx = j / C, c = j - lx * C;
        const int gy = y0 + ly, gx = x0 + lx;
        int a = 0, p = 0;
        if (gy < h && gx < w) {
            const size_t at = img + ((size_t)gy * w + gx) * C + c;
            a = gt[at];
            p = pr[at];
            if ((ly < IM_T || last_y) && (lx < IM_T || last_x)) {       // this tile owns the pixel
                const int d = a - p;
                sse += (unsigned)(d * d);
            }
        }
        sg[c][ly][lx] = (unsigned char)a;
        sp[c][ly][lx] = (unsigned char)p;
    }
    sse = block_sum(sse, red_u);                    // (its barriers also publish the staged bytes)
    if (tid == 0) ws_sse[(size_t)b * ntiles + tile] = sse;

    const int vx = tid & (IM_T - 1), vy = (tid >> 5) * IM_VROWS;       // vertical pass: column vx, rows vy ... vy + IM_VROWS - 1
    for (int c = 0; c < C; ++c) {
        __syncthreads();                            // the vertical pass of the previous channel has read hs
        // horizontal 11-tap sums: a thread takes IM_SEG consecutive outputs of one row, the first in full, the others by sliding
        if (tid < IM_S * (IM_T / IM_SEG)) {
            const int r = tid / (IM_T / IM_SEG), xs = (tid % (IM_T / IM_SEG)) * IM_SEG;
            const unsigned char* ga = &sg[c][r][xs];
            const unsigned char* pa = &sp[c][r][xs];
            int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int k = 0; k < IM_WIN; ++k) {
                const int a = ga[k], p = pa[k];
                sx += a;
                sy += p;
                sxx += a * a;
                syy += p * p;
                sxy += a * p;
            }
#pragma unroll
            for (int j = 0; j < IM_SEG; ++j) {
                hs[0][r][xs + j] = sx;
                hs[1][r][xs + j] = sy;
                hs[2][r][xs + j] = sxx;
                hs[3][r][xs + j] = syy;
                hs[4][r][xs + j] = sxy;
                if (j + 1 < IM_SEG) {
                    const int a0 = ga[j], p0 = pa[j], a1 = ga[j + IM_WIN], p1 = pa[j + IM_WIN];
                    // the leaving products as values of their own: written as `a1 * p1 - a0 * p0` on bytes, hipcc (ROCm 7.2) matched the
                    // difference into v_dot4_u32_u8, which ADDS both products -- seen on the GPU as sxy growing along a segment
                    int laa = a0 * a0, lpp = p0 * p0, lap = a0 * p0;
                    asm volatile("" : "+v"(laa), "+v"(lpp), "+v"(lap));
                    sx += a1 - a0;
                    sy += p1 - p0;
                    sxx += a1 * a1 - laa;
                    syy += p1 * p1 - lpp;
                    sxy += a1 * p1 - lap;
                }
            }
        }
        __syncthreads();
        // vertical sums of IM_VROWS consecutive windows of one column, sliding the same way; S where the window lies wholly inside the image
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int j = 0; j < IM_WIN; ++j) {
            sx += hs[0][vy + j][vx];
            sy += hs[1][vy + j][vx];
            sxx += hs[2][vy + j][vx];
            syy += hs[3][vy + j][vx];
            sxy += hs[4][vy + j][vx];
        }
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < IM_VROWS; ++k) {
            const int y = vy + k;
            if (y0 + y < h - IM_HALO && x0 + vx < w - IM_HALO) acc += ssim_window(sx, sy, sxx, syy, sxy);
            if (k + 1 < IM_VROWS) {
                sx += hs[0][y + IM_WIN][vx] - hs[0][y][vx];
                sy += hs[1][y + IM_WIN][vx] - hs[1][y][vx];
                sxx += hs[2][y + IM_WIN][vx] - hs[2][y][vx];
                syy += hs[3][y + IM_WIN][vx] - hs[3][y][vx];
                sxy += hs[4][y + IM_WIN][vx] - hs[4][y][vx];
            }
        }
        acc = block_sum(acc, red_d);
        if (tid == 0) ws_ssim[((size_t)b * IM_MAX_C + c) * ntiles + tile] = acc;
    }
}

__global__ __launch_bounds__(IM_THREADS) void im_final_kernel(const double* __restrict__ ws_ssim, const unsigned long long* __restrict__ ws_sse,
                                                              int h, int w, int C, int ntiles, unsigned long long* __restrict__ sse_out,
                                                              double* __restrict__ ssim_c, double* __restrict__ out) {
    __shared__ double red_d[IM_THREADS / 64];
    __shared__ unsigned long long red_u[IM_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    unsigned long long s = 0;
    for (int t = tid; t < ntiles; t += IM_THREADS) s += ws_sse[(size_t)b * ntiles + t];
    s = block_sum(s, red_u);
    const double windows = (double)(h - IM_HALO) * (double)(w - IM_HALO);
    double mean = 0.0;
    for (int c = 0; c < C; ++c) {
        double v = 0.0;
        const double* part = ws_ssim + ((size_t)b * IM_MAX_C + c) * ntiles;
        for (int t = tid; t < ntiles; t += IM_THREADS) v += part[t];
        v = block_sum(v, red_d);
        if (tid == 0) {
            v = v / windows;
            if (ssim_c) ssim_c[(size_t)b * C + c] = v;
            mean += v;
        }
    }
    if (tid == 0) {
        if (sse_out) sse_out[b] = s;
        const double mse = (double)s / ((double)h * (double)w * (double)C);
        out[2 * (size_t)b] = s == 0 ? (double)INFINITY : 10.0 * log10(65025.0 / mse);
        out[2 * (size_t)b + 1] = mean / (double)C;
    }
}

bool shape_ok(int64_t B, int h, int w, int C) {
    return B >= 1 && B <= IM_MAX_B && h >= IM_MIN_SIZE && h <= IM_MAX_SIZE && w >= IM_MIN_SIZE && w <= IM_MAX_SIZE && C >= 1 && C <= IM_MAX_C;
}

}  // namespace

extern "C" {

int nero_img_quantize(const float* in, int64_t n, unsigned char* out, void* stream) {
    if (n < 0) return nero_fail(NERO_ERR_ARG, "nero_img_quantize: n is negative");
    if (n == 0) return NERO_OK;
    if (!in || !out) return nero_fail(NERO_ERR_ARG, "nero_img_quantize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const bool wide = ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 4 == 0);
    const int64_t items = wide ? (n + 3) / 4 : n;
    const int64_t blocks = (items + IM_THREADS - 1) / IM_THREADS;
    if (blocks > 0x7fffffff) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_img_quantize: more than 2^31 - 1 workgroups");
    if (wide)
        hipLaunchKernelGGL(im_quantize4_kernel, dim3((unsigned)blocks), dim3(IM_THREADS), 0, s, in, out, n);
    else
        hipLaunchKernelGGL(im_quantize1_kernel, dim3((unsigned)blocks), dim3(IM_THREADS), 0, s, in, out, n);
    return nero_check_launch("nero_img_quantize");
}

size_t nero_img_metrics_workspace_bytes(int64_t B, int h, int w, int C) {
    if (!shape_ok(B, h, w, C)) return 0;
    const size_t ntiles = (size_t)tiles_of(h) * tiles_of(w);
    return align256((size_t)B * ntiles * (IM_MAX_C + 1) * 8);
}

int nero_img_metrics(const unsigned char* gt, const unsigned char* pr, int64_t B, int h, int w, int C, void* ws, unsigned long long* sse,
                     double* ssim_c, double* out, void* stream) {
    if (!shape_ok(B, h, w, C)) {
        static thread_local char msg[200];
        snprintf(msg, sizeof(msg), "nero_img_metrics: B %lld outside [1, %d], h %d or w %d outside [%d, %d] (an 11 x 11 window must fit), or C %d "
                 "outside [1, %d]", (long long)B, IM_MAX_B, h, w, IM_MIN_SIZE, IM_MAX_SIZE, C, IM_MAX_C);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (!gt || !pr || !ws || !out) return nero_fail(NERO_ERR_ARG, "nero_img_metrics: null pointer");
    if ((uintptr_t)ws % 8 != 0) return nero_fail(NERO_ERR_ARG, "nero_img_metrics: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nty = tiles_of(h), ntx = tiles_of(w), ntiles = ntx * nty;
    double* ws_ssim = (double*)ws;                                                      // [B][IM_MAX_C][ntiles]
    unsigned long long* ws_sse = (unsigned long long*)(ws_ssim + (size_t)B * IM_MAX_C * ntiles);      // [B][ntiles]
    const dim3 grid((unsigned)ntiles, (unsigned)B), block(IM_THREADS);
    switch (C) {
        case 1: hipLaunchKernelGGL(im_tile_kernel<1>, grid, block, 0, s, gt, pr, h, w, ntx, nty, ws_ssim, ws_sse); break;
        case 2: hipLaunchKernelGGL(im_tile_kernel<2>, grid, block, 0, s, gt, pr, h, w, ntx, nty, ws_ssim, ws_sse); break;
        case 3: hipLaunchKernelGGL(im_tile_kernel<3>, grid, block, 0, s, gt, pr, h, w, ntx, nty, ws_ssim, ws_sse); break;
        default: hipLaunchKernelGGL(im_tile_kernel<4>, grid, block, 0, s, gt, pr, h, w, ntx, nty, ws_ssim, ws_sse); break;
    }
    if (int rc = nero_check_launch("nero_img_metrics (tiles)")) return rc;
    hipLaunchKernelGGL(im_final_kernel, dim3((unsigned)B), block, 0, s, ws_ssim, ws_sse, h, w, C, ntiles, sse, ssim_c, out);
    return nero_check_launch("nero_img_metrics (final)");
}

}  // extern "C"
