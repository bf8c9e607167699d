/* nero_hip_denoise.h -- C ABI of libnero_hip.so, eighth header: an edge-aware denoiser for the relighter's pictures.
 *
 * A single-frame edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) steered by a per-pixel variance estimated from the picture
 * itself, as the spatial fallback of SVGF does (Schied et al. 2017); nothing temporal.  It works on an h x w image of pixels at the
 * resolution that was traced, where every pixel is one surface or none (nero_amd/denoise.py, Relighter.render(denoise=...); DESIGN.md
 * 9.12.3).
 *
 * Conventions are those of nero_hip.h: device pointers, every call asynchronous on `stream` (a hipStream_t passed as void*), 0 on success or
 * a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or synchronises.  Arguments are validated before
 * any device call.
 *
 * RECORDS, row-major over the image (pixel y w + x), 16-byte aligned:
 *   guide  [h w, 8 + G] fp32 = (nx, ny, nz, valid, px, py, pz, 0) and, for G = 4, four more guide channels (g0..g3).  valid is 1.0 or 0.0
 *          (anything but 0.0 counts as valid).  G is 0 or 4.
 *   signal [h w, 4] fp32 = (r, g, b, var).
 *
 * GUIDE WEIGHT of a pixel p against q: zero unless both are valid and q lies inside the image (a tap outside is dropped: no clamp, no
 * wrap).  Otherwise (w_n w_p) w_g with
 *   w_n = max(0, (nx nx' + ny ny') + nz nz')^(2^k), by k successive squarings (k in [0, 10]): perpendicular normals give exactly 0;
 *   w_p = expf(-(|(nx dx + ny dy) + nz dz| / sigma_p)), d = P_q - P_p: the distance of q from p's tangent plane;
 *   w_g = expf(-((((e0 e0 + e1 e1) + e2 e2) + e3 e3) / (sigma_g sigma_g))), e = g_p - g_q; absent (1) for G = 0.
 * lum = (0.2126 r + 0.7152 g) + 0.0722 b.
 *
 * ARITHMETIC: one thread owns one output pixel and sums its taps in row-major order; no atomics, no fast intrinsics (expf, sqrtf and IEEE
 * divisions), no contraction into fused multiply-adds: every operation is the fp32 operation a numpy restatement performs
 * (tests/denoise_ref.py), expf's last place excepted.  The same inputs give the same bits on every run.
 */
#ifndef NERO_HIP_DENOISE_H
#define NERO_HIP_DENOISE_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest h w the two entry points take (2^31 - 1); host only */
int64_t nero_denoise_max_pixels(void);

/* The variance pass.  For each valid p, over the 7 x 7 window around it and with W = the guide weight of p against q and d = lum_q - lum_p:
 * s0 = sum W, s1 = sum W d, s2 = sum W (d d); m1 = s1 / s0, m2 = s2 / s0; var_p = max(0, m2 - m1 m1): the guide-weighted variance of the
 * luminance, with the moments taken about lum_p (a variance does not depend on where its moments are taken, and a constant signal gives
 * exactly 0 this way).  sig_out = (r, g, b, var_p): rgb is copied through.  An invalid p, or one with s0 = 0, is copied through whole.
 * sig_in and sig_out must not be the same buffer.  Refused (NERO_ERR_ARG): h or w < 1, h w >= 2^31, k outside [0, 10], G not 0 or 4, a
 * sigma_p (and, for G = 4, a sigma_g) that is not finite and positive, a null pointer, a pointer that is not 16-byte aligned, sig_in == sig_out. */
int nero_denoise_variance(const float* guide, int G, const float* sig_in, int64_t h, int64_t w, int k, float sigma_p, float sigma_g,
                          float* sig_out, void* stream);

/* One a-trous iteration (step = 1, 2, 4, ... over the iterations).  For each valid p:
 *   gvar = the valid-weighted 3 x 3 Gaussian ((1/4, 1/2, 1/4) outer product) of var at stride 1: sum c valid_q var_q / sum c valid_q over
 *          the neighbours inside the image; den = sigma_l sqrtf(gvar) + 1e-6;
 *   over the 25 taps at offsets (-2..2) step in y and x, c = (1/16, 1/4, 3/8, 1/4, 1/16) outer product:
 *          wt = (c W) expf(-(|lum_p - lum_q| / den)), W the guide weight;
 *   rgb' = sum wt rgb_q / sum wt,  var' = sum (wt wt) var_q / (sum wt)^2.
 * The centre tap is one of the 25: its guide and luminance terms are 1 by arithmetic.  An invalid p, or one with sum wt = 0, is copied
 * through unchanged (and var alone where (sum wt)^2 underflows to 0).  sig_in and sig_out must not be the same buffer: the caller
 * ping-pongs two.  Refused (NERO_ERR_ARG): what nero_denoise_variance refuses, a step < 1 or > 2^20, a sigma_l that is not finite and
 * positive. */
int nero_denoise_atrous(const float* guide, int G, const float* sig_in, int64_t h, int64_t w, int step, int k, float sigma_l, float sigma_p,
                        float sigma_g, float* sig_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
