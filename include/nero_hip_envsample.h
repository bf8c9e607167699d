/* nero_hip_envsample.h -- C ABI of libnero_hip.so, fifth header: importance sampling of the environment map in the relighter, combined with
 * the two BRDF strategies of nero_hip_relight.h by multiple importance sampling (MIS, balance heuristic).
 *
 * Conventions are those of nero_hip_relight.h: device pointers to fp32 (int64 / int32 / bytes where stated), every call asynchronous on
 * `stream`, 0 on success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or synchronises.
 * Arguments are validated before any device call.  env, eh, ew, convention, rot, clamp_max: exactly as nero_env_lookup takes them.
 *
 * THE GRID.  gh x gw = eh x ew cells, equirectangular in WORLD directions (the direction before `rot`), by convention 2's formulas whatever
 * the map's own convention -- neither the rotation nor a convention is ever inverted.  With PI = (float) pi, TWO_PI = (float) 2 pi, every
 * float32 operation rounded on its own (no contraction), cosf / sinf / atan2f the device's:
 *   direction of (u, v):  el = (v - 0.5f) PI, phi = (u - 0.5f) TWO_PI, ce = cosf(el), d = (-(ce cosf(phi)), ce sinf(phi), sinf(el))
 *   centre of cell (r, c): u = ((float) c + 0.5f) / (float) gw, v = 1.0f - ((float) r + 0.5f) / (float) gh
 *   (u, v) of a direction d: u = atan2f(d.y, -d.x) / TWO_PI + 0.5f, v = atan2f(d.z, sqrtf(d.x d.x + d.y d.y)) / PI + 0.5f
 *   cell of a direction:   row = clamp((int) floorf((1.0f - v) (float) gh), 0, gh - 1), col = clamp((int) floorf(u (float) gw), 0, gw - 1)
 *
 * THE TABLE.  Y(u, v) = (0.2126f R + 0.7152f G) + 0.0722f B with (R, G, B) = the lookup of nero_env_lookup in the direction of (u, v)
 * (rotation, convention and clamp_max honoured).  a[k] (k = r gw + c) = Ymax max(ce, 0), ce of the cell's centre and Ymax the largest finite
 * Y over the nine points u = ((float) c + 0.5f s) / (float) gw, v = 1.0f - ((float) r + 0.5f t) / (float) gh, s, t in {0, 1, 2} (corners,
 * edge midpoints, centre; 0 when none is positive).  The lookup is bilinear, so a bright texel spills into the cells around its own; the
 * largest of the nine keeps L / p_l bounded there, where a weight read at the centre alone leaves nearly half of a lone texel's energy to
 * the chance of the BRDF strategies.  An a that is not finite or is negative counts as 0.  mx = max a, e = the frexp exponent of (double) mx (0 for mx = 0), B = min(40, 62 - bitlength(gh gw - 1)),
 * w[k] = (uint64) floor(ldexp((double) a[k], B - e)), cdf[k] = w[0] + ... + w[k] in int64 (an integer scan: the same bits however it is
 * partitioned), at most 2^62.  The marginal of row r is read from the same array: R_r = cdf[r gw + gw - 1].
 * FALLBACK: mx = 0 (a black or wholly non-finite map): a[k] = max(ce, 0) of the cell's centre, e = 0 -- uniform in solid angle.
 * info [5] int64 (DEVICE) = {cdf[gh gw - 1], the number of cells with w = 0, e, B, 1 if the fallback was taken else 0}.
 *
 * A LIGHT SAMPLE from variates (u1, u2) in [0, 1), in float64 and integers:
 *   total = info[0]; t1 = min((uint64)((double) u1 (double) total), total - 1); row = the first r with R_r > t1 (binary search)
 *   base = R_{row-1} (0 for row 0), rowtot = R_row - base; t2 = base + min((uint64)((double) u2 (double) rowtot), rowtot - 1)
 *   col = the first c with cdf[row gw + c] > t2 (binary search); k = row gw + col, prev = cdf[k - 1] (0 for k = 0), w_cell = cdf[k] - prev
 *   x1 = ((double) u1 (double) total - (double) base) / (double) rowtot, x2 = ((double) u2 (double) rowtot - (double)(prev - base)) /
 *   (double) w_cell, each clamped to [0, 1 - 2^-24] and rounded to float: the position inside the cell, so a stratified lattice stays
 *   stratified.  u = ((float) col + x2) / (float) gw, v = 1.0f - ((float) row + x1) / (float) gh, direction as above.
 * A cell or row of weight 0 is never chosen.
 * DENSITY per steradian of a direction with cell k and elevation el = (v - 0.5f) PI:
 *   p_l = ((float)((double) w_cell / (double) total) ((float) gh (float) gw)) / ((TWO_PI PI) fmaxf(cosf(el), 1e-6f))
 * with the cell and v a light sample was drawn with, or the cell and v of the direction (above) for a sample of another strategy.
 */
#ifndef NERO_HIP_ENVSAMPLE_H
#define NERO_HIP_ENVSAMPLE_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace of nero_env_cdf; 0 (reason in nero_last_error) for sizes the call would refuse or when hipCUB's size query fails */
size_t nero_env_cdf_workspace_bytes(int eh, int ew);

/* The table of the map env [eh,ew,3]: cdf [eh ew] int64, info [5] int64, and optionally weights [eh ew] fp32 = the a[k] the integer weights
 * were made from (the fallback's when it was taken), or NULL.  ws: nero_env_cdf_workspace_bytes(eh, ew) bytes, 256-byte aligned.
 * eh, ew in [1, 16384] and eh ew <= 2^26, else NERO_ERR_ARG (nero_bvh_relight still serves such a map). */
int nero_env_cdf(const float* env, int eh, int ew, int convention, const float* rot /* host [9] or NULL */, float clamp_max, void* ws,
                 int64_t* cdf /* [eh ew] */, int64_t* info /* [5] */, float* weights /* [eh ew] or NULL */, void* stream);

/* The sample set of nero_bvh_relight_mis, made by the same device functions: ray p D + j, D = Dd + Ds + Dl.  j < Dd + Ds: the ray of
 * nero_relight_rays, bit for bit.  Then the light samples from tab_l [Dl,2] in [0,1]: u1 = frac(tab_l[j][0] + rand_l[p][0]), u2 =
 * frac(tab_l[j][1] + rand_l[p][1]) (frac(s) = s - floorf(s), capped at 1 - 2^-24; rand_l [P,2] in [0,1), NULL: no shift), direction as
 * above, origin p + 1e-5 w.  dead [P D] bytes: geometry_type 0: any sample j >= Dd with n.w < -1e-6; geometry_type 1: none.
 * cell [P D] int32 = row gw + col, the drawn cell of a light sample and the looked-up cell of any other; pdf_l [P D] = p_l.
 * cdf, info: as nero_env_cdf left them for a gh x gw map.  Dd, Ds, Dl in [1, 4096]; P * (D rounded up to a multiple of 64) <= 2^31 - 64.
 * dead, cell and pdf_l may each be NULL. */
int nero_relight_mis_rays(const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l /* [P,2] or NULL */,
                          int P, int Dd, int Ds, int Dl, int geometry_type, const int64_t* cdf, const int64_t* info, int gh, int gw,
                          float* rays_o /* [P D,3] */, float* rays_d /* [P D,3] */, unsigned char* dead, int* cell, float* pdf_l, void* stream);

/* bytes of the workspace of nero_bvh_relight_mis: six floats per wavefront of (point, sample) lanes; 0 for arguments the call would refuse */
size_t nero_relight_mis_workspace_bytes(int P, int Dd, int Ds, int Dl);

/* The fused MIS kernel, with the lane layout and the reduction of nero_bvh_relight: one lane per (point, sample), the D = Dd + Ds + Dl
 * samples of a point padded to whole wavefronts, any-hit shadow walk within 10, the map looked up on a free ray only, a shuffle butterfly,
 * one six-float partial per wavefront in `ws`, a finishing kernel in index order; no floating-point atomic, nothing stored per ray.
 * With the saturated NoL, NoH, HoV, NoV, D_ggx = a^2 / (PI t^2 + 1e-4) and G of nero_bvh_relight, every sample -- whichever strategy
 * drew it -- is weighed by the same mixture of the densities the three samplers HAVE (the balance heuristic):
 *   p_d = NoL / PI, p_act = D(c) c with c = sat(w.r), r the reflection (floats 6-8 of the record), D(c) = a^2 / max(PI (c^2 (a^2 - 1) + 1)^2,
 *   1e-30): the GGX strategy lays its lobe around r itself; p_mix = (Dd p_d + Ds p_act + Dl p_l) / D
 *   diffuse_lin = mean over all D samples of albedo (1 - metallic) L (NoL / PI) / p_mix      (0 where p_mix == 0 or NoL == 0)
 *   spec_lin    = mean over all D samples of S(w) F L D_ggx G / (4 NoV p_mix + 1e-5)
 *   rgb_lin     = diffuse_lin + spec_lin
 * S(w) = 1 + p_act / (p_code + 1e-5) with p_code = D_ggx NoH / (4 HoV + 1e-5), the density nero_bvh_relight divides a GGX sample by.  That
 * kernel's specular mean is the SUM of two complete estimates of f = F L D_ggx G / (4 NoV) (each sample divided by its own strategy's
 * density times that strategy's share): the cosine half has the expectation Int f, the GGX half Int f p_act / p_code, because its samples
 * have the density p_act and are divided by p_code.  S(w) f is the integrand whose integral is that sum, so both kernels have the same
 * expectation (the Stage-II materials were fitted under the two-strategy one).  Where p_act = p_code, S = 2.
 * L = the map's radiance where the shadow ray is free and the sample not dead, else 0.  env .. clamp_max as for nero_env_lookup; cdf, info:
 * nero_env_cdf's for the same map, rotation, convention and cap (gh x gw = eh x ew).  ws: at least
 * nero_relight_mis_workspace_bytes(P, Dd, Ds, Dl) bytes, 4-byte aligned.  P == 0 does nothing.  Limits as for nero_relight_mis_rays, and
 * eh ew <= 2^26. */
int nero_bvh_relight_mis(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l,
                         const float* rand_l /* [P,2] or NULL */, int P, int Dd, int Ds, int Dl, int geometry_type, const float* env, int eh,
                         int ew, int convention, const float* rot /* host [9] or NULL */, float clamp_max, const int64_t* cdf,
                         const int64_t* info, float* rgb_lin /* [P,3] */, float* diffuse_lin /* [P,3] or NULL */,
                         float* spec_lin /* [P,3] or NULL */, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
