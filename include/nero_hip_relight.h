/* nero_hip_relight.h -- C ABI of libnero_hip.so, third header: relighting a mesh under a lat-long environment map.
 *
 * Direct lighting with shadows: the reference's shade_mixed estimator (GGX distribution, Schlick-GGX or height-correlated Smith geometry
 * term, Schlick Fresnel, cosine-weighted + GGX importance sampling) in which the light a direction fetches is "the environment's radiance
 * if the shadow ray is free, zero if it is blocked".  No inter-reflection here: a blocked direction contributes nothing (nero_hip_bounce.h
 * has the siblings of nero_bvh_relight that give it one bounce).
 *
 * Conventions are those of nero_hip.h and nero_hip_visibility.h: device pointers to fp32 (int32 / bytes where stated), rays and points as
 * [n,3] rows, every call asynchronous on `stream` (a hipStream_t passed as void*), 0 on success or a negative NERO_ERR_* code with a message
 * in nero_last_error().  Nothing here allocates or synchronises, except nero_bvh_export_faces.  Arguments are validated before any device
 * call.  The point record pt [P,32] is the one nero_mc_point_setup writes (floats 27 / 28: the point's azimuth rotations in radians, or
 * -1 for none); its roughness (float 10) is alpha = (perceptual roughness)^2.
 */
#ifndef NERO_HIP_RELIGHT_H
#define NERO_HIP_RELIGHT_H
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* faces_host [n_tris] int32 (HOST): entry k is the caller's face index of record k of nero_bvh_export's triangle array (the builders' leaf
 * order).  Synchronises the device, as nero_bvh_export does. */
int nero_bvh_export_faces(void* handle, int* faces_host);

/* Closest hit with the face.  depth[i]: the bits nero_bvh_trace reports (10 on a miss).  face[i]: the caller's index of the hit triangle,
 * -1 on a miss.  bary[i] = (u, v) of the tracer's own triangle test on the accepted triangle (0, 0 on a miss): the hit point is
 * (1 - u - v) V[F[face,0]] + u V[F[face,1]] + v V[F[face,2]], with u, v >= 0 and u + v <= 1.  The traversal kernel follows
 * nero_bvh_set_traversal as nero_bvh_trace does; both give the same bits.  n == 0 does nothing; n <= (2^31 - 1) / 3. */
int nero_bvh_trace_faces(void* handle, const float* rays_o, const float* rays_d, int n, float* depth /* [n] */, int* face /* [n] */,
                         float* bary /* [n,2] */, void* stream);

/* Bilinear radiance of an h x w lat-long map env [h,w,3] in the directions dirs [n,3] (any non-zero length).  rot: 9 HOST floats, row-major,
 * the direction is rotated first (d' = R d), or NULL.  convention:
 *   0, 1  this project's own grid (nero_env_encode, is_real = 0 / 1): column c at azimuth linspace(1, 0, w)[c] 2 pi - pi / 2, row r at
 *         elevation linspace(1, -1, h)[r] pi / 2, end points included -- the first and the last column are the same direction, the first
 *         and the last row are the poles.  is_real = 1: d = (cos el cos az, cos el sin az, sin el); 0: d = (cos el sin az, sin el, cos el cos az).
 *         The azimuth wraps, the elevation is clamped.
 *   2     equirectangular with pixel-centre sampling: u = atan2(d.y, -d.x) / 2 pi + 0.5, v = atan2(d.z, hypot(d.x, d.y)) / pi + 0.5,
 *         texel coordinates (u w - 0.5, (1 - v) h - 0.5), row 0 at the top; columns wrap, rows are clamped.
 * clamp_max > 0 caps each channel of the interpolated radiance; <= 0: no cap.  Non-finite texels are the caller's problem: they spread to
 * every lookup that touches them (also with weight 0).  A non-finite direction reads texels inside the map and returns some finite mix.
 * h, w in [1, 16384]; 0 <= n <= 2^31 - 1. */
int nero_env_lookup(const float* env, int h, int w, int convention, const float* rot /* host [9] or NULL */, const float* dirs, int64_t n,
                    float clamp_max, float* rgb /* [n,3] */, void* stream);

/* The sample set of nero_bvh_relight, made by the same device function: ray p D + j (D = Dd + Ds; j < Dd cosine-weighted around the normal
 * from tab_d [Dd,2], then GGX-sampled around the reflection from tab_s [Ds,2]; the tables hold (azimuth, elevation) in [0, 1]) with
 * direction w as nero_mc_dirs forms it, origin p + 1e-5 w, and dead [P D] bytes by the rule of nero_mc_dead_rays (geometry_type 0: a
 * GGX-sampled direction with n.w < -1e-6; geometry_type 1: none).  Every product and sum is rounded on its own.  Dd, Ds in [1, 4096];
 * P * (D rounded up to a multiple of 64) <= 2^31 - 64, else NERO_ERR_ARG (call in chunks).  dead may be NULL. */
int nero_relight_rays(const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                      float* rays_o /* [P D,3] */, float* rays_d /* [P D,3] */, unsigned char* dead /* [P D] or NULL */, void* stream);

/* bytes of the workspace of nero_bvh_relight: six floats per wavefront of (point, sample) lanes; 0 for arguments the call would refuse */
size_t nero_relight_workspace_bytes(int P, int Dd, int Ds);

/* The fused relighting kernel: one lane per (point, sample), sample index fastest, each point's D samples padded to whole wavefronts.  A
 * lane forms its direction, tests it for dead, walks its shadow ray (any hit within 10, as nero_bvh_occluded), fetches the environment's
 * radiance when the ray is free (as nero_env_lookup) and weighs it as shade_mixed does; no ray, flag or radiance is stored.
 *   diffuse_lin = mean over the Dd diffuse samples of albedo (1 - metallic) L
 *   spec_lin    = mean over all D samples of F L D_ggx G / (4 NoV p + 1e-5)
 *   rgb_lin     = diffuse_lin + spec_lin
 * The sums are taken in a fixed order -- a butterfly inside the wavefront, one partial per wavefront in `ws`, a second kernel that adds a
 * point's partials in index order -- and no floating-point atomic is used: the same bits on every run, for every way of chunking the
 * points.  geometry_type 0: Schlick-GGX, 1: height-correlated Smith.  env, eh, ew, convention, rot, clamp_max as for nero_env_lookup.
 * diffuse_lin, spec_lin [P,3] or NULL.  ws: at least nero_relight_workspace_bytes(P, Dd, Ds) bytes, 4-byte aligned.  P == 0 does nothing.
 * Limits on Dd, Ds and P as for nero_relight_rays. */
int nero_bvh_relight(void* handle, const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                     const float* env, int eh, int ew, int convention, const float* rot /* host [9] or NULL */, float clamp_max,
                     float* rgb_lin /* [P,3] */, float* diffuse_lin /* [P,3] or NULL */, float* spec_lin /* [P,3] or NULL */, void* ws,
                     size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
