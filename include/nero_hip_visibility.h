/* nero_hip_visibility.h -- C ABI of libnero_hip.so, second header: visibility queries on the mesh tracer's BVH and ambient occlusion.
 *
 * The entry points of nero_hip.h answer "where is the closest hit" (nero_bvh_trace and its variants).  The ones below answer the cheaper
 * question "is anything in the way within distance t" -- what ambient occlusion, shadowing and light-visibility tests reduce to -- on the
 * same handle (nero_bvh_create / nero_bvh_create_device), with the same box and triangle arithmetic, operation by operation.
 *
 * Conventions are those of nero_hip.h: device pointers to fp32 (int32 / bytes where stated), rays and points as [n,3] rows, every call
 * asynchronous on `stream` (a hipStream_t passed as void*), 0 on success or a negative NERO_ERR_* code with a message in
 * nero_last_error().  Nothing here allocates or synchronises.  Arguments are validated before any device call.
 */
#ifndef NERO_HIP_VISIBILITY_H
#define NERO_HIP_VISIBILITY_H
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Any hit.  occluded[i] = 1 when some triangle passes the tracer's own intersection predicates for ray i with 0 < t < tmax_i (strictly,
 * as the closest-hit search compares against its best distance), else 0; tmax_i = tmax[i] when `tmax` is given, else tmax_all.  tmax_all
 * must lie in (0, 10] -- 10 is the tracer's miss distance -- whether or not `tmax` is given; per-ray values are clamped to [0, 10] (0 and
 * below: nothing is accepted; NaN counts as 10).  skip [n] bytes or NULL: a ray with a non-zero byte reports 0 without a node visit.  Up to
 * rounding of the box test near t = tmax_i, occluded[i] == (depth_i < tmax_i) for the depth nero_bvh_trace reports.  The traversal kernel
 * follows nero_bvh_set_traversal and the tree's depth exactly as nero_bvh_trace does, and stops at the first accepted triangle.  n == 0
 * does nothing; n <= (2^31 - 1) / 3.  Null handle, rays or output: NERO_ERR_ARG. */
int nero_bvh_occluded(void* handle, const float* rays_o, const float* rays_d, int n, const float* tmax /* [n] or NULL */, float tmax_all,
                      const unsigned char* skip /* [n] or NULL */, unsigned char* occluded /* [n] */, void* stream);

/* The ambient-occlusion sample set: S rays per point, ray j S + s at that index.  For point j (position pts[j], UNIT normal nrm[j], hash
 * key key[j] -- the texel's row-major index, so that the set does not depend on how the points are chunked) and sample s, in uint32 / fp32:
 *   lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   h1 = lowbias32(key * 0x9E3779B9 + seed), h2 = lowbias32(h1 + 0x68E31DA4), r1 = (h1 >> 8) 2^-24, r2 = (h2 >> 8) 2^-24
 *   a = frac((s + 0.5) / S + r1), b = frac(bitreverse32(s) 2^-32 + r2)              (one fp32 add and one x - floorf(x) each)
 *   local direction (sqrtf(a) cos phi, sqrtf(a) sin phi, sqrtf(1 - a)), phi = 2 pi b  (cosine-weighted; sincosf)
 *   frame (Duff et al. 2017): sg = copysignf(1, n.z), c0 = -1 / (sg + n.z), c1 = n.x n.y c0,
 *                             t = (1 + sg n.x^2 c0, sg c1, -sg n.x), u = (c1, sg + n.y^2 c0, -n.y)
 *   d = normalize(x t + y u + z n), o = p + bias n
 * with every product and sum rounded on its own.  S: a power of two in [8, 1024]; n S <= 2^31 - 64, else NERO_ERR_ARG (call in chunks). */
int nero_ao_rays(const float* pts, const float* nrm, const int* key, int n, int S, unsigned seed, float bias,
                 float* rays_o /* [n S,3] */, float* rays_d /* [n S,3] */, void* stream);

/* Ambient occlusion counts: count[j] = how many of point j's S rays (those nero_ao_rays writes, made by the same device function) are
 * occluded within tmax (as nero_bvh_occluded with tmax_all = tmax) -- without a ray ever being stored.  Integer counts from wave ballots
 * (and, for S >= 64, one integer atomic add per wavefront into counts the call zeroes first): the same bits on every run.  tmax in (0, 10];
 * S and n S as for nero_ao_rays. */
int nero_bvh_ao(void* handle, const float* pts, const float* nrm, const int* key, int n, int S, unsigned seed, float bias, float tmax,
                int* count /* [n] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
