/* nero_hip_surface.h -- C ABI of libnero_hip.so, fourth header: area-weighted sampling of points on the surface of a triangle mesh.
 *
 * What the reference's eval.md leaves to CloudCompare ("sample points on the surface", 500k by default) ahead of eval_real_shape.py: a
 * triangle is chosen with probability proportional to its area, a point uniformly inside it.
 *
 * Conventions are those of nero_hip.h: device pointers, verts [V,3] fp32, tris [T,3] int32, every call asynchronous on `stream` (a
 * hipStream_t passed as void*), 0 on success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or
 * synchronises.  Arguments are validated before any device call.
 *
 * DETERMINISM: the same mesh, n_total, seed and mode give the same bits on every run and for every way of cutting [0, n_total) into calls.
 * The areas become INTEGER weights before they are summed, so the scan's result does not depend on how it is partitioned; sample i is a
 * function of (i, n_total, seed) alone; no floating-point atomic is used.  Every float64 operation below is rounded on its own (no
 * contraction), sqrt is correctly rounded: a numpy restatement reproduces every output bit for bit (tests/surface_ref.py).
 */
#ifndef NERO_HIP_SURFACE_H
#define NERO_HIP_SURFACE_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace of nero_surface_cdf; 0 (reason in nero_last_error) for a T outside [1, 2^31 - 2] or when hipCUB's size query fails */
size_t nero_surface_cdf_workspace_bytes(int64_t T);

/* Weights and their running sum.  Per triangle t, its vertices widened to float64: c = (p1 - p0) x (p2 - p0), a2 = sqrt((cx cx + cy cy) +
 * cz cz) (twice the area); a2 = 0 when an index lies outside [0, V) or a2 is not finite.  mx = max a2, e = its frexp exponent (mx < 2^e;
 * 0 for mx = 0), L = the bit length of T - 1, B = min(40, 62 - L), w[t] = (uint64) floor(ldexp(a2, B - e)), cdf[t] = w[0] + ... + w[t]
 * (< 2^62).  info [4] int64 (DEVICE) = {cdf[T - 1], the number of triangles with w = 0, e, B}; the area of the mesh is
 * info[0] 2^(e - B) / 2 up to the flooring.  cdf [T] int64.  ws: nero_surface_cdf_workspace_bytes(T) bytes, 256-byte aligned.
 * T and V in [1, 2^31 - 2]. */
int nero_surface_cdf(const float* verts, int64_t V, const int* tris, int64_t T, void* ws, int64_t* cdf /* [T] */, int64_t* info /* [4] */,
                     void* stream);

/* Samples [first, first + n) of n_total, sample i a function of (i, n_total, seed, stratified) alone.  With lowbias32 of
 * nero_hip_visibility.h: h1 = lowbias32(i 0x9E3779B9 + seed), h2 = lowbias32(h1 + 0x68E31DA4), h3, h4 from h2, h3 by the same step.
 *   u       stratified != 0: ((double) i + (h1 >> 8) 2^-24) / (double) n_total (one jittered sample per stratum of the total weight:
 *           every triangle gets its expected count to within 2); else ((uint64) h1 << 21 | h4 >> 11) 2^-53 (independent draws)
 *   face    the first t with cdf[t] > min((uint64)(u (double) total), total - 1), total = info[0]: a triangle of weight 0 is never chosen
 *   point   r1 = (h2 >> 8) 2^-24, r2 = (h3 >> 8) 2^-24, su = sqrt(r1), b0 = 1 - su, b1 = su (1 - r2), b2 = su r2,
 *           (b0 p0 + b1 p1) + b2 p2 per axis in float64, stored as fp32
 * pts [n,3] fp32.  Optional, each NULL or: face [n] int32; bary [n,2] fp32 = (b1, b2); normal [n,3] fp32 = c / |c| of the face (the
 * winding's direction).  total == 0 (a mesh without area): face -1, everything else 0.  cdf, info: as nero_surface_cdf left them, for the
 * same verts and tris.  n == 0 does nothing.  T and V in [1, 2^31 - 2]; 0 <= first, first + n <= n_total <= 2^31 - 1. */
int nero_surface_sample(const float* verts, int64_t V, const int* tris, int64_t T, const int64_t* cdf, const int64_t* info, int64_t first,
                        int64_t n, int64_t n_total, unsigned seed, int stratified, float* pts /* [n,3] */, int* face /* [n] or NULL */,
                        float* bary /* [n,2] or NULL */, float* normal /* [n,3] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
