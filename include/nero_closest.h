/* nero_closest.h -- C ABI of libnero_hip.so, tenth header: exact point-to-mesh distance on the mesh tracer's BVH.
 *
 * The entry points of nero_hip.h and nero_hip_visibility.h ask a mesh what a ray hits.  The one below asks how far a point is from the
 * surface and where the nearest point of it lies -- cloud-to-mesh distance, the distance a simplified mesh moved from its source, the
 * start of detail and attribute transfer -- on the same handle (nero_bvh_create / nero_bvh_create_device), by a third walk over the same
 * nodes.
 *
 * Conventions are those of nero_hip_visibility.h: device pointers to fp32 (int32 where stated), points as [n,3] rows, the call
 * asynchronous on `stream` (a hipStream_t passed as void*), 0 on success or a negative NERO_ERR_* code with a message in
 * nero_last_error().  Nothing here allocates or synchronises.  Arguments are validated before any device call.
 */
#ifndef NERO_CLOSEST_H
#define NERO_CLOSEST_H
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Closest point.  For a triangle as the tree stores it (v0, e1 = v1 - v0, e2 = v2 - v0) the point-to-triangle function yields weights
 * b1 >= 0, b2 >= 0, b1 + b2 <= 1 and d2, the squared length of (p - v0) - (b1 e1 + b2 e2), every product and sum rounded on its own: the
 * minimum over the nearest points of the three edge segments and the clamped foot of the perpendicular (nero_amd/csrc/closest_point_math.h
 * IS the definition; tests/closest_ref.py restates it in numpy).  d2 belongs to a point OF the triangle: it may exceed the true distance by
 * rounding, never undercut it by more; a zero-area triangle is the segment or point it is; finite vertices give a finite distance.
 * Per point i the call reports the minimum of that function over ALL triangles, bit for bit, whatever the tree:
 *   dist[i]  = sqrtf(d2);  face[i] = the LOWEST caller face index among the triangles that attain the minimum;
 *   bary[i]  = (b1, b2) on that face;  point[i] = v0 + (b1 e1 + b2 e2), each operation rounded on its own.
 * max_dist: only triangles with d2 <= max_dist * max_dist (one fp32 product) count; +inf: no limit; <= 0 or NaN: NERO_ERR_ARG.  A point with
 * nothing in range, or with a non-finite coordinate, reports face -1, dist +inf and zero weights and point.  The box bound of the walk is
 * padded for a scene of unit scale queried from |coordinate| <= 10, the tracer's own domain.  The traversal follows nero_bvh_set_traversal
 * and the tree's depth as nero_bvh_trace does.  No atomics: the same bits on every run.  n == 0 does nothing; n <= 2^36.  Null handle,
 * pts, dist or face: NERO_ERR_ARG. */
int nero_bvh_closest(void* handle, const float* pts /* [n,3] */, int64_t n, float max_dist /* <= 0 or NaN: refused; +inf: none */,
                     float* dist /* [n] */, int* face /* [n] */, float* bary /* [n,2] or NULL */, float* point /* [n,3] or NULL */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
