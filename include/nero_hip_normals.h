/* nero_hip_normals.h -- C ABI of libnero_hip.so, seventh header: smooth per-vertex normals of a triangle mesh.
 *
 * A vertex normal is the normalised weighted sum of the normals of the faces around the vertex, weighted by the faces' areas or by their
 * angles at the vertex.  The relighter interpolates them for smooth shading (nero_amd/relight.py), the PLY writer stores them.
 *
 * Conventions are those of nero_hip.h: device pointers, verts [V,3] fp32, tris [T,3] int32, every call asynchronous on `stream` (a
 * hipStream_t passed as void*), 0 on success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or
 * synchronises.  Arguments are validated before any device call.
 *
 * DETERMINISM: the same mesh and weight give the same bits on every run and for every order of the triangles.  A face's contribution
 * becomes an INTEGER (fixed point) before it is added, and integer addition is associative, so the order in which the adds land decides
 * nothing; no floating-point atomic is used.  Every float64 operation below is rounded on its own (no contraction), sqrt is correctly
 * rounded: a numpy restatement reproduces the area mode bit for bit and the angle mode up to the last places of atan2
 * (tests/normals_ref.py).
 */
#ifndef NERO_HIP_NORMALS_H
#define NERO_HIP_NORMALS_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspace of nero_vertex_normals; 0 (reason in nero_last_error) for a V or T outside [1, 2^31 - 2] */
size_t nero_vertex_normals_workspace_bytes(int64_t V, int64_t T);

/* Per face t, its vertices widened to float64: c = (p1 - p0) x (p2 - p0).  The face is REFUSED when an index lies outside [0, V) or a
 * component of c is not finite, DEGENERATE when c is zero (a repeated index falls here by arithmetic); neither contributes.  L = the bit
 * length of T - 1.
 *   weight 0 (area)   mx = the largest |c_k| over the accepted faces and k in {x, y, z}, e = its frexp exponent (0 for mx = 0), B = min(40,
 *                     61 - L); each of the three corners adds q_k = llrint(ldexp(c_k, B - e)) to its vertex (llrint: half to even).
 *   weight 1 (angle)  len = sqrt((cx cx + cy cy) + cz cz), n = c / len; at corner i, with a = p(i+1) - p(i) and b = p(i+2) - p(i) (indices
 *                     mod 3), theta = atan2(|a x b|, a . b) with |a x b| formed like len and a . b = (ax bx + ay by) + az bz; the corner
 *                     adds llrint(ldexp(theta n_k, B)) with B = min(40, 59 - L).
 * A vertex's three int64 sums s (below 2^61 in magnitude) are converted to float64, l = sqrt((sx sx + sy sy) + sz sz), and normals[v] =
 * (float)(s_k / l); (0, 0, 0) when all three sums are zero (an unreferenced vertex, faces that cancel).
 * info [4] int64 (DEVICE) = {refused faces, degenerate faces, vertices written as zero, e (0 in angle mode)}.  normals [V,3] fp32.
 * ws: nero_vertex_normals_workspace_bytes(V, T) bytes, 256-byte aligned.  T and V in [1, 2^31 - 2]; weight 0 or 1. */
int nero_vertex_normals(const float* verts, int64_t V, const int* tris, int64_t T, int weight, void* ws, float* normals /* [V,3] */,
                        int64_t* info /* [4] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif
