/* nero_hip_bounce.h -- C ABI of libnero_hip.so, sixth header: one bounce of inter-reflection in the relighter.
 *
 * Conventions are those of nero_hip_relight.h and nero_hip_envsample.h: device pointers to fp32 (int64 / int32 / uint32 / bytes where stated),
 * every call asynchronous on `stream`, 0 on success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here
 * allocates or synchronises.  Arguments are validated before any device call.
 *
 * THE MODEL.  Path depth two: camera, x, y, map.  For sample direction w of the point x (the sample set of nero_relight_rays /
 * nero_relight_mis_rays, bit for bit):
 *   primary ray free:                           L = env(w), as nero_bvh_relight
 *   primary ray meets the mesh at y (closest hit within 10):   L = L_o(y, -w), one sample of y's direct lighting with a shadow ray of its
 *                                               own; black when that shadow ray is blocked or the sample is dead.  No further bounce.
 * L then goes through the primary estimator unchanged: the two-strategy weight of nero_bvh_relight, or the mixture of nero_bvh_relight_mis.
 * The closest-hit walk accepts a triangle exactly when the any-hit walk of the no-bounce kernels does, so the bounced lanes are exactly the
 * lanes those kernels call blocked: diffuse_lin and spec_lin below are the no-bounce kernels' outputs bit for bit.
 *
 * THE SURFACE AT y, from the caller's mesh verts [V,3], tris [T,3] int32 (the arrays the tree was built from: T must be the handle's triangle
 * count), mat5 [V,5] = (metallic, PERCEPTUAL roughness, albedo) and optionally normals [V,3].  Every product and sum rounded on its own:
 *   face = the caller's index of the hit triangle, (u, v) = nero_bvh_trace_faces' bary, (i0, i1, i2) = tris[face]; an index outside [0, V)
 *   makes the lane contribute 0 (state 4 below) and nothing of verts, mat5 or normals is read for it
 *   a(X) = ((1 - u - v) X[i0] + u X[i1]) + v X[i2];  y = a(verts), (metallic, rough, albedo) = a(mat5), alpha = rough rough
 *   normal: normals == NULL: g = (V1 - V0) x (V2 - V0), negated when g.w > 0 (turned against the incoming ray); else g = a(normals), not
 *   turned.  n2 = norm(norm(g)), view = norm(-w), norm(a) = a / max(|a|, 1e-12)
 *   NoV = sat(view.n2), reflection = (view.n2) n2 2 - view, and the two tangent frames of nero_mc_point_setup (get_orthogonal_directions of n2
 *   and of the reflection, then the cross products); no azimuth rotation.
 *
 * THE SECONDARY SAMPLE.  Shares c_d = (float) Dd / (float) D, c_s = (float) Ds / (float) D (D = Dd + Ds + Dl; Dl = 0 in the two-strategy
 * variant).  Three variates from a counter hash of the point's key and the lane's sample index j (uint32 arithmetic):
 *   lowbias32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   k1 = lowbias32(key[p] + j 0x9E3779B9), k2 = lowbias32(k1 + 0x68E31DA4), k3 = lowbias32(k2 + 0x68E31DA4), u_i = (float)(k_i >> 8) 2^-24
 *   strategy 0 (u_1 < c_d): cosine-weighted around n2, (u_2, u_3) in the place of a table's (azimuth, elevation)
 *   strategy 1 (u_1 < c_d + c_s, or any other u_1 in the two-strategy variant): GGX around the reflection, (u_2, u_3) likewise
 *   strategy 2 (otherwise): the light draw of nero_hip_envsample.h from the variates (u_2, u_3)
 * Direction w2, origin y + 1e-5 w2; dead: geometry_type 0, strategy 1 or 2, n2.w2 < -1e-6.  Shadow ray: any hit within 10.
 *   L_o = [albedo (1 - metallic) (NoL / PI) / p_mix2 + S(w2) F D_ggx G / (4 NoV p_mix2 + 1e-5)] env(w2)
 * with p_mix2 = (Dd NoL / PI + Ds p_act + Dl p_l) / D and every term, guard and 1e-5 exactly as nero_bvh_relight_mis states them (p_l = 0
 * in the two-strategy variant; else the drawn cell's density for strategy 2 and the looked-up cell's for the others).
 * clamp_max > 0 caps env(w) and env(w2), and also each channel of L_o.
 */
#ifndef NERO_HIP_BOUNCE_H
#define NERO_HIP_BOUNCE_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of the workspaces of the two fused kernels: twelve floats per wavefront of (point, sample) lanes; 0 for arguments the call refuses */
size_t nero_relight_bounce_workspace_bytes(int P, int Dd, int Ds);
size_t nero_relight_mis_bounce_workspace_bytes(int P, int Dd, int Ds, int Dl);

/* nero_bvh_relight with one bounce.  Lane layout, padding to whole wavefronts, limits and lookup-on-a-free-ray-only as there; the primary
 * walk is the closest-hit walk, the secondary the any-hit walk on the same stack.  Partials of twelve floats per wavefront (direct diffuse,
 * direct specular, indirect diffuse, indirect specular) from the same butterfly, added in index order by a finishing kernel; no
 * floating-point atomic: the same bits on every run, for every chunking (a lane's bounce depends on key[p] and j alone) and for both walks.
 *   diffuse_lin, spec_lin   the direct terms: those of nero_bvh_relight, bit for bit
 *   indirect_lin            the bounced lanes' diffuse sum / Dd + their specular sum / D
 *   rgb_lin                 (diffuse_lin + spec_lin) + indirect_lin
 * key [P] uint32 or NULL (every key 0).  diffuse_lin, spec_lin, indirect_lin [P,3] or NULL.  T != the handle's triangle count, V < 1:
 * NERO_ERR_ARG.  ws: at least nero_relight_bounce_workspace_bytes(P, Dd, Ds) bytes, 4-byte aligned.  P == 0 does nothing. */
int nero_bvh_relight_bounce(void* handle, const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                            const float* env, int eh, int ew, int convention, const float* rot /* host [9] or NULL */, float clamp_max,
                            const float* verts /* [V,3] */, int V, const int* tris /* [T,3] */, int T, const float* mat5 /* [V,5] */,
                            const float* normals /* [V,3] or NULL */, const unsigned* key /* [P] or NULL */, float* rgb_lin /* [P,3] */,
                            float* diffuse_lin, float* spec_lin, float* indirect_lin, void* ws, size_t ws_bytes, void* stream);

/* nero_bvh_relight_mis with one bounce: as above, every term a mean over all D = Dd + Ds + Dl samples. */
int nero_bvh_relight_mis_bounce(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l,
                                const float* rand_l /* [P,2] or NULL */, int P, int Dd, int Ds, int Dl, int geometry_type, const float* env,
                                int eh, int ew, int convention, const float* rot /* host [9] or NULL */, float clamp_max, const int64_t* cdf,
                                const int64_t* info, const float* verts /* [V,3] */, int V, const int* tris /* [T,3] */, int T,
                                const float* mat5 /* [V,5] */, const float* normals /* [V,3] or NULL */, const unsigned* key /* [P] or NULL */,
                                float* rgb_lin /* [P,3] */, float* diffuse_lin, float* spec_lin, float* indirect_lin, void* ws, size_t ws_bytes,
                                void* stream);

/* The same device functions writing instead of reducing: what lane (p, j) of the fused kernels decides, at row p D + j.  tab_l == NULL
 * selects the two-strategy variant (Dl must be 0; rand_l, cdf, info, gh, gw are not read), else the MIS variant (cdf, info, gh, gw as for
 * nero_relight_mis_rays).  No secondary shadow ray is walked and no map is read.  Each output may be NULL:
 *   state [P D] bytes    0 primary ray free, 1 primary sample dead, 2 bounced, 3 bounced with a dead secondary sample, 4 the hit face names
 *                        a vertex outside [0, V)
 *   face [P D] int32, bary [P D,2]   of the primary hit, as nero_bvh_trace_faces reports them (-1 and (0, 0) for states 0 and 1)
 *   sec_o, sec_d [P D,3] origin and direction of the secondary sample (states 2 and 3; else zeros)
 *   strategy [P D] int32 0, 1 or 2 (states 2 and 3; else -1);  pdf_l [P D] = p_l of the secondary direction (else 0)
 *   cell [P D] int32     the table's cell p_l was read from: the drawn cell of strategy 2, the looked-up cell of the others (-1 in the
 *                        two-strategy variant and for the other states) */
int nero_relight_bounce_rays(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l /* or NULL */,
                             const float* rand_l /* [P,2] or NULL */, int P, int Dd, int Ds, int Dl, int geometry_type, const int64_t* cdf,
                             const int64_t* info, int gh, int gw, const float* verts /* [V,3] */, int V, const int* tris /* [T,3] */, int T,
                             const float* mat5 /* [V,5] */, const float* normals /* [V,3] or NULL */, const unsigned* key /* [P] or NULL */,
                             unsigned char* state, int* face, float* bary, float* sec_o, float* sec_d, int* strategy, float* pdf_l,
                             int* cell, void* stream);

#ifdef __cplusplus
}
#endif
#endif
