/* nero_hip_texfetch.h -- C ABI of libnero_hip.so, ninth header: mip-mapped UV material lookup for the relighter.
 *
 * The maps that bake_materials writes (albedo, metallic, roughness as 8-bit sRGB-encoded images over a UV atlas) are packed into one record
 * per texel, reduced to a mip pyramid, and fetched at the relighter's hits with a trilinear filter whose level follows the pixel's footprint
 * (nero_amd/texfetch.py, Relighter(textures=...)).
 *
 * Conventions are those of nero_hip_relight.h: device pointers, every call asynchronous on `stream` (a hipStream_t passed as void*), 0 on
 * success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or synchronises.  Arguments are
 * validated before any device call.  Maps are [h, w] row-major, texel (row y, column x) has its centre at u = (x + 0.5) / w, v = (y + 0.5) / h
 * (nero_hip.h); h and w lie in [1, 16384].
 *
 * RECORDS AND PYRAMID.  A texel record is 8 bytes, 8-byte aligned: (r, g, b, metallic, roughness, 0, 0, 0).  Level k of an h x w map is
 * (h >> k) x (w >> k) records; a level exists while both sizes of the one below are even (at most 15 levels); the levels lie back to back,
 * level 0 first.  Every byte of level k + 1 is (a + b + c + d + 2) >> 2 of the 2 x 2 block below, the rule of nero_tex_downsample2.
 *
 * DECODING.  A byte b stands for lut[b], a 256-entry fp32 table the caller makes on the host: the inverse of the sRGB curve
 * nero_tex_quantize applies to every channel.  The roughness channel holds the network's alpha; the output carries sqrtf of it, the
 * perceptual roughness of the relighter's mat5.
 *
 * ARITHMETIC: fp32, every product and sum rounded on its own (no contraction into fused multiply-adds), IEEE sqrtf and division, no
 * floating-point atomics: the same inputs give the same bits on every run, the bits of the numpy restatement of the tests
 * (tests/texfetch_ref.py).
 */
#ifndef NERO_HIP_TEXFETCH_H
#define NERO_HIP_TEXFETCH_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* levels of the pyramid of an h x w map: 1 + min(ctz(h), ctz(w)), at most 15; 0 for a size outside [1, 16384].  Host only. */
int nero_tex_mip_levels(int64_t h, int64_t w);

/* bytes of the whole pyramid (8 per record, all levels); 0 for a size outside [1, 16384].  Host only. */
size_t nero_tex_mip_bytes(int64_t h, int64_t w);

/* Level 0: out [h w] records from albedo u8 [h,w,3], metallic u8 [h,w], roughness u8 [h,w].  Refused (NERO_ERR_ARG): a size outside
 * [1, 16384], a null pointer, an `out` that is not 8-byte aligned. */
int nero_tex_pack(const unsigned char* albedo, const unsigned char* metallic, const unsigned char* roughness, int64_t h, int64_t w,
                  unsigned char* out, void* stream);

/* Levels 1 and above of `pyramid` (nero_tex_mip_bytes(h, w) bytes, level 0 filled) from the level below each, one launch per level; the
 * three padding bytes of every record stay 0.  A map with one level: nothing is launched.  Refused: as nero_tex_pack. */
int nero_tex_mip_build(unsigned char* pyramid, int64_t h, int64_t w, void* stream);

/* Texels per world unit of every face: scale[f] = sqrtf(A_uv / A_world), A_uv = |ax by - ay bx| with a = ((vt1 - vt0).x w, (vt1 - vt0).y h)
 * and b likewise of vt2 (indices ft[f]), A_world = |(V1 - V0) x (V2 - V0)| (indices tris[f]).  0 where either area is 0, where the ratio
 * is not finite, or where an index of tris[f] lies outside [0, V) or one of ft[f] outside [0, Vt): nothing is read through a bad index.
 * verts [V,3], tris [T,3] int32, vt [Vt,2], ft [T,3] int32, scale [T].  T == 0 does nothing.  Refused: a size outside [1, 16384], a
 * negative count or one of 2^31 - 1 or more, a null pointer where the count is positive. */
int nero_tex_face_scale(const float* verts, int64_t V, const int* tris, const float* vt, int64_t Vt, const int* ft, int64_t T, int64_t h,
                        int64_t w, float* scale, void* stream);

/* The fused fetch, one lane per hit i.  With (j0, j1, j2) = ft[face[i]], (u, v) = bary[i] and a(X) = (((1 - u) - v) X[j0] + u X[j1]) + v X[j2]:
 *   uv = a(vt);
 *   s = fmaxf(((depth[i] spread) scale[face[i]]) lod_scale, 1) (a NaN gives 1): the pixel's footprint in texels of level 0.  lod_scale is
 *       exp2(lod_bias), taken by the caller;
 *   l = min(exponent of s, L - 1);  t = s 2^-l - 1 in [0, 1), exact; t = 0 at the top level (l = L - 1), so for an infinite s too;
 *   in level k of size (h_k, w_k): x = fminf(fmaxf(uv.x w_k - 0.5, -1), w_k) (a NaN gives -1), x0 = floorf(x), fx = x - x0, columns x0 and
 *       x0 + 1 clamped to [0, w_k - 1]; y likewise with h_k: a coordinate outside the map, or not finite, reads edge texels;
 *   every tap is decoded through lut and mixed in the form p + f (q - p): along x, then along y, then, where t != 0, between levels l and
 *       l + 1 by t (for t = 0 the mix returns level l's value bit for bit, and level l + 1 is not read);
 *   mat5[i] = (metallic, sqrtf(roughness channel), r, g, b).
 * A constant map therefore returns its decoded value exactly at every level of detail.  face[i] < 0, face[i] >= T or an index of ft
 * outside [0, Vt) writes five zeros (and eight to dbg) and reads nothing else.  n == 0 does nothing.
 * dbg: NULL, or [n,8] fp32 = (l, t, x0, y0, fx, fy of level l, uv.x, uv.y): what the lane decided.
 * pyramid: nero_tex_mip_bytes(h, w) bytes, 8-byte aligned; lut [256] fp32; vt [Vt,2]; ft [T,3] int32; scale [T]; face [n] int32; bary
 * [n,2]; depth [n]; mat5 [n,5].  Refused: a size outside [1, 16384], a negative count or one of 2^31 - 1 or more, a spread or lod_scale
 * that is NaN or negative, a null pointer where the count is positive, a pyramid that is not 8-byte aligned. */
int nero_tex_materials(const unsigned char* pyramid, int64_t h, int64_t w, const float* lut, const float* vt, int64_t Vt, const int* ft,
                       int64_t T, const float* scale, const int* face, const float* bary, const float* depth, int64_t n, float spread,
                       float lod_scale, float* mat5, float* dbg, void* stream);

/* Per-vertex materials, the stand-in the bounce kernels read at secondary hits: vertex i takes the level-0 bilinear fetch (the arithmetic
 * above with l = 0, t = 0) at vt[ft[f][c]] of its lowest-numbered face corner 3 f + c with tris[f][c] == i, chosen by an integer atomic
 * minimum into owner_ws [V] int32 (so the same on every run); mat5_v [V,5] = (metallic, sqrtf(roughness channel), r, g, b).  A vertex no
 * face names, or one whose corner has an ft index outside [0, Vt), gets five zeros; an index of tris outside [0, V) is passed over.
 * owner_ws holds the chosen corner numbers afterwards (2^31 - 1: none).  V == 0 does nothing.  Refused: as nero_tex_materials, and a T
 * of (2^31 - 1) / 3 or more. */
int nero_tex_vertex_materials(const unsigned char* pyramid, int64_t h, int64_t w, const float* lut, const float* vt, int64_t Vt,
                              const int* tris, const int* ft, int64_t T, int64_t V, int* owner_ws, float* mat5_v, void* stream);

#ifdef __cplusplus
}
#endif
#endif
