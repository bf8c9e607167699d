/* nero_transfer.h -- C ABI of libnero_hip.so, eleventh header: detail transfer from a dense mesh (the source) to a simplified one with a
 * UV atlas (the target) -- attribute interpolation at the points nero_bvh_closest returns, per-UV-vertex tangents, the encoding of a
 * tangent- or object-space normal map, its mip pyramid, and the fused lookup that perturbs the relighter's normals at its hits
 * (nero_amd/transfer.py, Relighter(normal_map=...)).
 *
 * Conventions are those of nero_hip_texfetch.h: device pointers, every call asynchronous on `stream` (a hipStream_t passed as void*), 0 on
 * success or a negative NERO_ERR_* code with a message in nero_last_error().  Nothing here allocates or synchronises.  Arguments are
 * validated before any device call.  Maps are [h, w] row-major, texel (row y, column x) has its centre at u = (x + 0.5) / w,
 * v = (y + 0.5) / h (nero_hip.h); h and w lie in [1, 16384]; counts are non-negative and below 2^31 - 1.
 *
 * ARITHMETIC: fp32 (float64 where stated), every product and sum rounded on its own (no contraction into fused multiply-adds), IEEE sqrtf
 * and division, no floating-point atomics: the same inputs give the same bits on every run, the bits of the numpy restatement of the
 * tests (tests/transfer_ref.py).  dot(a, b) below is (a.x b.x + a.y b.y) + a.z b.z; |a| is sqrtf(dot(a, a)).
 *
 * THE FRAME at a point of face f, from a normal N (any length), a tangent T (any length) and s = face_sign[f]:
 *   n  = N / |N|, component by component;
 *   p  = T - dot(T, n) n;  where dot(p, p) > 1e-12 dot(T, T) does NOT hold (a zero tangent, T parallel to N, a NaN) T is replaced by the unit
 *        vector of the axis k with the smallest |n_k| (the lowest k among equals) and p is taken again: that one always has a direction;
 *   T' = p / |p|;
 *   B  = s' (n x T'), s' = -1 where s < 0 and +1 otherwise.
 * face_sign is the handedness of the face's UV chart as a FILE stores it, (u, 1 - v): +1 where (u, 1 - v) runs counter-clockwise seen from
 * the side the winding normal points to, -1 where it is mirrored.  With it B points along increasing file v = 1 - v of the row coordinate:
 * green up, the OpenGL convention.  (On the square x, y in [0, 1] with normal +z: u = x, file v = y gives T' = +x, B = +y, sign +1; u = -x
 * gives T' = -x, B = +y, sign -1.)  The frame exists where |N| is finite and not zero.
 *
 * THE BYTES of a unit vector x: clamp(lrintf(127 x_k) + 128, 1, 255) per component; a byte b stands for (b - 128) / 127.  Zero is exactly
 * 128, the flat tangent-space normal exactly (128, 128, 255).
 */
#ifndef NERO_TRANSFER_H
#define NERO_TRANSFER_H
#include <stddef.h>
#include <stdint.h>
#include "nero_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A per-vertex attribute at (face, bary) pairs, what nero_bvh_closest and nero_bvh_trace_faces return.  One lane per query i: with
 * (i0, i1, i2) = tris[face[i]] and (b1, b2) = bary[i], out[i][c] = a0 + (b1 (a1 - a0) + b2 (a2 - a0)) for c < C, a_k = attr[i_k][c].
 * face[i] outside [0, T) or an index of tris[face[i]] outside [0, V) writes `fill` to all C channels and reads nothing else.
 * attr [V,C], tris [T,3] int32, face [n] int32, bary [n,2], out [n,C].  n == 0 does nothing.  Refused (NERO_ERR_ARG): C outside [1, 8], a
 * negative count or one of 2^31 - 1 or more, a null pointer where the count is positive. */
int nero_mesh_attr_at(const float* attr, int64_t V, int C, const int* tris, int64_t T, const int* face, const float* bary, int64_t n,
                      float fill, float* out, void* stream);

/* bytes of the workspace of nero_uv_tangents (256 + three int64 sums per UV vertex, rounded up to 256); 0 for a count out of range. */
size_t nero_uv_tangents_workspace_bytes(int64_t Vt, int64_t T);

/* Per UV vertex (an index into vt: a seam keeps a frame per side) the tangent along increasing u.  Per face in float64, from the fp32
 * inputs: e1 = P1 - P0, e2 = P2 - P0 (tris[f]); (du1, dv1) = vt1 - vt0, (du2, dv2) = vt2 - vt0 (ft[f]); det = du1 dv2 - du2 dv1;
 * t = (e1 dv2 - e2 dv1) sign(det); c = e1 x e2; the face adds (t / |t|) |c| -- the unit tangent times twice the face's area -- to each of
 * its three UV vertices, as fixed-point integers with 64-bit integer atomic adds, by the scheme of nero_vertex_normals' area mode: with
 * 2^(e-1) <= max |c| < 2^e over the contributing faces and B = min(40, 61 - bit_length(T - 1)), a component x adds llrint(x 2^(B - e)).
 * Integer sums: the same bits on every run and for every order of the triangles.  tangent[j] = the sum as float64, normalised, rounded to
 * fp32; (0, 0, 0) where the sum is zero.  face_sign [T] int8: -sign(det) (the file's handedness, see THE FRAME), and 0 for a face that
 * contributes nothing: an index of tris[f] outside [0, V) or of ft[f] outside [0, Vt), a c or t that is not finite (refused), det == 0
 * or NaN, c == 0 or t == 0 (degenerate).  info [4] int64 on the device: refused faces, degenerate faces, UV vertices written as zero, e.
 * verts [V,3], tris [T,3] int32, vt [Vt,2], ft [T,3] int32, ws: nero_uv_tangents_workspace_bytes, 256-byte aligned, tangent [Vt,3].
 * T == 0 or Vt == 0 does nothing.  Refused: a count out of range, a null pointer where the count is positive, a misaligned ws. */
int nero_uv_tangents(const float* verts, int64_t V, const int* tris, const float* vt, int64_t Vt, const int* ft, int64_t T, void* ws,
                     float* tangent, signed char* face_sign, int64_t* info, void* stream);

/* The bytes of a normal map at the covered texels, one lane per texel i: frame normal N = nrm[i], tangent T = tan[i], s = sign[i] (the
 * face_sign of the texel's triangle), source normal ns[i], valid[i], written to map[3 texel[i] ..] of an [h,w,3] map; a texel[i] outside
 * [0, h w) writes nothing.  space 0 (tangent): x = (dot(ns, T'), dot(ns, B), dot(ns, n)) / its length in THE FRAME; space 1 (object):
 * x = ns / |ns|.  A texel is INVALID where valid[i] == 0 (no source within reach), where ns is not finite or zero, where x is not finite,
 * or (tangent space) where the frame does not exist: it takes the flat bytes (128, 128, 255) in tangent space, the bytes of n in object
 * space ((128, 128, 255) too where n does not exist), and is counted into *invalid (int64 on the device, zeroed by the call; integer
 * atomic adds).  n == 0 does nothing.  Refused: a size outside [1, 16384], a count out of range, space not 0 or 1, a null
 * pointer. */
int nero_nmap_encode(const float* nrm, const float* tan, const signed char* sign, const float* ns, const unsigned char* valid,
                     const int* texel, int64_t n, int64_t h, int64_t w, int space, unsigned char* map, int64_t* invalid, void* stream);

/* bytes of the whole pyramid of normal-map records (4 per record; levels and layout as nero_tex_mip_levels); 0 for a size out of range. */
size_t nero_nmap_mip_bytes(int64_t h, int64_t w);

/* Level 0: out [h w] records (x, y, z, 0) of 4 bytes, 4-byte aligned, from map u8 [h,w,3]. */
int nero_nmap_pack(const unsigned char* map, int64_t h, int64_t w, unsigned char* out, void* stream);

/* Levels 1 and above of `pyramid` (nero_nmap_mip_bytes(h, w) bytes, level 0 filled): every byte is (a + b + c + d + 2) >> 2 of the 2 x 2
 * block below, the rule of nero_tex_downsample2; the fourth byte stays 0.  A flat map is flat at every level. */
int nero_nmap_mip_build(unsigned char* pyramid, int64_t h, int64_t w, void* stream);

/* The fused lookup, one lane per hit i.  UV, footprint, level l, weight t and the taps are exactly those of nero_tex_materials
 * (nero_hip_texfetch.h) from (face, bary, vt, ft, depth, spread, scale, lod_scale); the three bytes of every tap are decoded as
 * (b - 128) / 127 and mixed as p + f (q - p) along x, along y and, where t != 0, between levels l and l + 1: (x, y, z).
 *   space 0: THE FRAME from N = nrm_in[i], T = a(tangent) (the hit's UV weights over tangent[ft[face]]), s = face_sign[face]:
 *            nrm_out[i] = ((x T' + y B) |N|) + z N, and z N alone where x == 0 and y == 0: a fetch that decodes to (0, 0, 1) returns
 *            nrm_in[i] bit for bit, the sign of a zero included.  (|N| scales the tilt because N may have any length;)
 *   space 1: nrm_out[i] = (x, y, z).
 * Where the result is not finite, is zero, or dot(result, nrm_in[i]) > 0 does not hold, and where the frame does not exist,
 * nrm_out[i] = nrm_in[i].  The result is NOT normalised.  face[i] outside [0, T) or an index of ft outside [0, Vt) copies nrm_in[i]
 * (zeros to dbg) and reads nothing else.  dbg: NULL or [n,8] = (l, t, x0, y0, fx, fy of level l, u, v).  n == 0 does nothing.
 * pyramid: nero_nmap_mip_bytes(h, w) bytes, 4-byte aligned; tangent [Vt,3]; face_sign [T] int8; scale [T]; nrm_in, nrm_out [n,3].
 * Refused: a size outside [1, 16384], a count out of range, a spread or lod_scale that is NaN or negative, space not 0 or 1, a null
 * pointer where the count is positive, a misaligned pyramid. */
int nero_nmap_apply(const unsigned char* pyramid, int64_t h, int64_t w, const float* vt, int64_t Vt, const int* ft, int64_t T,
                    const float* scale, const float* tangent, const signed char* face_sign, const int* face, const float* bary,
                    const float* depth, const float* nrm_in, int64_t n, float spread, float lod_scale, int space, float* nrm_out, float* dbg,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
