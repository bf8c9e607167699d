// detail_transfer.hip -- detail transfer from a dense mesh to a simplified one with a UV atlas (include/nero_transfer.h):
// attribute interpolation at closest points, per-UV-vertex tangents, the bytes of a normal map, its pyramid and the fused lookup at the
// relighter's hits.
//   One lane owns one output (a query, a face, a UV vertex, a texel, a record, a hit); no LDS.  The only atomics are integer ones: the
//   fixed-point tangent sums (the scheme of mesh_normals.hip's area mode, so the sums are the same bits in whatever order the adds land)
//   and the counters.  Every index read from memory is checked before it is followed, and a texel number before it is written through.
//   The level-of-detail rule and the tap addresses are tex_lod.h's, shared with tex_fetch.hip.
// The file is compiled without floating-point contraction: every operation is the one the numpy restatement of the tests performs
// (tests/transfer_ref.py).  Arithmetic is written per component (tests/test_no_packed_fp32.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_transfer.h"
#include "common.h"
#include "device_prims.h"
#include "tex_lod.h"
#include "transfer_math.h"
#include "transfer_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_transfer;
using nero_prims::wave_max;
using nero_texfetch::Axis;
using nero_texfetch::hit_uv;
using nero_texfetch::in_range;
using nero_texfetch::lerp;
using nero_texfetch::Lod;
using nero_texfetch::lod_of;
using nero_texfetch::make_plan;
using nero_texfetch::Plan;
using nero_texfetch::Taps;
using nero_texfetch::taps_of;

typedef unsigned long long u64;

// ---- attributes at (face, bary) ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void attr_at_kernel(const float* __restrict__ attr, int64_t V, int C, const int* __restrict__ tris, int64_t T,
                                                          const int* __restrict__ face, const float* __restrict__ bary, int64_t n, float fill,
                                                          float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = face[i];
    int i0 = -1, i1 = -1, i2 = -1;
    if (in_range(f, T)) {
        i0 = tris[3 * (int64_t)f];
        i1 = tris[3 * (int64_t)f + 1];
        i2 = tris[3 * (int64_t)f + 2];
    }
    float* o = out + (int64_t)C * i;
    if (!(in_range(i0, V) && in_range(i1, V) && in_range(i2, V))) {
#pragma clang loop vectorize(disable) interleave(disable)
        for (int c = 0; c < C; ++c) o[c] = fill;
        return;
    }
    const float b1 = bary[2 * i], b2 = bary[2 * i + 1];
    const float* a0 = attr + (int64_t)C * i0;
    const float* a1 = attr + (int64_t)C * i1;
    const float* a2 = attr + (int64_t)C * i2;
    // (one channel at a time: the loop vectoriser would form packed fp32 arithmetic, which the library does without -- common.h)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int c = 0; c < C; ++c) o[c] = a0[c] + (b1 * (a1[c] - a0[c]) + b2 * (a2[c] - a0[c]));
}

// ---- tangents ---------------------------------------------------------------------------------------------------------------------------------
enum { FACE_OK = 0, FACE_REFUSED = 1, FACE_DEGENERATE = 2 };

struct FaceTangent {
    int j[3];                                                   // the UV vertices
    double w[3];                                                // (t / |t|) |c|
    double weight;                                              // |c|
    int sign;                                                   // -sign(det)
};

__device__ __forceinline__ double norm3d(const double* c) { return __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]); }

// nothing is read through an index out of range
__device__ __forceinline__ int face_tangent(const float* __restrict__ verts, int64_t V, const int* __restrict__ tris, const float* __restrict__ vt,
                                            int64_t Vt, const int* __restrict__ ft, int64_t f, FaceTangent* o) {
    const int i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
    o->j[0] = ft[3 * f], o->j[1] = ft[3 * f + 1], o->j[2] = ft[3 * f + 2];
    if (!(in_range(i0, V) && in_range(i1, V) && in_range(i2, V) && in_range(o->j[0], Vt) && in_range(o->j[1], Vt) && in_range(o->j[2], Vt)))
        return FACE_REFUSED;
    const float* p0 = verts + 3 * (int64_t)i0;
    const float* p1 = verts + 3 * (int64_t)i1;
    const float* p2 = verts + 3 * (int64_t)i2;
    const double e1[3] = {(double)p1[0] - (double)p0[0], (double)p1[1] - (double)p0[1], (double)p1[2] - (double)p0[2]};
    const double e2[3] = {(double)p2[0] - (double)p0[0], (double)p2[1] - (double)p0[1], (double)p2[2] - (double)p0[2]};
    const float* q0 = vt + 2 * (int64_t)o->j[0];
    const float* q1 = vt + 2 * (int64_t)o->j[1];
    const float* q2 = vt + 2 * (int64_t)o->j[2];
    const double du1 = (double)q1[0] - (double)q0[0], dv1 = (double)q1[1] - (double)q0[1];
    const double du2 = (double)q2[0] - (double)q0[0], dv2 = (double)q2[1] - (double)q0[1];
    const double det = du1 * dv2 - du2 * dv1;
    const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double sg = det > 0.0 ? 1.0 : -1.0;
    const double t[3] = {(e1[0] * dv2 - e2[0] * dv1) * sg, (e1[1] * dv2 - e2[1] * dv1) * sg, (e1[2] * dv2 - e2[2] * dv1) * sg};
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]) && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]))) return FACE_REFUSED;
    if (!(det != 0.0) || det != det) return FACE_DEGENERATE;    // zero or NaN
    const double tl = norm3d(t), cl = norm3d(c);
    if (tl == 0.0 || cl == 0.0 || !isfinite(tl) || !isfinite(cl)) return FACE_DEGENERATE;
#pragma unroll
    for (int k = 0; k < 3; ++k) o->w[k] = (t[k] / tl) * cl;
    o->weight = cl;
    o->sign = det > 0.0 ? -1 : 1;
    return FACE_OK;
}

// the largest |c| of the contributing faces in *mx_bits (zeroed by the caller): non-negative doubles order as their bit patterns do
__global__ __launch_bounds__(THREADS) void tangent_max_kernel(const float* __restrict__ verts, int64_t V, const int* __restrict__ tris,
                                                              const float* __restrict__ vt, int64_t Vt, const int* __restrict__ ft, int64_t T,
                                                              u64* mx_bits) {
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    double m = 0.0;
    if (f < T) {
        FaceTangent ftg;
        if (face_tangent(verts, V, tris, vt, Vt, ft, f, &ftg) == FACE_OK) m = ftg.weight;
    }
    const u64 mx = wave_max((u64)__double_as_longlong(m));
    if ((threadIdx.x & 63) == 0 && mx != 0) atomicMax(mx_bits, mx);
}

// sums [Vt,3] int64 and info[0..1] zeroed by the caller
__global__ __launch_bounds__(THREADS) void tangent_add_kernel(const float* __restrict__ verts, int64_t V, const int* __restrict__ tris,
                                                              const float* __restrict__ vt, int64_t Vt, const int* __restrict__ ft, int64_t T, int B,
                                                              const u64* __restrict__ mx_bits, long long* sums, signed char* __restrict__ face_sign,
                                                              int64_t* info) {
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    int state = FACE_OK;
    if (f < T) {
        FaceTangent ftg;
        state = face_tangent(verts, V, tris, vt, Vt, ft, f, &ftg);
        face_sign[f] = (signed char)(state == FACE_OK ? ftg.sign : 0);
        if (state == FACE_OK) {
            int e = 0;
            (void)frexp(__longlong_as_double((long long)*mx_bits), &e);          // (a contributing face exists: mx > 0)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const long long q = llrint(ldexp(ftg.w[k], B - e));
                if (q != 0)
#pragma unroll
                    for (int c = 0; c < 3; ++c)                                   // j[c] < Vt: inside the sums
                        __hip_atomic_fetch_add(sums + 3 * (int64_t)ftg.j[c] + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    const int refused = __popcll(__ballot(state == FACE_REFUSED)), degenerate = __popcll(__ballot(state == FACE_DEGENERATE));
    if ((threadIdx.x & 63) == 0) {
        if (refused) atomicAdd((u64*)info, (u64)refused);
        if (degenerate) atomicAdd((u64*)(info + 1), (u64)degenerate);
    }
}

// behind the kernel boundary; info[2] zeroed by the caller
__global__ __launch_bounds__(THREADS) void tangent_finish_kernel(const long long* __restrict__ sums, int64_t Vt, const u64* __restrict__ mx_bits,
                                                                 float* __restrict__ tangent, int64_t* info) {
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    bool zero = false;
    if (v < Vt) {
        const long long s[3] = {sums[3 * v], sums[3 * v + 1], sums[3 * v + 2]};
        zero = s[0] == 0 && s[1] == 0 && s[2] == 0;
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (!zero) {
            const double d[3] = {(double)s[0], (double)s[1], (double)s[2]};
            const double l = norm3d(d);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = (float)(d[k] / l);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) tangent[3 * v + k] = out[k];
    }
    const int zeros = __popcll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd((u64*)(info + 2), (u64)zeros);
    if (v == 0) {
        int e = 0;
        const double mx = __longlong_as_double((long long)*mx_bits);
        if (mx > 0.0) (void)frexp(mx, &e);
        info[3] = e;
    }
}

// ---- the bytes of the map ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void nmap_encode_kernel(const float* __restrict__ nrm, const float* __restrict__ tan,
                                                              const signed char* __restrict__ sign, const float* __restrict__ ns,
                                                              const uint8_t* __restrict__ valid, const int* __restrict__ texel, int64_t n,
                                                              int64_t texels, int space, uint8_t* __restrict__ map, int64_t* invalid) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float N[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
        const float S[3] = {ns[3 * i], ns[3 * i + 1], ns[3 * i + 2]};
        float x[3] = {0.0f, 0.0f, 1.0f};                                        // the flat normal
        bool ok = valid[i] != 0 && finite3(S);
        if (space == SPACE_TANGENT) {
            const float T[3] = {tan[3 * i], tan[3 * i + 1], tan[3 * i + 2]};
            const Frame F = frame_of(N, T, (int)sign[i]);
            const float v[3] = {dot3(S, F.t), dot3(S, F.b), dot3(S, F.n)};
            float u[3];
            ok = unit3(v, u) && ok && F.ok && finite3(u);
            if (ok) x[0] = u[0], x[1] = u[1], x[2] = u[2];
        } else {
            float u[3];
            ok = unit3(S, u) && ok && finite3(u);
            if (ok) {
                x[0] = u[0], x[1] = u[1], x[2] = u[2];
            } else {
                float m[3];
                if (unit3(N, m) && finite3(m)) x[0] = m[0], x[1] = m[1], x[2] = m[2];
            }
        }
        bad = !ok;
        const int at = texel[i];
        if (at >= 0 && (int64_t)at < texels) {                                  // 3 at + 2 < 3 h w: inside the map
            uint8_t* o = map + 3 * (int64_t)at;
            o[0] = (uint8_t)nmap_byte(x[0]);
            o[1] = (uint8_t)nmap_byte(x[1]);
            o[2] = (uint8_t)nmap_byte(x[2]);
        }
    }
    const int bads = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0 && bads) atomicAdd((u64*)invalid, (u64)bads);
}

// ---- records and pyramid ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void nmap_pack_kernel(const uint8_t* __restrict__ map, int64_t n, uint32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t x = map[3 * i], y = map[3 * i + 1], z = map[3 * i + 2];
    out[i] = x | (y << 8) | (z << 16);
}

__device__ __forceinline__ uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int sh) {
    return (((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u) + 2u) >> 2;
}

// level k + 1 (ho x wo) from level k (2 ho x 2 wo): one lane per output record
__global__ __launch_bounds__(THREADS) void nmap_mip_kernel(const uint32_t* __restrict__ below, int ho, int wo, uint32_t* __restrict__ above) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (int64_t)ho * wo) return;
    const int y = (int)(i / wo), x = (int)(i - (int64_t)y * wo);
    const int64_t at = (int64_t)(2 * y) * (2 * wo) + 2 * x;                 // < (2 ho)(2 wo): the 2 x 2 block lies inside level k
    const uint32_t a = below[at], b = below[at + 1], c = below[at + 2 * wo], d = below[at + 2 * wo + 1];
    above[i] = mean4(a, b, c, d, 0) | (mean4(a, b, c, d, 8) << 8) | (mean4(a, b, c, d, 16) << 16);      // the fourth byte stays 0
}

// ---- the lookup -------------------------------------------------------------------------------------------------------------------------------
struct Vec3 {
    float x, y, z;
};

__device__ __forceinline__ Vec3 decode3(uint32_t q) {
    Vec3 v;
    v.x = nmap_decode(q & 255u);
    v.y = nmap_decode((q >> 8) & 255u);
    v.z = nmap_decode((q >> 16) & 255u);
    return v;
}

__device__ __forceinline__ Vec3 lerp3(const Vec3& p, const Vec3& q, float f) {
    Vec3 v;
    v.x = lerp(p.x, q.x, f);
    v.y = lerp(p.y, q.y, f);
    v.z = lerp(p.z, q.z, f);
    return v;
}

__device__ __forceinline__ Vec3 bilinear3(const uint32_t* __restrict__ pyr, const Plan& P, int k, float u, float v, Axis* ax, Axis* ay) {
    const Taps t = taps_of(P, k, u, v);                                     // every record number lies below P.records
    const Vec3 top = lerp3(decode3(pyr[t.r00]), decode3(pyr[t.r01]), t.ax.f);
    const Vec3 bot = lerp3(decode3(pyr[t.r10]), decode3(pyr[t.r11]), t.ax.f);
    *ax = t.ax;
    *ay = t.ay;
    return lerp3(top, bot, t.ay.f);
}

__global__ __launch_bounds__(THREADS) void nmap_apply_kernel(const uint32_t* __restrict__ pyr, Plan P, const float* __restrict__ vt, int64_t Vt,
                                                             const int* __restrict__ ft, int64_t T, const float* __restrict__ scale,
                                                             const float* __restrict__ tangent, const signed char* __restrict__ face_sign,
                                                             const int* __restrict__ face, const float* __restrict__ bary,
                                                             const float* __restrict__ depth, const float* __restrict__ nrm_in, int64_t n,
                                                             float spread, float lod_scale, int space, float* __restrict__ nrm_out,
                                                             float* __restrict__ dbg) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float N[3] = {nrm_in[3 * i], nrm_in[3 * i + 1], nrm_in[3 * i + 2]};
    float* o = nrm_out + 3 * i;
    const int f = face[i];
    int j0 = -1, j1 = -1, j2 = -1;
    if (in_range(f, T)) {
        j0 = ft[3 * (int64_t)f];
        j1 = ft[3 * (int64_t)f + 1];
        j2 = ft[3 * (int64_t)f + 2];
    }
    if (!(in_range(j0, Vt) && in_range(j1, Vt) && in_range(j2, Vt))) {
        o[0] = N[0], o[1] = N[1], o[2] = N[2];
        if (dbg)
#pragma unroll
            for (int j = 0; j < 8; ++j) dbg[8 * i + j] = 0.0f;
        return;
    }
    const float bu = bary[2 * i], bv = bary[2 * i + 1];
    float u, v;
    hit_uv(vt, j0, j1, j2, bu, bv, &u, &v);
    const Lod lod = lod_of(depth[i], spread, scale[f], lod_scale, P.L);
    Axis ax, ay, bx, by;
    Vec3 m = bilinear3(pyr, P, lod.l, u, v, &ax, &ay);
    if (lod.t != 0.0f) m = lerp3(m, bilinear3(pyr, P, lod.l + 1, u, v, &bx, &by), lod.t);      // l + 1 <= L - 1 where t != 0
    float r[3] = {m.x, m.y, m.z};
    bool ok = true;
    if (space == SPACE_TANGENT) {
        const float w0 = (1.0f - bu) - bv;
        float Tt[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Tt[k] = (w0 * tangent[3 * (int64_t)j0 + k] + bu * tangent[3 * (int64_t)j1 + k]) + bv * tangent[3 * (int64_t)j2 + k];
        const Frame F = frame_of(N, Tt, (int)face_sign[f]);
        ok = F.ok;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float zn = m.z * N[k];
            // no tilt: z N alone, so that (0, 0, 1) returns N bit for bit -- adding the zero tilt would turn a -0 of N into +0
            r[k] = (m.x == 0.0f && m.y == 0.0f) ? zn : ((m.x * F.t[k] + m.y * F.b[k]) * F.len) + zn;
        }
    }
    ok = ok && finite3(r) && !(r[0] == 0.0f && r[1] == 0.0f && r[2] == 0.0f) && dot3(r, N) > 0.0f;
    // (three selects on values: `ok ? r[k] : N[k]` in a loop became one select between the two arrays' addresses, and both went to scratch)
    const float o0 = ok ? r[0] : N[0], o1 = ok ? r[1] : N[1], o2 = ok ? r[2] : N[2];
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
    if (dbg) {
        float* d = dbg + 8 * i;
        d[0] = (float)lod.l;
        d[1] = lod.t;
        d[2] = (float)ax.i0;
        d[3] = (float)ay.i0;
        d[4] = ax.f;
        d[5] = ay.f;
        d[6] = u;
        d[7] = v;
    }
}

int refuse(const char* fn, const char* why) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", fn, why);
    return nero_fail(NERO_ERR_ARG, msg);
}

const char* const BAD_SIZE = "h and w must lie in [1, 16384]";
const char* const BAD_COUNT = "a count is negative or 2^31 - 1 or more";
const char* const BAD_PTR = "null pointer";
const char* const BAD_SPACE = "space must be 0 (tangent) or 1 (object)";
const char* const BAD_ALIGN = "the records are not 4-byte aligned";

}  // namespace

int nero_mesh_attr_at(const float* attr, int64_t V, int C, const int* tris, int64_t T, const int* face, const float* bary, int64_t n,
                      float fill, float* out, void* stream) {
    if (!channels_ok(C)) return refuse("nero_mesh_attr_at", "C must lie in [1, 8]");
    if (!count_ok(V) || !count_ok(T) || !count_ok(n)) return refuse("nero_mesh_attr_at", BAD_COUNT);
    if (n == 0) return NERO_OK;
    if (!face || !bary || !out || (V > 0 && !attr) || (T > 0 && !tris)) return refuse("nero_mesh_attr_at", BAD_PTR);
    hipLaunchKernelGGL(attr_at_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, attr, V, C, tris, T, face, bary, n, fill, out);
    return nero_check_launch("nero_mesh_attr_at");
}

size_t nero_uv_tangents_workspace_bytes(int64_t Vt, int64_t T) {
    if (!count_ok(Vt) || !count_ok(T)) return 0;
    return tangent_workspace_bytes(Vt);
}

int nero_uv_tangents(const float* verts, int64_t V, const int* tris, const float* vt, int64_t Vt, const int* ft, int64_t T, void* ws,
                     float* tangent, signed char* face_sign, int64_t* info, void* stream) {
    if (!count_ok(V) || !count_ok(Vt) || !count_ok(T)) return refuse("nero_uv_tangents", BAD_COUNT);
    if (T == 0 || Vt == 0) return NERO_OK;
    if (!tris || !vt || !ft || !ws || !tangent || !face_sign || !info || (V > 0 && !verts)) return refuse("nero_uv_tangents", BAD_PTR);
    if (!aligned(ws, 256)) return refuse("nero_uv_tangents", "the workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    u64* mx_bits = (u64*)b;
    long long* sums = (long long*)(b + nero_normals::HEAD_BYTES);
    // (the head and the sums are one run of bytes: one memset clears both)
    if (hipMemsetAsync(ws, 0, tangent_workspace_bytes(Vt), s) != hipSuccess || hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_uv_tangents: hipMemsetAsync failed");
    hipLaunchKernelGGL(tangent_max_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, verts, V, tris, vt, Vt, ft, T, mx_bits);
    if (int rc = nero_check_launch("nero_uv_tangents: max pass")) return rc;
    hipLaunchKernelGGL(tangent_add_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, verts, V, tris, vt, Vt, ft, T, tangent_term_bits(T),
                       (const u64*)mx_bits, sums, face_sign, info);
    if (int rc = nero_check_launch("nero_uv_tangents: add pass")) return rc;
    hipLaunchKernelGGL(tangent_finish_kernel, dim3(blocks_of(Vt)), dim3(THREADS), 0, s, (const long long*)sums, Vt, (const u64*)mx_bits, tangent,
                       info);
    return nero_check_launch("nero_uv_tangents: finish pass");
}

int nero_nmap_encode(const float* nrm, const float* tan, const signed char* sign, const float* ns, const unsigned char* valid,
                     const int* texel, int64_t n, int64_t h, int64_t w, int space, unsigned char* map, int64_t* invalid, void* stream) {
    if (!size_ok(h, w)) return refuse("nero_nmap_encode", BAD_SIZE);
    if (!count_ok(n)) return refuse("nero_nmap_encode", BAD_COUNT);
    if (!space_ok(space)) return refuse("nero_nmap_encode", BAD_SPACE);
    if (n == 0) return NERO_OK;
    if (!invalid || !nrm || !tan || !sign || !ns || !valid || !texel || !map) return refuse("nero_nmap_encode", BAD_PTR);
    if (hipMemsetAsync(invalid, 0, sizeof(int64_t), (hipStream_t)stream) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_nmap_encode: hipMemsetAsync failed");
    hipLaunchKernelGGL(nmap_encode_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, nrm, tan, sign, ns, valid, texel, n, h * w,
                       space, map, invalid);
    return nero_check_launch("nero_nmap_encode");
}

size_t nero_nmap_mip_bytes(int64_t h, int64_t w) { return nmap_bytes(h, w); }

int nero_nmap_pack(const unsigned char* map, int64_t h, int64_t w, unsigned char* out, void* stream) {
    if (!size_ok(h, w)) return refuse("nero_nmap_pack", BAD_SIZE);
    if (!map || !out) return refuse("nero_nmap_pack", BAD_PTR);
    if (!aligned(out, NMAP_RECORD_BYTES)) return refuse("nero_nmap_pack", BAD_ALIGN);
    const int64_t n = h * w;
    hipLaunchKernelGGL(nmap_pack_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, map, n, (uint32_t*)out);
    return nero_check_launch("nero_nmap_pack");
}

int nero_nmap_mip_build(unsigned char* pyramid, int64_t h, int64_t w, void* stream) {
    Plan P;
    if (!make_plan(h, w, &P)) return refuse("nero_nmap_mip_build", BAD_SIZE);
    if (!pyramid) return refuse("nero_nmap_mip_build", BAD_PTR);
    if (!aligned(pyramid, NMAP_RECORD_BYTES)) return refuse("nero_nmap_mip_build", BAD_ALIGN);
    uint32_t* rec = (uint32_t*)pyramid;
    for (int k = 1; k < P.L; ++k) {
        const int64_t n = (int64_t)P.h[k] * P.w[k];
        hipLaunchKernelGGL(nmap_mip_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, (const uint32_t*)(rec + P.off[k - 1]), P.h[k],
                           P.w[k], rec + P.off[k]);
        if (int rc = nero_check_launch("nero_nmap_mip_build")) return rc;
    }
    return NERO_OK;
}

int nero_nmap_apply(const unsigned char* pyramid, int64_t h, int64_t w, const float* vt, int64_t Vt, const int* ft, int64_t T,
                    const float* scale, const float* tangent, const signed char* face_sign, const int* face, const float* bary,
                    const float* depth, const float* nrm_in, int64_t n, float spread, float lod_scale, int space, float* nrm_out, float* dbg,
                    void* stream) {
    Plan P;
    if (!make_plan(h, w, &P)) return refuse("nero_nmap_apply", BAD_SIZE);
    if (!count_ok(Vt) || !count_ok(T) || !count_ok(n)) return refuse("nero_nmap_apply", BAD_COUNT);
    if (!(spread >= 0.0f) || !(lod_scale >= 0.0f)) return refuse("nero_nmap_apply", "spread and lod_scale must not be negative or NaN");
    if (!space_ok(space)) return refuse("nero_nmap_apply", BAD_SPACE);
    if (n == 0) return NERO_OK;
    if (!pyramid || !face || !bary || !depth || !nrm_in || !nrm_out || (Vt > 0 && (!vt || !tangent)) || (T > 0 && (!ft || !scale || !face_sign)))
        return refuse("nero_nmap_apply", BAD_PTR);
    if (!aligned(pyramid, NMAP_RECORD_BYTES)) return refuse("nero_nmap_apply", BAD_ALIGN);
    hipLaunchKernelGGL(nmap_apply_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, (const uint32_t*)pyramid, P, vt, Vt, ft, T,
                       scale, tangent, face_sign, face, bary, depth, nrm_in, n, spread, lod_scale, space, nrm_out, dbg);
    return nero_check_launch("nero_nmap_apply");
}
