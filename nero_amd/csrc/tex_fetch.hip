// tex_fetch.hip -- mip-mapped UV material lookup for the relighter (include/nero_hip_texfetch.h): the texel records and
// their pyramid, the per-face texel density, the fused trilinear fetch at the hits and the per-vertex stand-in of the bounce kernels.
//   One lane owns one output (a texel, a face, a hit, a vertex).  A tap is one 8-byte load of a record; its five bytes are decoded through
//   the 256-entry table, which every workgroup stages in LDS first (one entry per thread).  Level sizes and offsets travel by value in a
//   Plan (tex_fetch_plan.h); a record is addressed as off[k] + y w_k + x with y and x clamped to the level, so no lane leaves the pyramid
//   whatever its coordinates are.  The level-of-detail rule and the addressing are tex_lod.h's, shared with detail_transfer.hip.
// The file is compiled without floating-point contraction: every fp32 operation is the one the numpy restatement of the tests performs
// (tests/texfetch_ref.py).  Wide LOADS only: all arithmetic is written per component (tests/test_no_packed_fp32.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip_texfetch.h"
#include "common.h"
#include "tex_fetch_plan.h"
#include "tex_lod.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_texfetch;

// ---- records and pyramid --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void tex_pack_kernel(const uint8_t* __restrict__ albedo, const uint8_t* __restrict__ metallic,
                                                           const uint8_t* __restrict__ roughness, int64_t n, uint2* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = albedo[3 * i], g = albedo[3 * i + 1], b = albedo[3 * i + 2], m = metallic[i], a = roughness[i];
    out[i] = make_uint2(r | (g << 8) | (b << 16) | (m << 24), a);
}

// byte j of the four words: (a + b + c + d + 2) >> 2
__device__ __forceinline__ uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, int j) {
    const int sh = 8 * j;
    return (((a >> sh) & 255u) + ((b >> sh) & 255u) + ((c >> sh) & 255u) + ((d >> sh) & 255u) + 2u) >> 2;
}

// level k + 1 (ho x wo) from level k (2 ho x 2 wo): one lane per output record
__global__ __launch_bounds__(THREADS) void tex_mip_kernel(const uint2* __restrict__ below, int ho, int wo, uint2* __restrict__ above) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= (int64_t)ho * wo) return;
    const int y = (int)(i / wo), x = (int)(i - (int64_t)y * wo);
    const int64_t at = (int64_t)(2 * y) * (2 * wo) + 2 * x;                 // < (2 ho)(2 wo): the 2 x 2 block lies inside level k
    const uint2 a = below[at], b = below[at + 1], c = below[at + 2 * wo], d = below[at + 2 * wo + 1];
    uint2 o;
    o.x = mean4(a.x, b.x, c.x, d.x, 0) | (mean4(a.x, b.x, c.x, d.x, 1) << 8) | (mean4(a.x, b.x, c.x, d.x, 2) << 16) |
          (mean4(a.x, b.x, c.x, d.x, 3) << 24);
    o.y = mean4(a.y, b.y, c.y, d.y, 0);                                     // the padding bytes stay 0
    above[i] = o;
}

// ---- per-face texel density -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void tex_face_scale_kernel(const float* __restrict__ verts, int64_t V, const int* __restrict__ tris,
                                                                 const float* __restrict__ vt, int64_t Vt, const int* __restrict__ ft, int64_t T,
                                                                 float wf, float hf, float* __restrict__ scale) {
    const int64_t f = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (f >= T) return;
    const int i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
    const int j0 = ft[3 * f], j1 = ft[3 * f + 1], j2 = ft[3 * f + 2];
    float out = 0.0f;
    if (in_range(i0, V) && in_range(i1, V) && in_range(i2, V) && in_range(j0, Vt) && in_range(j1, Vt) && in_range(j2, Vt)) {
        const float ax = (vt[2 * (int64_t)j1] - vt[2 * (int64_t)j0]) * wf, ay = (vt[2 * (int64_t)j1 + 1] - vt[2 * (int64_t)j0 + 1]) * hf;
        const float bx = (vt[2 * (int64_t)j2] - vt[2 * (int64_t)j0]) * wf, by = (vt[2 * (int64_t)j2 + 1] - vt[2 * (int64_t)j0 + 1]) * hf;
        const float a_uv = fabsf(ax * by - ay * bx);
        const float* p0 = verts + 3 * (int64_t)i0;
        const float* p1 = verts + 3 * (int64_t)i1;
        const float* p2 = verts + 3 * (int64_t)i2;
        const float ex = p1[0] - p0[0], ey = p1[1] - p0[1], ez = p1[2] - p0[2];
        const float gx = p2[0] - p0[0], gy = p2[1] - p0[1], gz = p2[2] - p0[2];
        const float cx = ey * gz - ez * gy, cy = ez * gx - ex * gz, cz = ex * gy - ey * gx;
        const float a_world = sqrtf((cx * cx + cy * cy) + cz * cz);
        if (a_uv != 0.0f && a_world != 0.0f) {                              // (a NaN area passes and is caught below)
            const float ratio = a_uv / a_world;
            if (isfinite(ratio)) out = sqrtf(ratio);
        }
    }
    scale[f] = out;
}

// ---- the fetch ------------------------------------------------------------------------------------------------------------------------------
struct Texel5 {
    float r, g, b, m, a;                                                    // albedo, metallic, the roughness channel (alpha)
};

__device__ __forceinline__ Texel5 decode(const uint2 q, const float* lut) {
    Texel5 t;
    t.r = lut[q.x & 255u];
    t.g = lut[(q.x >> 8) & 255u];
    t.b = lut[(q.x >> 16) & 255u];
    t.m = lut[q.x >> 24];
    t.a = lut[q.y & 255u];
    return t;
}

__device__ __forceinline__ Texel5 lerp5(const Texel5& p, const Texel5& q, float f) {
    Texel5 t;
    t.r = lerp(p.r, q.r, f);
    t.g = lerp(p.g, q.g, f);
    t.b = lerp(p.b, q.b, f);
    t.m = lerp(p.m, q.m, f);
    t.a = lerp(p.a, q.a, f);
    return t;
}

// the bilinear fetch in level k (addresses: tex_lod.h); ax and ay (of that level) are returned for dbg
__device__ __forceinline__ Texel5 bilinear(const uint2* __restrict__ pyr, const Plan& P, int k, float u, float v, const float* lut, Axis* ax_out,
                                           Axis* ay_out) {
    const Taps t = taps_of(P, k, u, v);                                     // every record number lies below P.records
    const uint2 q00 = pyr[t.r00], q01 = pyr[t.r01], q10 = pyr[t.r10], q11 = pyr[t.r11];
    const Texel5 top = lerp5(decode(q00, lut), decode(q01, lut), t.ax.f);
    const Texel5 bot = lerp5(decode(q10, lut), decode(q11, lut), t.ax.f);
    *ax_out = t.ax;
    *ay_out = t.ay;
    return lerp5(top, bot, t.ay.f);
}

__device__ __forceinline__ void stage_lut(float* l_lut, const float* __restrict__ lut) {
    l_lut[threadIdx.x] = lut[threadIdx.x];                                  // THREADS == 256 entries
    __syncthreads();
}

__device__ __forceinline__ void write5(float* __restrict__ out, const Texel5& t) {
    out[0] = t.m;
    out[1] = sqrtf(t.a);
    out[2] = t.r;
    out[3] = t.g;
    out[4] = t.b;
}

__device__ __forceinline__ void zero5(float* __restrict__ out) {
#pragma unroll
    for (int j = 0; j < 5; ++j) out[j] = 0.0f;
}

__global__ __launch_bounds__(THREADS) void tex_materials_kernel(const uint2* __restrict__ pyr, Plan P, const float* __restrict__ lut,
                                                                const float* __restrict__ vt, int64_t Vt, const int* __restrict__ ft, int64_t T,
                                                                const float* __restrict__ scale, const int* __restrict__ face,
                                                                const float* __restrict__ bary, const float* __restrict__ depth, int64_t n,
                                                                float spread, float lod_scale, float* __restrict__ mat5, float* __restrict__ dbg) {
    __shared__ float l_lut[256];
    static_assert(THREADS == 256, "one thread stages one entry of the table");
    stage_lut(l_lut, lut);
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int f = face[i];
    int j0 = -1, j1 = -1, j2 = -1;
    if (in_range(f, T)) {
        j0 = ft[3 * (int64_t)f];
        j1 = ft[3 * (int64_t)f + 1];
        j2 = ft[3 * (int64_t)f + 2];
    }
    if (!(in_range(j0, Vt) && in_range(j1, Vt) && in_range(j2, Vt))) {
        zero5(mat5 + 5 * i);
        if (dbg)
#pragma unroll
            for (int j = 0; j < 8; ++j) dbg[8 * i + j] = 0.0f;
        return;
    }
    float u, v;
    hit_uv(vt, j0, j1, j2, bary[2 * i], bary[2 * i + 1], &u, &v);
    const Lod lod = lod_of(depth[i], spread, scale[f], lod_scale, P.L);
    const int l = lod.l;
    const float t = lod.t;
    Axis ax, ay, bx, by;
    Texel5 m = bilinear(pyr, P, l, u, v, l_lut, &ax, &ay);
    if (t != 0.0f) m = lerp5(m, bilinear(pyr, P, l + 1, u, v, l_lut, &bx, &by), t);   // l + 1 <= L - 1 where t != 0
    write5(mat5 + 5 * i, m);
    if (dbg) {
        float* d = dbg + 8 * i;
        d[0] = (float)l;
        d[1] = t;
        d[2] = (float)ax.i0;
        d[3] = (float)ay.i0;
        d[4] = ax.f;
        d[5] = ay.f;
        d[6] = u;
        d[7] = v;
    }
}

// ---- the per-vertex stand-in ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void tex_owner_fill_kernel(int* __restrict__ owner, int64_t V) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i < V) owner[i] = NO_OWNER;
}

__global__ __launch_bounds__(THREADS) void tex_owner_min_kernel(const int* __restrict__ tris, int64_t corners, int64_t V, int* __restrict__ owner) {
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= corners) return;
    const int i = tris[c];
    if (in_range(i, V)) atomicMin(owner + i, (int)c);                       // an integer minimum: the same whatever the arrival order
}

__global__ __launch_bounds__(THREADS) void tex_vertex_kernel(const uint2* __restrict__ pyr, Plan P, const float* __restrict__ lut,
                                                             const float* __restrict__ vt, int64_t Vt, const int* __restrict__ ft, int64_t corners,
                                                             const int* __restrict__ owner, int64_t V, float* __restrict__ mat5_v) {
    __shared__ float l_lut[256];
    stage_lut(l_lut, lut);
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= V) return;
    const int c = owner[i];
    const int j = (c >= 0 && (int64_t)c < corners) ? ft[c] : -1;            // NO_OWNER >= corners
    if (!in_range(j, Vt)) {
        zero5(mat5_v + 5 * i);
        return;
    }
    Axis ax, ay;
    write5(mat5_v + 5 * i, bilinear(pyr, P, 0, vt[2 * (int64_t)j], vt[2 * (int64_t)j + 1], l_lut, &ax, &ay));
}

int refuse(const char* fn, const char* why) {
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", fn, why);
    return nero_fail(NERO_ERR_ARG, msg);
}

const char* const BAD_SIZE = "h and w must lie in [1, 16384]";
const char* const BAD_COUNT = "a count is negative or 2^31 - 1 or more";
const char* const BAD_PTR = "null pointer";
const char* const BAD_ALIGN = "the records are not 8-byte aligned";

}  // namespace

int nero_tex_mip_levels(int64_t h, int64_t w) { return levels(h, w); }

size_t nero_tex_mip_bytes(int64_t h, int64_t w) { return pyramid_bytes(h, w); }

int nero_tex_pack(const unsigned char* albedo, const unsigned char* metallic, const unsigned char* roughness, int64_t h, int64_t w,
                  unsigned char* out, void* stream) {
    if (!size_ok(h, w)) return refuse("nero_tex_pack", BAD_SIZE);
    if (!albedo || !metallic || !roughness || !out) return refuse("nero_tex_pack", BAD_PTR);
    if (!aligned(out, RECORD_BYTES)) return refuse("nero_tex_pack", BAD_ALIGN);
    const int64_t n = h * w;
    hipLaunchKernelGGL(tex_pack_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, albedo, metallic, roughness, n, (uint2*)out);
    return nero_check_launch("nero_tex_pack");
}

int nero_tex_mip_build(unsigned char* pyramid, int64_t h, int64_t w, void* stream) {
    Plan P;
    if (!make_plan(h, w, &P)) return refuse("nero_tex_mip_build", BAD_SIZE);
    if (!pyramid) return refuse("nero_tex_mip_build", BAD_PTR);
    if (!aligned(pyramid, RECORD_BYTES)) return refuse("nero_tex_mip_build", BAD_ALIGN);
    uint2* rec = (uint2*)pyramid;
    for (int k = 1; k < P.L; ++k) {
        const int64_t n = (int64_t)P.h[k] * P.w[k];
        hipLaunchKernelGGL(tex_mip_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, (const uint2*)(rec + P.off[k - 1]), P.h[k],
                           P.w[k], rec + P.off[k]);
        if (int rc = nero_check_launch("nero_tex_mip_build")) return rc;
    }
    return NERO_OK;
}

int nero_tex_face_scale(const float* verts, int64_t V, const int* tris, const float* vt, int64_t Vt, const int* ft, int64_t T, int64_t h,
                        int64_t w, float* scale, void* stream) {
    if (!size_ok(h, w)) return refuse("nero_tex_face_scale", BAD_SIZE);
    if (!count_ok(V) || !count_ok(Vt) || !count_ok(T)) return refuse("nero_tex_face_scale", BAD_COUNT);
    if (T == 0) return NERO_OK;
    if (!tris || !ft || !scale || (V > 0 && !verts) || (Vt > 0 && !vt)) return refuse("nero_tex_face_scale", BAD_PTR);
    hipLaunchKernelGGL(tex_face_scale_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, (hipStream_t)stream, verts, V, tris, vt, Vt, ft, T, (float)w,
                       (float)h, scale);
    return nero_check_launch("nero_tex_face_scale");
}

int nero_tex_materials(const unsigned char* pyramid, int64_t h, int64_t w, const float* lut, const float* vt, int64_t Vt, const int* ft,
                       int64_t T, const float* scale, const int* face, const float* bary, const float* depth, int64_t n, float spread,
                       float lod_scale, float* mat5, float* dbg, void* stream) {
    Plan P;
    if (!make_plan(h, w, &P)) return refuse("nero_tex_materials", BAD_SIZE);
    if (!count_ok(Vt) || !count_ok(T) || !count_ok(n)) return refuse("nero_tex_materials", BAD_COUNT);
    if (!(spread >= 0.0f) || !(lod_scale >= 0.0f)) return refuse("nero_tex_materials", "spread and lod_scale must not be negative or NaN");
    if (n == 0) return NERO_OK;
    if (!pyramid || !lut || !face || !bary || !depth || !mat5 || (Vt > 0 && !vt) || (T > 0 && (!ft || !scale)))
        return refuse("nero_tex_materials", BAD_PTR);
    if (!aligned(pyramid, RECORD_BYTES)) return refuse("nero_tex_materials", BAD_ALIGN);
    hipLaunchKernelGGL(tex_materials_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, (const uint2*)pyramid, P, lut, vt, Vt, ft, T,
                       scale, face, bary, depth, n, spread, lod_scale, mat5, dbg);
    return nero_check_launch("nero_tex_materials");
}

int nero_tex_vertex_materials(const unsigned char* pyramid, int64_t h, int64_t w, const float* lut, const float* vt, int64_t Vt,
                              const int* tris, const int* ft, int64_t T, int64_t V, int* owner_ws, float* mat5_v, void* stream) {
    Plan P;
    if (!make_plan(h, w, &P)) return refuse("nero_tex_vertex_materials", BAD_SIZE);
    if (!count_ok(Vt) || !count_ok(V)) return refuse("nero_tex_vertex_materials", BAD_COUNT);
    if (!corners_ok(T)) return refuse("nero_tex_vertex_materials", "T is negative or (2^31 - 1) / 3 or more");
    if (V == 0) return NERO_OK;
    if (!pyramid || !lut || !owner_ws || !mat5_v || (Vt > 0 && !vt) || (T > 0 && (!tris || !ft))) return refuse("nero_tex_vertex_materials", BAD_PTR);
    if (!aligned(pyramid, RECORD_BYTES)) return refuse("nero_tex_vertex_materials", BAD_ALIGN);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tex_owner_fill_kernel, dim3(blocks_of(V)), dim3(THREADS), 0, s, owner_ws, V);
    if (int rc = nero_check_launch("nero_tex_vertex_materials: fill")) return rc;
    if (T > 0) {
        hipLaunchKernelGGL(tex_owner_min_kernel, dim3(blocks_of(3 * T)), dim3(THREADS), 0, s, tris, 3 * T, V, owner_ws);
        if (int rc = nero_check_launch("nero_tex_vertex_materials: owners")) return rc;
    }
    hipLaunchKernelGGL(tex_vertex_kernel, dim3(blocks_of(V)), dim3(THREADS), 0, s, (const uint2*)pyramid, P, lut, vt, Vt, ft, 3 * T, (const int*)owner_ws,
                       V, mat5_v);
    return nero_check_launch("nero_tex_vertex_materials");
}
