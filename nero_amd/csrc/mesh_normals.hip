// mesh_normals.hip -- smooth per-vertex normals of a triangle mesh (include/nero_hip_normals.h): the weighted sum of the
// normals of the faces around each vertex, by area or by the angle at the vertex.
//   max      area mode only: one pass over the faces for the largest |c_k| (an integer atomic max on the bit pattern of a non-negative
//            double: order-free), which fixes the scale of the fixed-point terms.
//   add      one lane per face: its three corners add their terms, as INTEGERS, to the three int64 sums of their vertices with agent-scope
//            atomic adds.  Integer addition is associative, so the sums are the same bits in whatever order the adds land -- a float sum
//            would not be.
//   finish   one lane per vertex, behind the kernel boundary (the XCDs' L2 caches are not coherent inside a launch): the sums as float64,
//            normalised, stored as fp32.
// The file is compiled without floating-point contraction and with correctly rounded square roots: every float64 operation is the IEEE
// operation the numpy restatement of the tests performs (atan2 excepted: the angle mode agrees up to its last places).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nero_hip_normals.h"
#include "common.h"
#include "device_prims.h"
#include "normals_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_normals;
using namespace nero_prims;
using namespace nero_ws;

typedef unsigned long long u64;

enum { FACE_OK = 0, FACE_REFUSED = 1, FACE_DEGENERATE = 2 };

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double norm3(const double* c) { return __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]); }

// corners p [3][3] and c = (p1 - p0) x (p2 - p0) of face t in float64; nothing is read through an index out of range
__device__ __forceinline__ int face_cross(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t t, int* idx, double* p,
                                          double* c) {
    idx[0] = tris[3 * t], idx[1] = tris[3 * t + 1], idx[2] = tris[3 * t + 2];
    if (!(in_range(idx[0], V) && in_range(idx[1], V) && in_range(idx[2], V))) return FACE_REFUSED;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[3 * k + a] = (double)verts[3 * (int64_t)idx[k] + a];
    const double u[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, w[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    cross3(u, w, c);
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) return FACE_REFUSED;
    return c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0 ? FACE_DEGENERATE : FACE_OK;
}

// the largest |c_k| of the accepted faces in *mx_bits (zeroed by the caller): non-negative doubles order as their bit patterns do
__global__ __launch_bounds__(THREADS) void normals_max_kernel(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t T,
                                                              u64* mx_bits) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    double m = 0.0;
    if (t < T) {
        int idx[3];
        double p[9], c[3];
        if (face_cross(verts, V, tris, t, idx, p, c) == FACE_OK) m = fmax(fmax(fabs(c[0]), fabs(c[1])), fabs(c[2]));
    }
    const u64 mx = wave_max((u64)__double_as_longlong(m));            // (lanes past T, refused and degenerate faces hold +0)
    if ((threadIdx.x & 63) == 0 && mx != 0) atomicMax(mx_bits, mx);
}

// sums [V,3] int64 and info[0..1] zeroed by the caller; B = term_bits(T, weight)
__global__ __launch_bounds__(THREADS) void normals_add_kernel(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t T,
                                                              int weight, int B, const u64* __restrict__ mx_bits, long long* sums,
                                                              int64_t* info) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    int state = FACE_OK;
    if (t < T) {
        int idx[3];
        double p[9], c[3];
        state = face_cross(verts, V, tris, t, idx, p, c);
        if (state == FACE_OK) {
            double term[3][3];                                        // [corner][component], before the fixed-point scale
            int shift = B;
            if (weight == WEIGHT_AREA) {
                int e = 0;
                (void)frexp(__longlong_as_double((long long)*mx_bits), &e);      // (an accepted face exists: mx > 0)
                shift = B - e;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = 0; k < 3; ++k) term[i][k] = c[k];
            } else {
                const double len = norm3(c);
                const double n[3] = {c[0] / len, c[1] / len, c[2] / len};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double* o = p + 3 * i;
                    const double* p1 = p + 3 * ((i + 1) % 3);
                    const double* p2 = p + 3 * ((i + 2) % 3);
                    const double a[3] = {p1[0] - o[0], p1[1] - o[1], p1[2] - o[2]}, b[3] = {p2[0] - o[0], p2[1] - o[1], p2[2] - o[2]};
                    double x[3];
                    cross3(a, b, x);
                    const double theta = atan2(norm3(x), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]);
#pragma unroll
                    for (int k = 0; k < 3; ++k) term[i][k] = theta * n[k];
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const long long q = llrint(ldexp(term[i][k], shift));
                    if (q != 0) __hip_atomic_fetch_add(sums + 3 * (int64_t)idx[i] + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
        }
    }
    const int refused = __popcll(__ballot(state == FACE_REFUSED)), degenerate = __popcll(__ballot(state == FACE_DEGENERATE));
    if ((threadIdx.x & 63) == 0) {
        if (refused) atomicAdd((u64*)info, (u64)refused);
        if (degenerate) atomicAdd((u64*)(info + 1), (u64)degenerate);
    }
}

// info[2] zeroed by the caller; info[3] = e (area mode), 0 (angle mode)
__global__ __launch_bounds__(THREADS) void normals_finish_kernel(const long long* __restrict__ sums, int64_t V, int weight,
                                                                 const u64* __restrict__ mx_bits, float* __restrict__ normals, int64_t* info) {
    const int64_t v = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    bool zero = false;
    if (v < V) {
        const long long s[3] = {sums[3 * v], sums[3 * v + 1], sums[3 * v + 2]};
        zero = s[0] == 0 && s[1] == 0 && s[2] == 0;
        float out[3] = {0.0f, 0.0f, 0.0f};
        if (!zero) {
            const double d[3] = {(double)s[0], (double)s[1], (double)s[2]};
            const double l = norm3(d);
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = (float)(d[k] / l);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) normals[3 * v + k] = out[k];
    }
    const int zeros = __popcll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd((u64*)(info + 2), (u64)zeros);
    if (v == 0) {
        int e = 0;
        const double mx = __longlong_as_double((long long)*mx_bits);
        if (weight == WEIGHT_AREA && mx > 0.0) (void)frexp(mx, &e);
        info[3] = e;
    }
}

}  // namespace

size_t nero_vertex_normals_workspace_bytes(int64_t V, int64_t T) {
    if (!sizes_ok(V, T)) {
        nero_fail(NERO_ERR_UNSUPPORTED, "nero_vertex_normals_workspace_bytes: V and T must be in [1, 2^31 - 2]");
        return 0;
    }
    return workspace_bytes(V);
}

int nero_vertex_normals(const float* verts, int64_t V, const int* tris, int64_t T, int weight, void* ws, float* normals, int64_t* info,
                        void* stream) {
    if (!verts || !tris || !ws || !normals || !info) return nero_fail(NERO_ERR_ARG, "nero_vertex_normals: null pointer");
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_ARG, "nero_vertex_normals: V and T must be in [1, 2^31 - 2]");
    if (!weight_ok(weight)) return nero_fail(NERO_ERR_ARG, "nero_vertex_normals: weight must be 0 (area) or 1 (angle)");
    if (((uintptr_t)ws & 255u) != 0) return nero_fail(NERO_ERR_ARG, "nero_vertex_normals: the workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    u64* mx_bits = (u64*)b;
    long long* sums = (long long*)(b + HEAD_BYTES);
    // (the head and the sums are one run of bytes: one memset clears both)
    if (hipMemsetAsync(ws, 0, workspace_bytes(V), s) != hipSuccess || hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_vertex_normals: hipMemsetAsync failed");
    if (weight == WEIGHT_AREA) {
        hipLaunchKernelGGL(normals_max_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, verts, (int)V, tris, T, mx_bits);
        if (int rc = nero_check_launch("nero_vertex_normals: max pass")) return rc;
    }
    hipLaunchKernelGGL(normals_add_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, verts, (int)V, tris, T, weight, term_bits(T, weight),
                       (const u64*)mx_bits, sums, info);
    if (int rc = nero_check_launch("nero_vertex_normals: add pass")) return rc;
    hipLaunchKernelGGL(normals_finish_kernel, dim3(blocks_of(V)), dim3(THREADS), 0, s, (const long long*)sums, V, weight, (const u64*)mx_bits,
                       normals, info);
    return nero_check_launch("nero_vertex_normals: finish pass");
}
