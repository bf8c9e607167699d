// surface_sample.hip -- area-weighted sampling of points on a triangle mesh (include/nero_hip_surface.h): what the
// reference's eval.md leaves to CloudCompare between the mesh clean-up and eval_real_shape.py.
//   cdf      one pass over the triangles for the doubled areas and their maximum (an integer atomic max on the bit pattern of a
//            non-negative double: order-free), one pass that turns them into integer weights on the scale of that maximum, and hipCUB's
//            inclusive sum.  Integer addition is associative, so the running sum is the same bits however hipCUB partitions it -- a float
//            sum would not be -- and the search below needs no tolerance.
//   sample   one lane per sample: counter hashes of the global sample index, a binary search of the running sum, the square-root map of
//            the unit square onto the triangle.  A sample depends on its index alone, so every chunking of the range gives the same bits.
// The file is compiled without floating-point contraction and with correctly rounded square roots: every float64 operation is the IEEE
// operation the numpy restatement of the tests performs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/nero_hip_surface.h"
#include "common.h"
#include "cub_calls.h"
#include "device_prims.h"
#include "surface_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_cub;
using namespace nero_prims;
using namespace nero_surface;
using namespace nero_ws;

typedef unsigned long long u64;

// c = (p1 - p0) x (p2 - p0) of triangle t in float64 -> |c| (twice the area); false, and nothing read, when an index is out of range
__device__ __forceinline__ bool tri_cross(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t t, double* p,
                                          double* c, double* len) {
    const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
    if (!(in_range(i0, V) && in_range(i1, V) && in_range(i2, V))) return false;
    const int idx[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) p[3 * k + a] = (double)verts[3 * (int64_t)idx[k] + a];
    const double ux = p[3] - p[0], uy = p[4] - p[1], uz = p[5] - p[2];
    const double vx = p[6] - p[0], vy = p[7] - p[1], vz = p[8] - p[2];
    c[0] = uy * vz - uz * vy;
    c[1] = uz * vx - ux * vz;
    c[2] = ux * vy - uy * vx;
    *len = __dsqrt_rn((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    return true;
}

// a2[t], and the largest of them in *mx_bits (zeroed by the caller): non-negative doubles order as their bit patterns do
__global__ __launch_bounds__(THREADS) void surface_area_kernel(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t T,
                                                               double* __restrict__ a2, u64* mx_bits) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    double a = 0.0;
    if (t < T) {
        double p[9], c[3], len;
        if (tri_cross(verts, V, tris, t, p, c, &len) && isfinite(len)) a = len;
        a2[t] = a;
    }
    const u64 m = wave_max((u64)__double_as_longlong(a));          // (lanes past T hold +0)
    if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(mx_bits, m);
}

// w[t] = floor(a2[t] 2^(B - e)) over a2's own words; info = {., zero weights, e, B} (info[1] zeroed by the caller, info[0] after the scan)
__global__ __launch_bounds__(THREADS) void surface_weight_kernel(u64* __restrict__ w, int64_t T, const u64* __restrict__ mx_bits, int B,
                                                                 int64_t* info) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const double mx = __longlong_as_double((long long)*mx_bits);
    int e = 0;
    if (mx > 0.0) (void)frexp(mx, &e);
    bool zero = false;
    if (t < T) {
        const double a = __longlong_as_double((long long)w[t]);
        const u64 wt = mx > 0.0 ? (u64)floor(ldexp(a, B - e)) : 0ull;   // a <= mx < 2^e: below 2^B, exact
        w[t] = wt;
        zero = wt == 0;
    }
    const int zeros = __popcll(__ballot(zero));
    if ((threadIdx.x & 63) == 0 && zeros) atomicAdd((u64*)(info + 1), (u64)zeros);
    if (t == 0) {
        info[2] = e;
        info[3] = B;
    }
}

__global__ __launch_bounds__(THREADS) void surface_sample_kernel(const float* __restrict__ verts, int V, const int* __restrict__ tris, int64_t T,
                                                                 const int64_t* __restrict__ cdf, const int64_t* __restrict__ info, int64_t first,
                                                                 int64_t n, int64_t n_total, unsigned seed, int stratified,
                                                                 float* __restrict__ pts, int* __restrict__ face, float* __restrict__ bary,
                                                                 float* __restrict__ normal) {
    const int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (j >= n) return;
    const int64_t i = first + j;
    const u64 total = (u64)info[0];
    float out[3] = {0.0f, 0.0f, 0.0f}, bb[2] = {0.0f, 0.0f}, nn[3] = {0.0f, 0.0f, 0.0f};
    int f = -1;
    if (total > 0) {
        const unsigned h1 = lowbias32((unsigned)i * 0x9E3779B9u + seed), h2 = lowbias32(h1 + 0x68E31DA4u);
        const unsigned h3 = lowbias32(h2 + 0x68E31DA4u), h4 = lowbias32(h3 + 0x68E31DA4u);
        const double u = stratified ? ((double)i + (double)(h1 >> 8) * 0x1p-24) / (double)n_total
                                    : (double)(((u64)h1 << 21) | (u64)(h4 >> 11)) * 0x1p-53;
        u64 target = (u64)(u * (double)total);
        if (target > total - 1) target = total - 1;
        int64_t lo = 0, hi = T - 1;                                   // cdf[T - 1] = total > target: the answer lies in [lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((u64)cdf[mid] > target) hi = mid; else lo = mid + 1;
        }
        double p[9], c[3], len;
        // (a chosen triangle has a weight, hence indices in range and 0 < len < inf; a cdf of another mesh yields face -1 and zeros here)
        if (tri_cross(verts, V, tris, lo, p, c, &len) && len > 0.0 && isfinite(len)) {
            f = (int)lo;
            const double r1 = (double)(h2 >> 8) * 0x1p-24, r2 = (double)(h3 >> 8) * 0x1p-24;
            const double su = __dsqrt_rn(r1);
            const double b0 = 1.0 - su, b1 = su * (1.0 - r2), b2 = su * r2;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                out[a] = (float)((b0 * p[a] + b1 * p[3 + a]) + b2 * p[6 + a]);
                nn[a] = (float)(c[a] / len);
            }
            bb[0] = (float)b1;
            bb[1] = (float)b2;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) pts[3 * j + a] = out[a];
    if (face) face[j] = f;
    if (bary) {
        bary[2 * j] = bb[0];
        bary[2 * j + 1] = bb[1];
    }
    if (normal) {
#pragma unroll
        for (int a = 0; a < 3; ++a) normal[3 * j + a] = nn[a];
    }
}

// workspace: [HEAD_BYTES: the maximum's bit pattern][weights_bytes(T): a2, then w][hipCUB's scratch]
int cdf_layout(int64_t T, size_t* temp_bytes) {
    if (scan_temp<u64>(T, temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_surface_cdf: the scratch-size query of the weight scan failed");
    return NERO_OK;
}

}  // namespace

size_t nero_surface_cdf_workspace_bytes(int64_t T) {
    if (T < 1 || T > MAX_ITEMS) return no_workspace("nero_surface_cdf_workspace_bytes: T must be in [1, 2^31 - 2]");
    size_t temp = 0;
    if (cdf_layout(T, &temp) != NERO_OK) return 0;
    return HEAD_BYTES + weights_bytes(T) + temp;
}

int nero_surface_cdf(const float* verts, int64_t V, const int* tris, int64_t T, void* ws, int64_t* cdf, int64_t* info, void* stream) {
    if (!verts || !tris || !ws || !cdf || !info) return nero_fail(NERO_ERR_ARG, "nero_surface_cdf: null pointer");
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_ARG, "nero_surface_cdf: V and T must be in [1, 2^31 - 2]");
    if (((uintptr_t)ws & 255u) != 0) return nero_fail(NERO_ERR_ARG, "nero_surface_cdf: the workspace is not 256-byte aligned");
    size_t temp_bytes = 0;
    if (int rc = cdf_layout(T, &temp_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    u64* mx_bits = (u64*)b;
    u64* w = (u64*)(b + HEAD_BYTES);
    void* temp = b + HEAD_BYTES + weights_bytes(T);
    if (hipMemsetAsync(mx_bits, 0, sizeof(u64), s) != hipSuccess || hipMemsetAsync(info, 0, 4 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_surface_cdf: hipMemsetAsync failed");
    hipLaunchKernelGGL(surface_area_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, verts, (int)V, tris, T, (double*)w, mx_bits);
    if (int rc = nero_check_launch("nero_surface_cdf: area pass")) return rc;
    hipLaunchKernelGGL(surface_weight_kernel, dim3(blocks_of(T)), dim3(THREADS), 0, s, w, T, (const u64*)mx_bits, weight_bits(T), info);
    if (int rc = nero_check_launch("nero_surface_cdf: weight pass")) return rc;
    if (int rc = inclusive_sum(temp, temp_bytes, (const u64*)w, (u64*)cdf, T, s, "nero_surface_cdf: the weight scan failed"))
        return rc;
    if (hipMemcpyAsync(info, cdf + (T - 1), sizeof(int64_t), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_surface_cdf: the copy of the total failed");
    return NERO_OK;
}

int nero_surface_sample(const float* verts, int64_t V, const int* tris, int64_t T, const int64_t* cdf, const int64_t* info, int64_t first,
                        int64_t n, int64_t n_total, unsigned seed, int stratified, float* pts, int* face, float* bary, float* normal,
                        void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_ARG, "nero_surface_sample: V and T must be in [1, 2^31 - 2]");
    if (!range_ok(first, n, n_total))
        return nero_fail(NERO_ERR_ARG, "nero_surface_sample: 0 <= first, 0 <= n and first + n <= n_total <= 2^31 - 1 must hold");
    if (n == 0) return NERO_OK;
    if (!verts || !tris || !cdf || !info || !pts) return nero_fail(NERO_ERR_ARG, "nero_surface_sample: null pointer");
    hipLaunchKernelGGL(surface_sample_kernel, dim3(blocks_of(n)), dim3(THREADS), 0, (hipStream_t)stream, verts, (int)V, tris, T, cdf, info,
                       first, n, n_total, seed, stratified, pts, face, bary, normal);
    return nero_check_launch("nero_surface_sample");
}
