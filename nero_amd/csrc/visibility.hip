// visibility.hip -- shadow-ray queries on the mesh tracer's BVH, and ambient occlusion on top of them (include/nero_hip_visibility.h).
//   * nero_bvh_occluded: is any triangle in the way within tmax?  The any-hit expansions of the two walks of bvh_walk.h: the same
//     visits in the same order with the same box and triangle arithmetic as nero_bvh_trace, ended at the first accepted triangle.
//   * nero_ao_rays: the AO sample set -- a per-texel Cranley-Patterson rotation of a (regular, radical-inverse) point set, mapped to the
//     cosine-weighted hemisphere around the normal.  ao_ray() below IS the definition; tests/ao_ref.py restates it in numpy.
//   * nero_bvh_ao: the same rays from the same function, cast through the any-hit walk without ever being stored; a wavefront's occluded
//     rays are counted by ballot and popcount.
#include <hip/hip_runtime.h>
#include "../../include/nero_hip.h"
#include "../../include/nero_hip_visibility.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "device_prims.h"
#include "visibility_plan.h"

namespace {

using namespace nero_bvh;
using nero_prims::lowbias32;
using namespace nero_vis;               // samples_ok, total_ok, log2_of, grid_blocks (visibility_plan.h)
constexpr float MISS_DEPTH = 10.0f;        // the tracer's miss distance: no query looks further
constexpr int PRIV_THREADS = 256;          // workgroup of the private-stack kernels (as trace_kernel)

// a per-ray tmax is clamped to [0, MISS_DEPTH]; 0 (and anything below) accepts no triangle, NaN is taken for MISS_DEPTH
__device__ __forceinline__ float clamp_tmax(float t) { return fmaxf(fminf(t, MISS_DEPTH), 0.f); }

// bool HIT = does the ray (o, d) meet a triangle nearer than TMAX, starting at CUR0 (NONE: not traversed): the any-hit expansion of the
// walk that the kernel's OVERLAP selects.  In scope: nodes, tris, o, d, st.
#define NERO_ANY_HIT(HIT, TMAX, CUR0)                                        \
    bool HIT;                                                                \
    {                                                                        \
        float inv[3];                                                        \
        ray_inverse(d, inv);                                                 \
        if constexpr (OVERLAP) {                                             \
            NERO_WALK_OVERLAP(true, TMAX, CUR0)                              \
            HIT = best >= 0;                                                 \
        } else {                                                             \
            NERO_WALK_PRIVATE(true, TMAX, CUR0)                              \
            HIT = best >= 0;                                                 \
        }                                                                    \
    }

// OVERLAP: PL_THREADS threads and the LDS stack (trees no deeper than PL_STACK), else PRIV_THREADS threads and the private stack
template <bool OVERLAP>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void occluded_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, int root, const float* __restrict__ ro, const float* __restrict__ rd, int n,
    const float* __restrict__ tmax, float tmax_all, const unsigned char* __restrict__ skip, unsigned char* __restrict__ occluded) {
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const float o[3] = {ro[r * 3], ro[r * 3 + 1], ro[r * 3 + 2]};
    const float d[3] = {rd[r * 3], rd[r * 3 + 1], rd[r * 3 + 2]};
    const float t = tmax != nullptr ? clamp_tmax(tmax[r]) : tmax_all;
    NERO_ANY_HIT(hit, t, (skip != nullptr && skip[r] != 0) ? NONE : root)                 // a skipped ray reports 0 without a node visit
    occluded[r] = hit ? 1 : 0;
}

// ---- the AO sample set --------------------------------------------------------------------------------------------------------------------
// Ray s of S of the point p with unit normal n and hash key `key`: origin o = p + bias n, direction d cosine-distributed around n.
// Integer-exact up to the square roots and the sine / cosine: (s + 0.5) / S and bitreverse(s) 2^-32 are exact in fp32 for S <= 1024, the
// two rotations r1, r2 are 24-bit fractions, and each of a, b is ONE fp32 add and one x - floorf(x).  Every product and sum below is
// rounded on its own (contraction off), in the order written.
__device__ __forceinline__ void ao_ray(const float* p, const float* n, unsigned key, unsigned s, int S, unsigned seed, float bias, float* o,
                                       float* d) {
#pragma clang fp contract(off)
    const unsigned h1 = lowbias32(key * 0x9E3779B9u + seed), h2 = lowbias32(h1 + 0x68E31DA4u);
    const float r1 = (float)(h1 >> 8) * 0x1p-24f, r2 = (float)(h2 >> 8) * 0x1p-24f;
    float a = ((float)s + 0.5f) / (float)S + r1;
    a = a - floorf(a);
    float b = (float)__brev(s) * 0x1p-32f + r2;
    b = b - floorf(b);
    const float phi = 6.283185307179586f * b;
    float sn, cs;
    sincosf(phi, &sn, &cs);
    const float ra = sqrtf(a);
    const float x = ra * cs, y = ra * sn, z = sqrtf(1.0f - a);
    // the frame of Duff et al., "Building an Orthonormal Basis, Revisited" (JCGT 2017), branchless
    const float sg = copysignf(1.0f, n[2]);
    const float c0 = -1.0f / (sg + n[2]);
    const float c1 = n[0] * n[1] * c0;
    const float t[3] = {1.0f + sg * n[0] * n[0] * c0, sg * c1, -sg * n[0]};
    const float u[3] = {c1, sg + n[1] * n[1] * c0, -n[1]};
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x * t[k] + y * u[k] + z * n[k];
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = v[k] / len;
        o[k] = p[k] + bias * n[k];
    }
}

__global__ __launch_bounds__(256) void ao_rays_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, const int* __restrict__ key,
                                                      int total, int log2S, unsigned seed, float bias, float* __restrict__ ro,
                                                      float* __restrict__ rd) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // ray j S + s
    if (g >= total) return;
    const int j = g >> log2S, S = 1 << log2S;
    const float p[3] = {pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2]};
    const float n[3] = {nrm[j * 3], nrm[j * 3 + 1], nrm[j * 3 + 2]};
    float o[3], d[3];
    ao_ray(p, n, (unsigned)key[j], (unsigned)(g & (S - 1)), S, seed, bias, o, d);
    const size_t at = (size_t)g * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ro[at + k] = o[k]; rd[at + k] = d[k]; }
}

// One ray per lane, sample index fastest.  S >= 64: the 64 rays of a wavefront belong to one point -- one integer atomic add of the
// ballot's popcount per wavefront into count[j] (zeroed by the caller; integer sums do not depend on their order).  S < 64: a wavefront
// holds 64 / S whole points, and the first lane of each stores the popcount of its S bits of the ballot.
template <bool OVERLAP>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void ao_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, int root, const float* __restrict__ pts, const float* __restrict__ nrm,
    const int* __restrict__ key, int total, int log2S, unsigned seed, float bias, float tmax, int* __restrict__ count) {
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // ray j S + s; total is a multiple of min(S, 64): a point's group of
    const bool live = g < total;                                       // lanes is live or dead as a whole
    const int j = g >> log2S, S = 1 << log2S;
    bool hit = false;
    if (live) {
        const float p[3] = {pts[j * 3], pts[j * 3 + 1], pts[j * 3 + 2]};
        const float n[3] = {nrm[j * 3], nrm[j * 3 + 1], nrm[j * 3 + 2]};
        float o[3], d[3];
        ao_ray(p, n, (unsigned)key[j], (unsigned)(g & (S - 1)), S, seed, bias, o, d);
        NERO_ANY_HIT(blocked, tmax, root)
        hit = blocked;
    }
    const unsigned long long votes = __ballot(hit);
    const int lane = threadIdx.x & 63;
    if (!live) return;
    if (log2S >= 6) {
        if (lane == 0) atomicAdd(count + j, __popcll(votes));
    } else if ((lane & (S - 1)) == 0) {
        count[j] = __popcll((votes >> lane) & ((1ull << S) - 1ull));
    }
}

int check_samples(int n, int S) {
    if (n < 0) return nero_fail(NERO_ERR_ARG, "ambient occlusion: n must be >= 0");
    if (!samples_ok(S)) return nero_fail(NERO_ERR_ARG, "ambient occlusion: S must be a power of two in [8, 1024]");
    if (!total_ok(n, S)) return nero_fail(NERO_ERR_ARG, "ambient occlusion: n * S must be at most 2^31 - 64: call in chunks");
    return NERO_OK;
}

}  // namespace

extern "C" {

int nero_bvh_occluded(void* handle, const float* rays_o, const float* rays_d, int n, const float* tmax, float tmax_all,
                      const unsigned char* skip, unsigned char* occluded, void* stream) {
    if (!handle || !rays_o || !rays_d || !occluded || n < 0) return nero_fail(NERO_ERR_ARG, "nero_bvh_occluded: bad argument");
    if (!(tmax_all > 0.f && tmax_all <= MISS_DEPTH)) return nero_fail(NERO_ERR_ARG, "nero_bvh_occluded: tmax_all must lie in (0, 10]");
    if ((long long)n > 2147483647ll / 3) return nero_fail(NERO_ERR_ARG, "nero_bvh_occluded: more than (2^31 - 1) / 3 rays: call in chunks");
    if (n == 0) return NERO_OK;
    Handle* h = (Handle*)handle;
    if (h->mode == 0)
        hipLaunchKernelGGL(occluded_kernel<false>, dim3(grid_blocks(n, PRIV_THREADS)), dim3(PRIV_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, rays_o, rays_d, n, tmax, tmax_all, skip, occluded);
    else
        hipLaunchKernelGGL(occluded_kernel<true>, dim3(grid_blocks(n, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, rays_o, rays_d, n, tmax, tmax_all, skip, occluded);
    return nero_check_launch("nero_bvh_occluded");
}

int nero_ao_rays(const float* pts, const float* nrm, const int* key, int n, int S, unsigned seed, float bias, float* rays_o, float* rays_d,
                 void* stream) {
    if (!pts || !nrm || !key || !rays_o || !rays_d) return nero_fail(NERO_ERR_ARG, "nero_ao_rays: null pointer");
    if (check_samples(n, S) != NERO_OK) return NERO_ERR_ARG;
    if (n == 0) return NERO_OK;
    const int total = n * S;
    hipLaunchKernelGGL(ao_rays_kernel, dim3(grid_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, pts, nrm, key, total, log2_of(S), seed, bias,
                       rays_o, rays_d);
    return nero_check_launch("nero_ao_rays");
}

int nero_bvh_ao(void* handle, const float* pts, const float* nrm, const int* key, int n, int S, unsigned seed, float bias, float tmax,
                int* count, void* stream) {
    if (!handle || !pts || !nrm || !key || !count) return nero_fail(NERO_ERR_ARG, "nero_bvh_ao: null handle or pointer");
    if (!(tmax > 0.f && tmax <= MISS_DEPTH)) return nero_fail(NERO_ERR_ARG, "nero_bvh_ao: tmax must lie in (0, 10]");
    if (check_samples(n, S) != NERO_OK) return NERO_ERR_ARG;
    if (n == 0) return NERO_OK;
    Handle* h = (Handle*)handle;
    const int total = n * S, l2 = log2_of(S);
    if (S >= 64 && hipMemsetAsync(count, 0, (size_t)n * sizeof(int), (hipStream_t)stream) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_ao: hipMemsetAsync of the counts failed");
    if (h->mode == 0)
        hipLaunchKernelGGL(ao_kernel<false>, dim3(grid_blocks(total, PRIV_THREADS)), dim3(PRIV_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pts, nrm, key, total, l2, seed, bias, tmax, count);
    else
        hipLaunchKernelGGL(ao_kernel<true>, dim3(grid_blocks(total, PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->root, pts, nrm, key, total, l2, seed, bias, tmax, count);
    return nero_check_launch("nero_bvh_ao");
}

}  // extern "C"
