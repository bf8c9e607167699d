// closest_point.hip -- exact point-to-mesh distance on the mesh tracer's BVH (include/nero_closest.h): for every query point the nearest
// point of the surface, as the minimum of point_triangle (closest_point_math.h) over ALL triangles, found by a third walk over the nodes the
// closest-hit and any-hit walks of bvh_walk.h read: nearer child first, a subtree left out only when the padded lower bound of its box
// EXCEEDS the best squared distance so far.  Equal distances are the normal case (a point over a shared edge or vertex), so nothing is ever
// pruned on equality and among equally near triangles the lowest caller face index wins: the result does not depend on the order of visits,
// and tests/closest_ref.py holds it to exhaustive search bit for bit.  One lane per point; no atomics; the same bits on every run.
//   * the traversal stack holds (node, bound) pairs, so a deferred sibling whose bound the best distance has passed meanwhile is dropped when
//     it is popped instead of being fetched: in LDS (PL_STACK entries per lane, one wavefront per workgroup as in the tracer's overlapped
//     walk) for trees no deeper than PL_STACK, in scratch for the deeper ones the builders admit (64 levels);
//   * node and triangle records travel as float4 loads; the next node is requested before the leaves of this one are tested.
#include <hip/hip_runtime.h>
#include <limits.h>
#include "../../include/nero_hip.h"
#include "../../include/nero_closest.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "closest_point_math.h"
#include "common.h"

namespace {

using namespace nero_bvh;
using namespace nero_closest;
constexpr int CP_PRIV_THREADS = 256;       // workgroup of the private-stack kernel (as trace_kernel)
constexpr int CP_PRIV_STACK = 64;          // the deepest tree nero_bvh_create admits

struct Best { float d2; int face, slot; float b1, b2; };

// the triangles of a leaf against p: all loads first (a short leaf re-reads its first triangle, as leaf_test_batched does), then the tests.
// Accepted: strictly nearer, or equally near with a lower caller face -- the face is only read for a triangle that is at least equally near.
__device__ __forceinline__ void cp_leaf(const Tri* __restrict__ tris, const int* __restrict__ face, int ref, const float* p, Best& best) {
    const int code = -ref - 1;
    const int start = code >> 3, count = code & 7;            // <= 4 (both builders)
    const float4* q = reinterpret_cast<const float4*>(tris + start);
    TriQ t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = i < count ? i : 0;
        t[i].a = q[3 * j]; t[i].b = q[3 * j + 1]; t[i].c = q[3 * j + 2];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= count) break;
        const float v0[3] = {t[i].a.x, t[i].a.y, t[i].a.z}, e1[3] = {t[i].a.w, t[i].b.x, t[i].b.y}, e2[3] = {t[i].b.z, t[i].b.w, t[i].c.x};
        const PointTri r = point_triangle(p, v0, e1, e2);
        if (r.d2 <= best.d2) {
            const int f = face[start + i];
            if (r.d2 < best.d2 || f < best.face) { best.d2 = r.d2; best.face = f; best.slot = start + i; best.b1 = r.b1; best.b2 = r.b2; }
        }
    }
}

// LDS: PL_THREADS threads, stack entry s of a lane at [s * PL_THREADS] of its column; else CP_PRIV_THREADS threads and a private stack
template <bool LDS>
__global__ __launch_bounds__(LDS ? PL_THREADS : CP_PRIV_THREADS) void closest_kernel(
    const Node* __restrict__ nodes, const Tri* __restrict__ tris, const int* __restrict__ face_of, int root, const float* __restrict__ pts,
    long long n, float r2, float* __restrict__ dist, int* __restrict__ face, float* __restrict__ bary, float* __restrict__ point) {
    constexpr int CAP = LDS ? PL_STACK : CP_PRIV_STACK;
    __shared__ int lds_node[LDS ? PL_STACK * PL_THREADS : 1];
    __shared__ float lds_bound[LDS ? PL_STACK * PL_THREADS : 1];
    int priv_node[LDS ? 1 : CP_PRIV_STACK];
    float priv_bound[LDS ? 1 : CP_PRIV_STACK];
    // entry s of this lane's stack: its column of the workgroup's LDS arrays, or its private arrays (no pointer that could be either)
    auto at = [&](int s) { return LDS ? s * PL_THREADS + (int)threadIdx.x : s; };
    auto push = [&](int node, float bound, int s) {
        if constexpr (LDS) { lds_node[at(s)] = node; lds_bound[at(s)] = bound; } else { priv_node[s] = node; priv_bound[s] = bound; }
    };
    auto pop = [&](int s, float& bound) -> int {
        if constexpr (LDS) { bound = lds_bound[at(s)]; return lds_node[at(s)]; } else { bound = priv_bound[s]; return priv_node[s]; }
    };

    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
    Best best = {r2, INT_MAX, -1, 0.f, 0.f};          // INT_MAX: a triangle AT d2 == r2 is accepted, whatever its face
    int cur = (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2])) ? root : NONE;
    int sp = 0;
    NodeQ nd = {};
    if (cur == NONE) {}
    else if (cur < 0) { cp_leaf(tris, face_of, cur, p, best); cur = NONE; }
    else nd = load_node(nodes, cur);
    while (cur != NONE) {
        const float lmin[3] = {nd.a.x, nd.a.y, nd.a.z}, lmax[3] = {nd.a.w, nd.b.x, nd.b.y};
        const float rmin[3] = {nd.b.z, nd.b.w, nd.c.x}, rmax[3] = {nd.c.y, nd.c.z, nd.c.w};
        const int left = __float_as_int(nd.d.x), right = __float_as_int(nd.d.y);
        const float bl = box_bound(lmin, lmax, p, CP_PAD), br = box_bound(rmin, rmax, p, CP_PAD);
        const bool swap = br < bl;                              // the nearer child first; the left one when they are equally near
        const int first = swap ? right : left, second = swap ? left : right;
        const float bf = swap ? br : bl, bs = swap ? bl : br;
        int next = NONE, leaf[2] = {NONE, NONE};
        if (!(bf > best.d2)) {
            if (first < 0) leaf[0] = first; else next = first;
        }
        if (!(bs > best.d2)) {
            if (second < 0) leaf[1] = second;
            else if (next == NONE) next = second;
            else if (sp < CAP) push(second, bs, sp++);
        }
        while (next == NONE && sp > 0) {                        // a deferred subtree the best distance has passed meanwhile is dropped unread
            float bound;
            const int node = pop(--sp, bound);
            if (!(bound > best.d2)) next = node;
        }
        nd = load_node(nodes, next != NONE ? next : 0);         // unconditional, in flight while the leaves are fetched and tested
        cur = next;
        for (int k = 0; k < 2; ++k)
            if (leaf[k] != NONE) cp_leaf(tris, face_of, leaf[k], p, best);
    }

    const bool found = best.slot >= 0;
    dist[i] = found ? sqrtf(best.d2) : INFINITY;
    face[i] = found ? best.face : -1;
    if (bary != nullptr) { bary[i * 2] = best.b1; bary[i * 2 + 1] = best.b2; }
    if (point != nullptr) {
        float q[3] = {0.f, 0.f, 0.f};
        if (found) {
#pragma clang fp contract(off)
            const TriQ t = load_tri(tris, best.slot);
            const float v0[3] = {t.a.x, t.a.y, t.a.z}, e1[3] = {t.a.w, t.b.x, t.b.y}, e2[3] = {t.b.z, t.b.w, t.c.x};
            for (int k = 0; k < 3; ++k) q[k] = v0[k] + (best.b1 * e1[k] + best.b2 * e2[k]);
        }
        for (int k = 0; k < 3; ++k) point[i * 3 + k] = q[k];
    }
}

}  // namespace

extern "C" {

int nero_bvh_closest(void* handle, const float* pts, int64_t n, float max_dist, float* dist, int* face, float* bary, float* point,
                     void* stream) {
    if (!handle || !pts || !dist || !face) return nero_fail(NERO_ERR_ARG, "nero_bvh_closest: null handle or pointer");
    if (n < 0) return nero_fail(NERO_ERR_ARG, "nero_bvh_closest: n must be >= 0");
    if (!(max_dist > 0.f)) return nero_fail(NERO_ERR_ARG, "nero_bvh_closest: max_dist must be positive (+inf: no limit)");
    if (n > ((int64_t)1 << 36)) return nero_fail(NERO_ERR_ARG, "nero_bvh_closest: more than 2^36 points: call in chunks");
    if (n == 0) return NERO_OK;
    const Handle* h = (const Handle*)handle;
    const float r2 = max_dist * max_dist;
    if (h->mode == 0)
        hipLaunchKernelGGL(closest_kernel<false>, dim3((unsigned)((n + CP_PRIV_THREADS - 1) / CP_PRIV_THREADS)), dim3(CP_PRIV_THREADS), 0,
                           (hipStream_t)stream, h->b.d_nodes, h->b.d_tris, h->b.d_face, h->root, pts, (long long)n, r2, dist, face, bary, point);
    else
        hipLaunchKernelGGL(closest_kernel<true>, dim3((unsigned)((n + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, (hipStream_t)stream,
                           h->b.d_nodes, h->b.d_tris, h->b.d_face, h->root, pts, (long long)n, r2, dist, face, bary, point);
    return nero_check_launch("nero_bvh_closest");
}

}  // extern "C"
