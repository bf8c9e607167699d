// bvh_walk.h -- the device side of the mesh ray tracer's traversal, shared by bvh.hip (closest hit) and visibility.hip (any hit): the box and
// triangle tests, the leaf loaders and the two walks.  A walk takes a compile-time flag ANY:
//   * ANY = false: closest hit.  `tbest` starts at the miss distance and shrinks with every accepted triangle; the walk visits every subtree
//     whose box is nearer than the best hit so far;
//   * ANY = true: any hit within `tbest` (a shadow ray).  The same visits in the same order with the same tests -- tbest, the caller's tmax,
//     bounds the boxes as a closest hit's tbest does before its first hit -- but the walk ends at the first accepted triangle.
// The walks are TEXT (NERO_WALK_PRIVATE / NERO_WALK_OVERLAP), expanded inside the kernels: written as inlined functions they compute the
// same bits with the same registers, but hipcc schedules the closest-hit kernels differently -- among other things it waits for the next
// node's load before the leaf's address arithmetic -- and nero_bvh_trace ran 1 - 4 % slower in an A/B.  Expanded in place, with the state
// declared in the order the kernels always declared it, the ANY = false kernels of bvh.hip have the instruction streams they had with the
// loops written out.
#pragma once
#include <hip/hip_runtime.h>
#include "bvh_types.h"

namespace nero_bvh {

// The slab test, over the box GROWN BY BOX_PAD on every side.  The contract of the walks is that they return what tri_test returns when it is run
// over every triangle, so a box must not be culled while tri_test would accept a triangle inside it -- and the bare test (t0 <= t1 on the
// rounded slab distances) culled two kinds of such boxes (tests/test_tracer_model_cpu.py):
//   * a box whose corner or edge the ray passes within rounding: the entry distance on one axis and the exit distance on another are then equal
//     up to their rounding, in either order (a ray aimed at a mesh vertex is aimed at the corner of the boxes of all triangles around it);
//   * a box with a face in whose plane the ray runs (direction component 0, origin coordinate equal to the face's: marching-cubes vertices on
//     grid lines, axis-aligned depth-map cameras): (mx - o) * 1e20 = 0 puts the exit at t = 0, while the box beyond the face is entered.
// The pad is a length: slab a becomes [mn - PAD, mx + PAD], i.e. its two distances move apart by PAD |inv[a]| each -- one fused multiply-add
// per distance, ((mn - o) - PAD) inv = fma(mn - o, inv, -PAD inv) whatever the sign of inv.  For a component below 1e-20 (inv = +-1e20) the slab
// turns into "o within PAD of [mn, mx]", faces included.  Its size, from the rounding of what is compared: a slab distance carries three
// roundings (the difference, the reciprocal, the product: 3 x 2^-24 relative), which moves the slab by at most 3 x 2^-24 |mn - o| <= 2^-19 for
// |mn - o| <= 10.6 -- the miss distance bounds every distance that matters; the other 2^-19 is for tri_test, whose accepted point o + tt d may
// lie that far outside the triangle's own box (its u, v and tt carry the roundings of two cross and three dot products of vectors of length
// |o - v0|).  The scene is of unit scale with the miss distance 10, as everywhere in the tracer.  What the pad does NOT cover is tri_test
// accepting a triangle far from where the ray is -- a ray almost in a triangle's plane, a sliver of aspect 1e4: the determinant gate of 1e-20
// lets quotients of rounding noise through -- no box test can follow that.  Cost: the multiplies become fused multiply-adds.
constexpr float BOX_PAD = 0x1p-18f;        // 3.8e-6: twice the 2^-19 above
__device__ __forceinline__ bool box_hit(const float* mn, const float* mx, const float* o, const float* inv, float tbest, float& tn) {
#pragma clang fp contract(off)
    float t0 = 0.f, t1 = tbest;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = BOX_PAD * inv[a];
        float ta = fmaf(mn[a] - o[a], inv[a], -p), tb = fmaf(mx[a] - o[a], inv[a], p);
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        t0 = fmaxf(t0, lo);
        t1 = fminf(t1, hi);
    }
    tn = t0;
    return t0 <= t1;
}

// The arithmetic of a ray is the same in every traversal kernel, operation by operation: contraction is switched off and every
// fused multiply-add is written out, so that the kernels agree bit for bit whatever hipcc makes of the code around the expressions.
struct TriQ { float4 a, b, c; };           // the 48 bytes of a Tri: v0 e1 | e1 e2 | e2 pad
__device__ __forceinline__ float cross_c(float a, float b, float c, float d) {     // a b - c d
#pragma clang fp contract(off)
    return fmaf(a, b, -(c * d));
}
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}
__device__ __forceinline__ void tri_test(const TriQ& q, int index, const float* o, const float* d, float& tbest, int& best) {
#pragma clang fp contract(off)
    const float v0[3] = {q.a.x, q.a.y, q.a.z}, e1[3] = {q.a.w, q.b.x, q.b.y}, e2[3] = {q.b.z, q.b.w, q.c.x};
    const float px = cross_c(d[1], e2[2], d[2], e2[1]), py = cross_c(d[2], e2[0], d[0], e2[2]), pz = cross_c(d[0], e2[1], d[1], e2[0]);
    const float det = dot3(e1[0], e1[1], e1[2], px, py, pz);
    if (fabsf(det) < 1e-20f) return;
    const float inv = 1.0f / det;
    const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
    const float u = dot3(tx, ty, tz, px, py, pz) * inv;
    if (u < 0.f || u > 1.f) return;
    const float qx = cross_c(ty, e1[2], tz, e1[1]), qy = cross_c(tz, e1[0], tx, e1[2]), qz = cross_c(tx, e1[1], ty, e1[0]);
    const float v = dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
    if (v < 0.f || u + v > 1.f) return;
    const float tt = dot3(e2[0], e2[1], e2[2], qx, qy, qz) * inv;
    if (tt > 0.f && tt < tbest) { tbest = tt; best = index; }
}
__device__ __forceinline__ TriQ load_tri(const Tri* __restrict__ tris, int i) {
    const float4* p = reinterpret_cast<const float4*>(tris + i);
    TriQ q;
    q.a = p[0]; q.b = p[1]; q.c = p[2];
    return q;
}
// the triangles of a leaf one after the other (low register use: walk_private)
template <bool ANY>
__device__ __forceinline__ void leaf_test(const Tri* __restrict__ tris, int ref, const float* o, const float* d, float& tbest, int& best) {
    const int code = -ref - 1;
    const int start = code >> 3, count = code & 7;
    for (int i = 0; i < count; ++i) {
        tri_test(load_tri(tris, start + i), start + i, o, d, tbest, best);
        if (ANY && best >= 0) return;
    }
}

// the reciprocal direction the box test multiplies by.  A component of at most 1e-20 (+0, -0, denormals) gets +-1e20: finite, so that a ray IN
// the plane of a box face gives (mx - o) inv = 0 and not NaN, and large enough that box_hit's padded slab [-(PAD + d) 1e20, (PAD + d) 1e20] is
// all or nothing against any tbest <= 10 (the kernels of bvh.hip write the same line out)
__device__ __forceinline__ void ray_inverse(const float* d, float* inv) {
#pragma unroll
    for (int a = 0; a < 3; ++a) inv[a] = 1.0f / (fabsf(d[a]) > 1e-20f ? d[a] : (d[a] < 0.f ? -1e-20f : 1e-20f));
}

// ---- private (scratch) stack, one request after the other: trees of any depth the builders admit ---------------------------------
// Expands to the walk of one ray.  In scope at the expansion: nodes, tris, o[3], d[3], inv[3].  Declares float tbest (starts at TSTART: only
// nearer triangles are accepted) and int best (-1: nothing accepted), which hold the result afterwards; CUR0 is the root reference, or NONE
// for a ray that is not to be traversed.
#define NERO_WALK_PRIVATE(ANY, TSTART, CUR0)                                                                  \
    float tbest = (TSTART);                                                                                   \
    int best = -1;                                                                                            \
    int stack[64];                                                                                            \
    int sp = 0;                                                                                               \
    int cur = (CUR0);                                                                                         \
    if (cur != NONE && cur < 0) { leaf_test<ANY>(tris, cur, o, d, tbest, best); cur = NONE; }                 \
    while (cur != NONE) {                                                                                     \
        const Node nd = nodes[cur];                                                                           \
        float tl, tr;                                                                                         \
        const bool hl = box_hit(nd.lmin, nd.lmax, o, inv, tbest, tl);                                         \
        const bool hr = box_hit(nd.rmin, nd.rmax, o, inv, tbest, tr);                                         \
        int next = NONE;                                                                                      \
        int first = nd.left, second = nd.right;                                                               \
        bool hf = hl, hs = hr;                                                                                \
        if (hl && hr && tr < tl) { first = nd.right; second = nd.left; }                                      \
        if (!hl) { first = nd.right; hf = hr; hs = false; }                                                   \
        if (hf) {                                                                                             \
            if (first < 0) leaf_test<ANY>(tris, first, o, d, tbest, best); else next = first;                 \
        }                                                                                                     \
        if (ANY && best >= 0) break;                                                                          \
        if (hs) {                                                                                             \
            if (second < 0) leaf_test<ANY>(tris, second, o, d, tbest, best);                                  \
            else if (next == NONE) next = second;                                                             \
            else if (sp < 64) stack[sp++] = second;                                                           \
        }                                                                                                     \
        if (ANY && best >= 0) break;                                                                          \
        if (next == NONE && sp > 0) next = stack[--sp];                                                       \
        cur = next;                                                                                           \
    }

// ---- memory latencies overlapped, stack in LDS: trees no deeper than PL_STACK ---------------------------------------------------------
struct NodeQ { float4 a, b, c, d; };       // the 64 bytes of a Node: lmin lmax | rmin rmax | left right pad pad
__device__ __forceinline__ NodeQ load_node(const Node* __restrict__ nodes, int i) {
    const float4* p = reinterpret_cast<const float4*>(nodes + i);
    NodeQ q;
    q.a = p[0]; q.b = p[1]; q.c = p[2]; q.d = p[3];
    return q;
}
__device__ __forceinline__ void leaf_test_batched(const Tri* __restrict__ tris, int ref, const float* o, const float* d, float& tbest, int& best) {
    const int code = -ref - 1;
    const int start = code >> 3, count = code & 7;            // <= 4 (Builder::build)
    const float4* p = reinterpret_cast<const float4*>(tris + start);
    TriQ q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {          // unconditional (a short leaf re-reads its first triangle): predicated loads come out of hipcc with a
        const int j = i < count ? i : 0;   // wait inside every predicated block, i.e. one triangle after the other again
        q[i].a = p[3 * j]; q[i].b = p[3 * j + 1]; q[i].c = p[3 * j + 2];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (i < count) tri_test(q[i], start + i, o, d, tbest, best);
}

constexpr int PL_THREADS = 64;             // one wavefront per workgroup (bvh.hip, above trace_overlap_kernel, has the measurements)

// As NERO_WALK_PRIVATE; also in scope: st, this lane's column of the workgroup's LDS stack (entry s at st[s * PL_THREADS]).
// ONE leaf section per step: the second leaf of a node is tested at the start of the lane's next step, before its next node -- the same
// order of visits, but a wavefront executes the triangle code once per step instead of twice (0.57 -> 0.52 ms per 1 M rays).
// The next node is loaded UNCONDITIONALLY (a finished lane re-reads node 0), in flight while the triangles are fetched and tested: behind
// `if (next != NONE)` hipcc reused a padding register of the load as scratch and waited for the node before it requested the triangles
// (0.77 -> 0.73 ms on the rays of a training step).
#define NERO_WALK_OVERLAP(ANY, TSTART, CUR0)                                                                  \
    float tbest = (TSTART);                                                                                   \
    int best = -1, sp = 0, cur = (CUR0);                                                                      \
    NodeQ nd = {};                                                                                            \
    if (cur == NONE) {}                                                                                       \
    else if (cur < 0) { leaf_test<ANY>(tris, cur, o, d, tbest, best); cur = NONE; }                           \
    else nd = load_node(nodes, cur);                                                                          \
    int pend = NONE;                                                                                          \
    while (cur != NONE || pend != NONE) {                                                                     \
        int leaf = pend;                                                                                      \
        pend = NONE;                                                                                          \
        if (leaf == NONE) {                                                                                   \
            const float lmin[3] = {nd.a.x, nd.a.y, nd.a.z}, lmax[3] = {nd.a.w, nd.b.x, nd.b.y};               \
            const float rmin[3] = {nd.b.z, nd.b.w, nd.c.x}, rmax[3] = {nd.c.y, nd.c.z, nd.c.w};               \
            const int left = __float_as_int(nd.d.x), right = __float_as_int(nd.d.y);                          \
            float tl, tr;                                                                                     \
            const bool hl = box_hit(lmin, lmax, o, inv, tbest, tl);                                           \
            const bool hr = box_hit(rmin, rmax, o, inv, tbest, tr);                                           \
            int next = NONE, leaf_a = NONE, leaf_b = NONE;                                                    \
            int first = left, second = right;                                                                 \
            bool hf = hl, hs = hr;                                                                            \
            if (hl && hr && tr < tl) { first = right; second = left; }                                        \
            if (!hl) { first = right; hf = hr; hs = false; }                                                  \
            if (hf) {                                                                                         \
                if (first < 0) leaf_a = first; else next = first;                                             \
            }                                                                                                 \
            if (hs) {                                                                                         \
                if (second < 0) leaf_b = second;                                                              \
                else if (next == NONE) next = second;                                                         \
                else if (sp < PL_STACK) st[(sp++) * PL_THREADS] = second;                                     \
            }                                                                                                 \
            if (next == NONE && sp > 0) next = st[(--sp) * PL_THREADS];                                       \
            nd = load_node(nodes, next != NONE ? next : 0);                                                   \
            cur = next;                                                                                       \
            if (leaf_a != NONE) { leaf = leaf_a; pend = leaf_b; } else leaf = leaf_b;                         \
        }                                                                                                     \
        if (leaf != NONE) leaf_test_batched(tris, leaf, o, d, tbest, best);                                   \
        if (ANY && best >= 0) break;                                                                          \
    }

}  // namespace nero_bvh
