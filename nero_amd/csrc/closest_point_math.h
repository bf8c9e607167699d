// closest_point_math.h -- the arithmetic of the closest-point query (closest_point.hip, include/nero_closest.h): the distance from a point to
// a triangle as the tree stores it, and the lower bound of the distance to a box.  Plain C++ that compiles for the device and for the host:
// tests/closest_point_main.cpp runs this same source under the sanitizers, tests/closest_ref.py restates it in numpy, one numpy operation per
// operation below.  Contraction is off and no fused multiply-add is written: every product, sum and quotient is rounded on its own, in the
// order written, so that the three agree bit for bit.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NERO_CP_FN __host__ __device__ __forceinline__
#else
#define NERO_CP_FN inline
#endif

namespace nero_closest {

struct PointTri { float d2, b1, b2; };     // squared distance to q = v0 + b1 e1 + b2 e2; b1 >= 0, b2 >= 0, b1 + b2 <= 1

NERO_CP_FN float cp_dot(const float* a, const float* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
NERO_CP_FN void cp_cross(const float* a, const float* b, float* c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
// t clamped to [0, hi] by comparisons: -0 and anything unordered give +0, so the sign of a zero weight does not depend on a library's fmaxf
NERO_CP_FN float cp_clamp(float t, float hi) { return t > 0.f ? (t < hi ? t : hi) : 0.f; }
// the parameter of the point of the segment {x0 + t e, 0 <= t <= 1} nearest to x0 + w: one clamp of dot / len2.  A segment of length 0 is its
// endpoint (t = 0) -- the quotient is never taken with a zero divisor, and for finite operands it is never NaN.
NERO_CP_FN float cp_segment(const float* w, const float* e) {
#pragma clang fp contract(off)
    const float len2 = cp_dot(e, e);
    const float t = cp_dot(w, e) / (len2 > 0.f ? len2 : 1.f);
    return len2 > 0.f ? cp_clamp(t, 1.f) : 0.f;
}
// a candidate (b1, b2): the squared length of d - (b1 e1 + b2 e2), kept when it is strictly smaller than what `best` holds
NERO_CP_FN void cp_candidate(const float* d, const float* e1, const float* e2, float b1, float b2, PointTri& best) {
#pragma clang fp contract(off)
    float r[3];
    for (int k = 0; k < 3; ++k) r[k] = d[k] - (b1 * e1[k] + b2 * e2[k]);
    const float d2 = cp_dot(r, r);
    if (d2 < best.d2) { best.d2 = d2; best.b1 = b1; best.b2 = b2; }
}

// The point of the triangle (v0, e1, e2) nearest to p, as the minimum over FOUR candidates, each a point of the triangle by construction:
//   * the nearest point of each of the three edge segments (one clamped quotient each).  They are always there, so a triangle of zero area is
//     the segment or the point it is, and a sliver whose interior candidate is noise still reports a distance to its boundary;
//   * the foot of the perpendicular, from the normal n = e1 x e2 (b1 = ((d x e2) . n) / |n|^2, b2 = ((e1 x d) . n) / |n|^2 -- the
//     determinant is |e1 x e2|^2 and not a c - b^2 of the Gram matrix, which cancels to nothing on slivers), with the weights clamped INTO the
//     triangle.  Inside, it is the nearest point; clamped, it is some point of the triangle and an edge candidate is nearer.  |n|^2 == 0: no
//     such candidate.
// d2 is computed from the weights that are returned, so it is the distance to a point OF the triangle up to the rounding of that one
// expression; b1 + b2 <= 1 holds exactly (1 - (1 - t) and 1 - t sum to 1 without rounding for every float t in [0, 1]).
// Candidates in a fixed order (edge e1, edge e2, the edge opposite v0, interior); a later one wins only when it is strictly nearer.
NERO_CP_FN PointTri point_triangle(const float* p, const float* v0, const float* e1, const float* e2) {
#pragma clang fp contract(off)
    const float d[3] = {p[0] - v0[0], p[1] - v0[1], p[2] - v0[2]};
    PointTri best = {INFINITY, 0.f, 0.f};
    cp_candidate(d, e1, e2, cp_segment(d, e1), 0.f, best);
    cp_candidate(d, e1, e2, 0.f, cp_segment(d, e2), best);
    {
        const float w[3] = {d[0] - e1[0], d[1] - e1[1], d[2] - e1[2]};
        const float e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
        const float b1 = 1.f - cp_segment(w, e3);
        cp_candidate(d, e1, e2, b1, 1.f - b1, best);
    }
    float n[3];
    cp_cross(e1, e2, n);
    const float nn = cp_dot(n, n);
    if (nn > 0.f) {
        float m1[3], m2[3];
        cp_cross(d, e2, m1);
        cp_cross(e1, d, m2);
        const float lim = 1.f - cp_clamp(cp_dot(m1, n) / nn, 1.f);
        const float b2 = cp_clamp(cp_dot(m2, n) / nn, lim);
        cp_candidate(d, e1, e2, 1.f - lim, b2, best);
    }
    return best;
}

// The lower bound of the squared distance from p to the points of the box [mn, mx], over the box GROWN BY CP_PAD on every side: per axis
// the gap max(mn - p, p - mx) less the pad, not below zero; the sum of the three squares.  The contract of the walk is that it returns what
// point_triangle returns when it is run over every triangle, so a box must not be pruned while a triangle inside it computes a d2 at or below
// the best so far: the COMPUTED bound has to stay at or below the COMPUTED d2 of every triangle of the box.  In exact arithmetic it does; in
// float32 both carry roundings, which the pad covers.  With u = 2^-24, D = |p - v0| and everything as a length:
//   * the triangle side.  The point q = v0 + b1 e1 + b2 e2 that d2 belongs to lies in the triangle, hence in the box.  r = d - (b1 e1 + b2 e2)
//     as computed differs from p - q by u |d| (the subtraction p - v0), 3 u (b1 |e1| + b2 |e2|) <= 6 u D (two products and a sum; an edge is no
//     longer than 2 D) and u |r| <= u D (the last subtraction): 8 u D.  The dot product of r with itself adds 3 u relative to d2, 1.5 u D as a length;
//   * the box side.  A gap carries two roundings (the subtraction, the pad) and its square a third, the two sums two more: at most 7 u relative
//     to the bound, 3.5 u D as a length.
// Together 13 u D.  Subtracting the pad on every axis shortens the gap vector g by at least the pad: |g| >= g . g'/|g'| = |g'| + pad (sum of
// the components of the unit vector g'/|g'|, all >= 0) >= |g'| + pad.  The domain is the tracer's: a scene of unit scale (|v| <= 1.1) queried
// from |coordinate| <= 10, so D <= 10 sqrt(3) + 1.1 < 18.5 and 13 u D < 1.44e-5 < 2^-16; the pad is twice that, as BOX_PAD is twice its bound.
// Cost: a box within 3.1e-5 of the best distance is opened instead of pruned.  tests/test_closest_point_cpu.py shows the walk equal to
// exhaustive search with this pad and unequal with none.
constexpr float CP_PAD = 0x1p-15f;
NERO_CP_FN float box_bound(const float* mn, const float* mx, const float* p, float pad) {
#pragma clang fp contract(off)
    float g[3];
    for (int k = 0; k < 3; ++k) g[k] = fmaxf(fmaxf(mn[k] - p[k], p[k] - mx[k]) - pad, 0.f);
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

}  // namespace nero_closest
