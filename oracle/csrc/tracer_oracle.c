/* tracer_oracle.c -- brute-force closest-hit ray/mesh oracle in float64 (Moeller-Trumbore over every triangle).
 *
 * TEST INFRASTRUCTURE ONLY (never linked or called by the product path; see oracle/tracer_oracle.py).  It is the C restatement
 * of oracle/tracer_oracle.py::trace_bruteforce -- same arithmetic, same predicates, same tie rule (first triangle with the
 * smallest t) -- fast enough for the Stage-II parity tests at benchmark-like sizes (10^5 secondary rays), plus the per-ray
 * ambiguity flag of trace_bruteforce_margins.  The contract restated: raytracing/raytracer.py:21-55 and
 * network/renderer.py:719-729 of the reference (closest hit with t > 0, geometric normal from the winding, depth >= 10 = miss);
 * the third-party `_raytracing` binary itself is absent from /root/reference, so parity w.r.t. it is unpinned.
 *
 * Build (by __graft_entry__.build(), flags in oracle/tracer_oracle.py::C_FLAGS):
 *   gcc -O2 -ffp-contract=off -fopenmp -shared -fPIC -o oracle/_build/libtracer_oracle.so oracle/csrc/tracer_oracle.c -lm
 * Below the float64 oracle: the float32 MODEL of the tracer (tracer_model_brute32, tracer_model_walk32).
 */
#include <math.h>
#include <stdint.h>

static void cross3(const double* a, const double* b, double* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

/* verts [nV,3] float32, tris [nT,3] int32, o/d [n,3] float64 -> pos [n,3], nrm [n,3], depth [n] (float64), tri [n] int64,
 * amb [n] uint8 (may be NULL).  Returns 0. */
int tracer_oracle_trace(const float* verts, int nV, const int32_t* tris, int nT, const double* o, const double* d, int64_t n,
                        double miss_depth, double eps_edge, double eps_t, double* pos, double* nrm, double* depth, int64_t* tri,
                        uint8_t* amb) {
    (void)nV;
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t r = 0; r < n; ++r) {
        const double* ro = o + 3 * r;
        const double* rd = d + 3 * r;
        double best = INFINITY;
        int64_t bi = -1;
        /* pass 1: closest hit */
        for (int k = 0; k < nT; ++k) {
            double v0[3], e1[3], e2[3], p[3], tv[3], q[3];
            for (int a = 0; a < 3; ++a) {
                v0[a] = (double)verts[3 * tris[3 * k] + a];
                e1[a] = (double)verts[3 * tris[3 * k + 1] + a] - v0[a];
                e2[a] = (double)verts[3 * tris[3 * k + 2] + a] - v0[a];
                tv[a] = ro[a] - v0[a];
            }
            cross3(rd, e2, p);
            const double det = dot3(e1, p);
            if (!(fabs(det) > 1e-20)) continue;
            const double inv = 1.0 / det;
            const double u = dot3(tv, p) * inv;
            cross3(tv, e1, q);
            const double v = dot3(q, rd) * inv;
            const double t = dot3(e2, q) * inv;
            if (u >= 0 && u <= 1 && v >= 0 && u + v <= 1 && t > 0 && t < miss_depth && t < best) { best = t; bi = k; }
        }
        const double dep = bi >= 0 ? best : miss_depth;
        depth[r] = dep;
        tri[r] = bi;
        for (int a = 0; a < 3; ++a) { pos[3 * r + a] = ro[a] + dep * rd[a]; nrm[3 * r + a] = 0.0; }
        if (bi >= 0) {
            double v0[3], e1[3], e2[3], nn[3];
            for (int a = 0; a < 3; ++a) {
                v0[a] = (double)verts[3 * tris[3 * bi] + a];
                e1[a] = (double)verts[3 * tris[3 * bi + 1] + a] - v0[a];
                e2[a] = (double)verts[3 * tris[3 * bi + 2] + a] - v0[a];
            }
            cross3(e1, e2, nn);
            const double l = sqrt(dot3(nn, nn));
            for (int a = 0; a < 3; ++a) nrm[3 * r + a] = nn[a] / l;
        }
        if (!amb) continue;
        /* pass 2: could a float32 tracer legitimately answer differently?  an edge within eps_edge (barycentric units) of a
         * candidate that is not farther than the closest hit, or a candidate within eps_t of the ray origin */
        uint8_t flag = 0;
        for (int k = 0; k < nT && !flag; ++k) {
            double v0[3], e1[3], e2[3], p[3], tv[3], q[3];
            for (int a = 0; a < 3; ++a) {
                v0[a] = (double)verts[3 * tris[3 * k] + a];
                e1[a] = (double)verts[3 * tris[3 * k + 1] + a] - v0[a];
                e2[a] = (double)verts[3 * tris[3 * k + 2] + a] - v0[a];
                tv[a] = ro[a] - v0[a];
            }
            cross3(rd, e2, p);
            const double det = dot3(e1, p);
            if (!(fabs(det) > 1e-20)) continue;
            const double inv = 1.0 / det;
            const double u = dot3(tv, p) * inv;
            cross3(tv, e1, q);
            const double v = dot3(q, rd) * inv;
            const double t = dot3(e2, q) * inv;
            const double outside = fmax(fmax(-u, -v), u + v - 1.0);          /* <= 0 inside */
            if (fabs(outside) < eps_edge && t > -eps_t && t < dep + eps_t) flag = 1;
            if (outside < eps_edge && fabs(t) < eps_t) flag = 1;
        }
        amb[r] = flag;
    }
    return 0;
}

/* ======================================================================================================================================
 * The float32 MODEL of the mesh tracer: nero_amd/csrc/bvh_walk.h (box_hit, tri_test, ray_inverse, NERO_WALK_PRIVATE) and write_hit of
 * nero_amd/csrc/bvh.hip restated for the host, operation by operation -- every fused multiply-add is an fmaf, nothing else is fused
 * (build_c compiles with -ffp-contract=off), division and square root are IEEE.  Two entry points:
 *   * tracer_model_brute32: tri_test over EVERY triangle record in leaf order -- what an acceleration structure has to reproduce;
 *   * tracer_model_walk32: the walk over the exported tree (64-byte nodes, 48-byte triangle records of nero_bvh_export), which the kernels
 *     have to equal bit for bit.
 * Keep in step with bvh_walk.h: a change of the arithmetic there is a change here.
 * ====================================================================================================================================== */
#define M_NONE (-(1 << 30))

typedef struct { float lmin[3], lmax[3], rmin[3], rmax[3]; int32_t left, right, pad[2]; } MNode;   /* bvh_types.h: Node */
typedef struct { float v0[3], e1[3], e2[3], pad[3]; } MTri;                                       /* bvh_types.h: Tri */

static inline float m_cross_c(float a, float b, float c, float d) { return fmaf(a, b, -(c * d)); }
static inline float m_dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

/* tri_test up to its last line: 1 and *tt when the determinant gate and the u, v, u + v predicates pass */
static inline int m_tri_eval(const MTri* q, const float* o, const float* d, float* tt_out) {
    const float* v0 = q->v0; const float* e1 = q->e1; const float* e2 = q->e2;
    const float px = m_cross_c(d[1], e2[2], d[2], e2[1]), py = m_cross_c(d[2], e2[0], d[0], e2[2]), pz = m_cross_c(d[0], e2[1], d[1], e2[0]);
    const float det = m_dot3(e1[0], e1[1], e1[2], px, py, pz);
    if (fabsf(det) < 1e-20f) return 0;
    const float inv = 1.0f / det;
    const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
    const float u = m_dot3(tx, ty, tz, px, py, pz) * inv;
    if (u < 0.f || u > 1.f) return 0;
    const float qx = m_cross_c(ty, e1[2], tz, e1[1]), qy = m_cross_c(tz, e1[0], tx, e1[2]), qz = m_cross_c(tx, e1[1], ty, e1[0]);
    const float v = m_dot3(d[0], d[1], d[2], qx, qy, qz) * inv;
    if (v < 0.f || u + v > 1.f) return 0;
    *tt_out = m_dot3(e2[0], e2[1], e2[2], qx, qy, qz) * inv;
    return 1;
}
static inline void m_tri_test(const MTri* q, int index, const float* o, const float* d, float* tbest, int* best) {
    float tt;
    if (!m_tri_eval(q, o, d, &tt)) return;
    if (tt > 0.f && tt < *tbest) { *tbest = tt; *best = index; }
}

/* how far the point tri_test reports, o + tt d (in float64), lies outside the triangle's own bounding box: tri_test is not watertight and,
 * for a ray (nearly) in the plane of a triangle, not even local -- it can accept a triangle at a tt that is nowhere near it */
static inline double m_outside(const MTri* q, const float* o, const float* d, float tt) {
    double out = -INFINITY;
    for (int a = 0; a < 3; ++a) {
        const double x0 = q->v0[a], x1 = (double)q->v0[a] + q->e1[a], x2 = (double)q->v0[a] + q->e2[a];
        const double mn = fmin(x0, fmin(x1, x2)), mx = fmax(x0, fmax(x1, x2)), p = (double)o[a] + (double)tt * d[a];
        out = fmax(out, fmax(mn - p, p - mx));
    }
    return out;
}

/* tris: nT records in leaf order; o, d [n,3] float32.  depth [n] (tmax: no triangle accepted), slot [n] (-1), and the ACCEPTED SET of a
 * ray: every slot whose own tt passes tri_test's predicates with 0 < tt < tmax and lies within `band` of the smallest -- n_acc [n] counts
 * them all, the first max_acc are listed in acc_slot / acc_t [n, max_acc] (-1 / NaN beyond).  t_inside / t_outside [n]: the smallest accepted
 * tt (0 < tt < tmax) among the triangles whose reported point lies within `margin` of their own box / farther outside it (INFINITY: none). */
int tracer_model_brute32(const void* tris_, int nT, const float* o, const float* d, int64_t n, float tmax, double band, int max_acc,
                         double margin, float* depth, int32_t* slot, int32_t* acc_slot, float* acc_t, int32_t* n_acc, float* t_inside,
                         float* t_outside) {
    const MTri* tris = (const MTri*)tris_;
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t r = 0; r < n; ++r) {
        const float* ro = o + 3 * r;
        const float* rd = d + 3 * r;
        float tbest = tmax;
        int best = -1;
        for (int k = 0; k < nT; ++k) m_tri_test(tris + k, k, ro, rd, &tbest, &best);
        depth[r] = tbest;
        slot[r] = best;
        int c = 0;
        float t_in = INFINITY, t_out = INFINITY;
        for (int j = 0; j < max_acc; ++j) { acc_slot[r * max_acc + j] = -1; acc_t[r * max_acc + j] = NAN; }
        if (best >= 0) {
            for (int k = 0; k < nT; ++k) {
                float tt;
                if (!m_tri_eval(tris + k, ro, rd, &tt)) continue;
                if (!(tt > 0.f && tt < tmax)) continue;
                if (m_outside(tris + k, ro, rd, tt) > margin) t_out = fminf(t_out, tt); else t_in = fminf(t_in, tt);
                if ((double)tt > (double)tbest + band) continue;
                if (c < max_acc) { acc_slot[r * max_acc + c] = k; acc_t[r * max_acc + c] = tt; }
                ++c;
            }
        }
        n_acc[r] = c;
        t_inside[r] = t_in;
        t_outside[r] = t_out;
    }
    return 0;
}

static inline void m_ray_inverse(const float* d, float* inv) {
    for (int a = 0; a < 3; ++a) inv[a] = 1.0f / (fabsf(d[a]) > 1e-20f ? d[a] : (d[a] < 0.f ? -1e-20f : 1e-20f));
}
/* box_pad: BOX_PAD of bvh_walk.h, which oracle/tracer_oracle.py reads from the header (0: the bare slab test bit for bit -- fmaf(x, y, -0)
 * rounds as x * y does) */
static inline int m_box_hit(const float* mn, const float* mx, const float* o, const float* inv, float tbest, float box_pad, float* tn) {
    float t0 = 0.f, t1 = tbest;
    for (int a = 0; a < 3; ++a) {
        const float p = box_pad * inv[a];
        const float ta = fmaf(mn[a] - o[a], inv[a], -p), tb = fmaf(mx[a] - o[a], inv[a], p);
        const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
        t0 = fmaxf(t0, lo);
        t1 = fminf(t1, hi);
    }
    *tn = t0;
    return t0 <= t1;
}
static inline void m_leaf_test(const MTri* tris, int ref, const float* o, const float* d, float* tbest, int* best, int any) {
    const int code = -ref - 1;
    const int start = code >> 3, count = code & 7;
    for (int i = 0; i < count; ++i) {
        m_tri_test(tris + start + i, start + i, o, d, tbest, best);
        if (any && *best >= 0) return;
    }
}

/* NERO_WALK_PRIVATE over the exported tree, then write_hit.  any = 0: closest hit below tstart (the kernels pass the miss distance 10);
 * any != 0: the walk ends at the first accepted triangle.  Outputs (each may be NULL): pos, nrm [n,3], depth [n], slot [n] (leaf order,
 * -1), steps [n] (nodes visited).  Returns 0, or -1 when a walk needed more than the 64 stack entries the kernel has. */
int tracer_model_walk32(const void* nodes_, const void* tris_, int root, const float* o_, const float* d_, int64_t n, float tstart, int any,
                        float box_pad, float* pos, float* nrm, float* depth, int32_t* slot, int32_t* steps) {
    const MNode* nodes = (const MNode*)nodes_;
    const MTri* tris = (const MTri*)tris_;
    int overflow = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(| : overflow)
    for (int64_t r = 0; r < n; ++r) {
        const float* o = o_ + 3 * r;
        const float* d = d_ + 3 * r;
        float inv[3];
        m_ray_inverse(d, inv);
        float tbest = tstart;
        int best = -1;
        int stack[64];
        int sp = 0, cur = root, visited = 0;
        if (cur != M_NONE && cur < 0) { m_leaf_test(tris, cur, o, d, &tbest, &best, any); cur = M_NONE; }
        while (cur != M_NONE) {
            const MNode* nd = nodes + cur;
            ++visited;
            float tl, tr;
            const int hl = m_box_hit(nd->lmin, nd->lmax, o, inv, tbest, box_pad, &tl);
            const int hr = m_box_hit(nd->rmin, nd->rmax, o, inv, tbest, box_pad, &tr);
            int next = M_NONE;
            int first = nd->left, second = nd->right;
            int hf = hl, hs = hr;
            if (hl && hr && tr < tl) { first = nd->right; second = nd->left; }
            if (!hl) { first = nd->right; hf = hr; hs = 0; }
            if (hf) {
                if (first < 0) m_leaf_test(tris, first, o, d, &tbest, &best, any); else next = first;
            }
            if (any && best >= 0) break;
            if (hs) {
                if (second < 0) m_leaf_test(tris, second, o, d, &tbest, &best, any);
                else if (next == M_NONE) next = second;
                else if (sp < 64) stack[sp++] = second;
                else overflow = 1;
            }
            if (any && best >= 0) break;
            if (next == M_NONE && sp > 0) next = stack[--sp];
            cur = next;
        }
        if (steps) steps[r] = visited;
        if (slot) slot[r] = best;
        if (depth) depth[r] = tbest;
        if (nrm) {
            if (best >= 0) {
                const float* e1 = tris[best].e1; const float* e2 = tris[best].e2;
                const float nx = m_cross_c(e1[1], e2[2], e1[2], e2[1]), ny = m_cross_c(e1[2], e2[0], e1[0], e2[2]),
                            nz = m_cross_c(e1[0], e2[1], e1[1], e2[0]);
                const float nn = fmaxf(sqrtf(m_dot3(nx, ny, nz, nx, ny, nz)), 1e-30f);
                nrm[r * 3] = nx / nn; nrm[r * 3 + 1] = ny / nn; nrm[r * 3 + 2] = nz / nn;
            } else {
                nrm[r * 3] = 0.f; nrm[r * 3 + 1] = 0.f; nrm[r * 3 + 2] = 0.f;
            }
        }
        if (pos) for (int a = 0; a < 3; ++a) pos[r * 3 + a] = fmaf(tbest, d[a], o[a]);
    }
    return overflow ? -1 : 0;
}
