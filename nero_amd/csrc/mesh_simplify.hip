// mesh_simplify.hip -- simplification of the extracted Stage-I mesh by vertex clustering on a uniform grid with quadric-error placement
// (include/nero_hip.h, nero_mesh_simplify_*; the definition is DESIGN.md's, restated in numpy by tests/mesh_simplify_ref.py).  A 512^3
// extraction gives one to three million triangles, far finer than anything Stage II resolves; this runs directly behind the clean-up of
// mesh_clean.hip, on the device mesh.
//   count    the cell key of every vertex (float64 floor((x - origin) / cell) per axis, a true division; 21 bits per axis), the survivor
//            flag of every triangle (three pairwise different keys) and its prefix sum; then a stable radix sort of the vertex keys, head
//            flags and a prefix sum number the occupied cells in ascending key order, the survivors flag the cells they touch (every writer
//            stores the same value), and a prefix sum numbers the used cells: the output vertices.  The 16-byte totals.
//   emit     a stable radix sort of the 3T contributions (triangle, corner) by the cell of the corner; one wave per used cell sums the
//            cell's vertices (ascending vertex id) and then its contributions (ascending 3 t + corner) in float64, in two fixed levels: the
//            sorted run is cut into pieces of MS_PIECE, the wave sums a piece (each lane its elements in ascending order, then a
//            butterfly) and adds the pieces in ascending order.  Lane 0 solves (A + lambda tr(A)/3 I) d = r by a pivot-free LDL^T (the
//            regulariser bounds the condition number by 3001) and clamps to the cell's box.  The survivors are renumbered; for the
//            de-duplication their sorted vertex triples (93 bits) are sorted by two stable passes, (middle, largest) and then smallest, so
//            that equal triples are adjacent in ascending input order and the first of each run stays.
// Every cross-workgroup value sits behind a kernel boundary (the XCDs' L2 caches are not coherent inside a launch, see mesh_clean.hip); the
// only atomics are integer counters of refused input.  No floating-point atomics: every output is bit-identical run to run.
// The file is compiled without floating-point contraction, so that the keys, the normals and the clamp bounds are the IEEE operations the
// restatement performs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip.h"
#include "common.h"
#include "cub_calls.h"
#include "device_prims.h"
#include "ws_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace nero_cub;
using namespace nero_prims;
using namespace nero_ws;

constexpr int MS_THREADS = 256;
constexpr int MS_PIECE = 2048;                                      // elements a wave sums into one partial
constexpr int64_t MS_MAX_V = ((int64_t)1 << 31) - 1;               // int32 ids, int item counts of hipCUB
constexpr int64_t MS_MAX_T = MS_MAX_V / 3;                          // the 3T contributions are hipCUB items too
constexpr double MS_AXIS_LIMIT = 2097152.0;                         // 2^21 cells per axis
constexpr double MS_LAMBDA = 1e-3;
constexpr unsigned long long MS_NO_KEY = ~0ull;                     // (the largest valid key is 2^63 - 1)

typedef unsigned long long u64;

struct MsParams {
    double cell, ox, oy, oz;
};

// hdr (int64): 0 V', 1 survivors, 2 refused vertices, 3 refused triangles, 4 occupied cells, 5 T' of the last emit, 6 the count was complete
enum { H_VOUT = 0, H_SURV = 1, H_BADV = 2, H_BADT = 3, H_CELLS = 4, H_TOUT = 5, H_FULL = 6, H_WORDS = 8 };

__device__ __forceinline__ bool ms_axis(float x, double o, double cell, u64* i) {
    const double d = floor(((double)x - o) / cell);
    if (!(d >= 0.0 && d < MS_AXIS_LIMIT)) return false;              // (NaN fails both)
    *i = (u64)d;
    return true;
}

__global__ __launch_bounds__(MS_THREADS) void ms_key_kernel(const float* __restrict__ verts, int V, MsParams p, u64* __restrict__ key,
                                                            unsigned* __restrict__ val, u64* hdr) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    bool bad = false;
    if (v < V) {
        u64 ix = 0, iy = 0, iz = 0;
        const bool ok = ms_axis(verts[3 * v], p.ox, p.cell, &ix) & ms_axis(verts[3 * v + 1], p.oy, p.cell, &iy) &
                        ms_axis(verts[3 * v + 2], p.oz, p.cell, &iz);
        key[v] = ok ? (ix << 42) | (iy << 21) | iz : MS_NO_KEY;
        val[v] = (unsigned)v;
        bad = !ok;
    }
    const u64 m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(hdr + H_BADV, (u64)__popcll(m));
}

// fflag [T + 1]: the triangle survives; fflag[T] = 0 (the scan's trailing entry)
__global__ __launch_bounds__(MS_THREADS) void ms_survivor_kernel(const int* __restrict__ tris, int64_t T, int V, const u64* __restrict__ key,
                                                                 int* __restrict__ fflag, u64* hdr) {
    const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    bool bad = false;
    if (t <= T) {
        int k = 0;
        if (t < T) {
            const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
            if (in_range(a, V) && in_range(b, V) && in_range(c, V)) {
                const u64 ka = key[a], kb = key[b], kc = key[c];
                k = ka != MS_NO_KEY && kb != MS_NO_KEY && kc != MS_NO_KEY && ka != kb && kb != kc && ka != kc;
            } else {
                bad = true;                                          // reported by the call; the triangle is never followed
            }
        }
        fflag[t] = k;
    }
    const u64 m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(hdr + H_BADT, (u64)__popcll(m));
}

// over the sorted keys, i in [0, V]: 1 at the first vertex of every cell; 0 at refused vertices (they sort last) and at i = V
__global__ __launch_bounds__(MS_THREADS) void ms_head_kernel(const u64* __restrict__ skey, int V, int* __restrict__ hflag) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i > V) return;
    hflag[i] = i < V && skey[i] != MS_NO_KEY && (i == 0 || skey[i] != skey[i - 1]);
}

// cellid[v] = the rank of v's cell among the occupied ones (-1 for a refused vertex); vstart[c] = the first sorted vertex of cell c,
// vstart[C] = the number of accepted vertices
__global__ __launch_bounds__(MS_THREADS) void ms_cell_kernel(const u64* __restrict__ skey, const unsigned* __restrict__ sval,
                                                             const int* __restrict__ hflag, const int* __restrict__ hpre, int V,
                                                             int* __restrict__ cellid, int* __restrict__ vstart) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i > V) return;
    const bool valid = i < V && skey[i] != MS_NO_KEY;
    if (i < V) cellid[sval[i]] = valid ? hpre[i] + hflag[i] - 1 : -1;
    const bool end = !valid && (i == 0 || skey[i - 1] != MS_NO_KEY);
    if ((valid && hflag[i]) || end) vstart[hpre[i]] = (int)i;
}

__global__ __launch_bounds__(MS_THREADS) void ms_used_kernel(const int* __restrict__ tris, int64_t T, const int* __restrict__ fflag,
                                                             const int* __restrict__ cellid, int* used) {
    const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (t >= T || !fflag[t]) return;                                 // (a survivor passed the range check and has three accepted vertices)
#pragma unroll
    for (int c = 0; c < 3; ++c) used[cellid[tris[3 * t + c]]] = 1;   // (every writer stores the same value)
}

__global__ void ms_totals_kernel(const int* __restrict__ fpre, int64_t T, const int* __restrict__ hpre, const int* __restrict__ upre, int V,
                                 int full, u64* hdr, int* __restrict__ totals) {
    if (threadIdx.x != 0) return;
    const long long surv = fpre[T], vout = full ? upre[V] : -1;
    hdr[H_VOUT] = (u64)vout;
    hdr[H_SURV] = (u64)surv;
    hdr[H_CELLS] = full ? (u64)hpre[V] : 0;
    hdr[H_FULL] = (u64)full;
    totals[0] = (int)vout;
    totals[1] = (int)surv;
    totals[2] = (int)hdr[H_BADV];
    totals[3] = (int)hdr[H_BADT];
}

// ---- emit -------------------------------------------------------------------------------------------------------------------------------
// contribution i = 3 t + c: sort key = the cell of corner c (V, behind every cell, for a triangle that is not followed)
__global__ __launch_bounds__(MS_THREADS) void ms_contrib_key_kernel(const int* __restrict__ tris, int64_t n3, int V,
                                                                    const int* __restrict__ cellid, unsigned* __restrict__ key,
                                                                    unsigned* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n3) return;
    const int64_t t = i / 3;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    int k = -1;
    if (in_range(a, V) && in_range(b, V) && in_range(c, V)) k = cellid[tris[i]];
    key[i] = k >= 0 ? (unsigned)k : (unsigned)V;
    val[i] = (unsigned)i;
}

// cstart / cend [V + 1], zeroed before: the run of each cell in the sorted contributions (a cell without one keeps the empty run)
__global__ __launch_bounds__(MS_THREADS) void ms_contrib_range_kernel(const unsigned* __restrict__ skey, int64_t n3, int* __restrict__ cstart,
                                                                      int* __restrict__ cend) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n3) return;
    const unsigned k = skey[i];
    if (i == 0 || skey[i - 1] != k) cstart[k] = (int)i;
    if (i == n3 - 1 || skey[i + 1] != k) cend[k] = (int)(i + 1);
}

// one wave per occupied cell; only the used cells are placed
__global__ __launch_bounds__(MS_THREADS) void ms_place_kernel(const float* __restrict__ verts, const int* __restrict__ tris,
                                                              const u64* __restrict__ skey, const unsigned* __restrict__ sval,
                                                              const int* __restrict__ vstart, const unsigned* __restrict__ cval,
                                                              const int* __restrict__ cstart, const int* __restrict__ cend,
                                                              const int* __restrict__ used, const int* __restrict__ upre, int64_t C,
                                                              MsParams p, int quadric, double* __restrict__ pos64, float* __restrict__ pos32,
                                                              long long* __restrict__ cell_key, int64_t v_cap) {
    const int64_t c = (int64_t)blockIdx.x * (MS_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= C || !used[c]) return;                                  // (wave-uniform)
    const int64_t out = upre[c];
    if (out >= v_cap) return;
    const int lane = threadIdx.x & 63;
    const int64_t vb = vstart[c], ve = vstart[c + 1];
    double m[3] = {0.0, 0.0, 0.0};
    for (int64_t pb = vb; pb < ve; pb += MS_PIECE) {
        const int64_t pe = pb + MS_PIECE < ve ? pb + MS_PIECE : ve;
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t i = pb + lane; i < pe; i += 64) {
            const float* q = verts + 3 * (int64_t)sval[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) s[a] += (double)q[a];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] += wave_sum(s[a]);
    }
    const double cnt = (double)(ve - vb);
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] /= cnt;
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};   // xx xy xz yy yz zz
    if (quadric) {
        const int64_t cb = cstart[c], ce = cend[c];
        for (int64_t pb = cb; pb < ce; pb += MS_PIECE) {
            const int64_t pe = pb + MS_PIECE < ce ? pb + MS_PIECE : ce;
            double sa[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sr[3] = {0.0, 0.0, 0.0};
            for (int64_t i = pb + lane; i < pe; i += 64) {
                const int64_t id = cval[i], t = id / 3;
                const int corner = (int)(id - 3 * t);
                double q[3][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float* src = verts + 3 * (int64_t)tris[3 * t + k];
#pragma unroll
                    for (int a = 0; a < 3; ++a) q[k][a] = (double)src[a];
                }
                const double ux = q[1][0] - q[0][0], uy = q[1][1] - q[0][1], uz = q[1][2] - q[0][2];
                const double wx = q[2][0] - q[0][0], wy = q[2][1] - q[0][1], wz = q[2][2] - q[0][2];
                const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                const double* pc = corner == 0 ? q[0] : corner == 1 ? q[1] : q[2];
                const double d = nx * (pc[0] - m[0]) + ny * (pc[1] - m[1]) + nz * (pc[2] - m[2]);
                sa[0] += nx * nx; sa[1] += nx * ny; sa[2] += nx * nz; sa[3] += ny * ny; sa[4] += ny * nz; sa[5] += nz * nz;
                sr[0] += nx * d;  sr[1] += ny * d;  sr[2] += nz * d;
            }
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a] += wave_sum(sa[a]);
#pragma unroll
            for (int a = 0; a < 3; ++a) r[a] += wave_sum(sr[a]);
        }
    }
    if (lane != 0) return;
    const u64 key = skey[vb];
    double x[3] = {m[0], m[1], m[2]};
    const double tr = A[0] + A[3] + A[5];
    if (quadric && tr != 0.0) {
        const double reg = MS_LAMBDA * (tr / 3.0);
        const double a00 = A[0] + reg, a01 = A[1], a02 = A[2], a11 = A[3] + reg, a12 = A[4], a22 = A[5] + reg;
        // M = L D L^T without pivoting (M is symmetric positive definite with condition number <= 3001)
        const double d0 = a00, l10 = a01 / d0, l20 = a02 / d0;
        const double d1 = a11 - l10 * a01, l21 = (a12 - l20 * a01) / d1;
        const double d2 = a22 - l20 * a02 - l21 * (l21 * d1);
        const double y0 = r[0], y1 = r[1] - l10 * y0, y2 = r[2] - l20 * y0 - l21 * y1;
        const double z2 = y2 / d2, z1 = y1 / d1 - l21 * z2, z0 = y0 / d0 - l10 * z1 - l20 * z2;
        const double o[3] = {p.ox, p.oy, p.oz}, dx[3] = {z0, z1, z2};
        const u64 idx[3] = {key >> 42, (key >> 21) & 0x1FFFFF, key & 0x1FFFFF};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = o[a] + (double)idx[a] * p.cell, hi = o[a] + (double)(idx[a] + 1) * p.cell;
            double xa = m[a] + dx[a];
            xa = xa < lo ? lo : xa;
            xa = xa > hi ? hi : xa;
            x[a] = xa;
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pos64[3 * out + a] = x[a];
        pos32[3 * out + a] = (float)x[a];
    }
    cell_key[out] = (long long)key;
}

__global__ __launch_bounds__(MS_THREADS) void ms_vmap_kernel(const int* __restrict__ cellid, const int* __restrict__ used,
                                                             const int* __restrict__ upre, int V, int* __restrict__ vmap) {
    const int64_t v = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= V) return;
    const int c = cellid[v];
    vmap[v] = c >= 0 && used[c] ? upre[c] : -1;
}

// the output vertices of survivor t in its own winding, and sorted ascending
__device__ __forceinline__ void ms_corners(const int* __restrict__ tris, int64_t t, const int* __restrict__ cellid,
                                           const int* __restrict__ upre, int* w) {
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = upre[cellid[tris[3 * t + c]]];
}
__device__ __forceinline__ void ms_sort3(int* w) {
    int t;
    if (w[0] > w[1]) { t = w[0]; w[0] = w[1]; w[1] = t; }
    if (w[1] > w[2]) { t = w[1]; w[1] = w[2]; w[2] = t; }
    if (w[0] > w[1]) { t = w[0]; w[0] = w[1]; w[1] = t; }
}

// survivor s = fpre[t]: surv_t[s] = t; first sort key (middle << 32 | largest) of its sorted triple
__global__ __launch_bounds__(MS_THREADS) void ms_triple_kernel(const int* __restrict__ tris, int64_t T, const int* __restrict__ fflag,
                                                               const int* __restrict__ fpre, const int* __restrict__ cellid,
                                                               const int* __restrict__ upre, unsigned* __restrict__ surv_t,
                                                               u64* __restrict__ key, unsigned* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (t >= T || !fflag[t]) return;
    const int s = fpre[t];
    int w[3];
    ms_corners(tris, t, cellid, upre, w);
    ms_sort3(w);
    surv_t[s] = (unsigned)t;
    key[s] = ((u64)(unsigned)w[1] << 32) | (unsigned)w[2];
    val[s] = (unsigned)s;
}

// second sort key of the survivors in the order of the first pass: the smallest vertex
__global__ __launch_bounds__(MS_THREADS) void ms_second_key_kernel(const int* __restrict__ tris, const unsigned* __restrict__ order, int64_t n,
                                                                   const unsigned* __restrict__ surv_t, const int* __restrict__ cellid,
                                                                   const int* __restrict__ upre, unsigned* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= n) return;
    int w[3];
    ms_corners(tris, surv_t[order[i]], cellid, upre, w);
    ms_sort3(w);
    key[i] = (unsigned)w[0];
}

// order: the survivors sorted by their triples, equal triples in ascending input order.  keep [n + 1]: the first of every run; keep[n] = 0
__global__ __launch_bounds__(MS_THREADS) void ms_first_kernel(const int* __restrict__ tris, const unsigned* __restrict__ order, int64_t n,
                                                              const unsigned* __restrict__ surv_t, const int* __restrict__ cellid,
                                                              const int* __restrict__ upre, int* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        keep[n] = 0;
        return;
    }
    int first = 1;
    if (i > 0) {
        int a[3], b[3];
        ms_corners(tris, surv_t[order[i]], cellid, upre, a);
        ms_corners(tris, surv_t[order[i - 1]], cellid, upre, b);
        ms_sort3(a);
        ms_sort3(b);
        first = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
    }
    keep[order[i]] = first;
}

__global__ __launch_bounds__(MS_THREADS) void ms_emit_tris_kernel(const int* __restrict__ tris, int64_t T, const int* __restrict__ fflag,
                                                                  const int* __restrict__ fpre, const int* __restrict__ cellid,
                                                                  const int* __restrict__ upre, const int* __restrict__ keep,
                                                                  const int* __restrict__ opre, int* __restrict__ out, int64_t t_cap,
                                                                  int* __restrict__ fmap) {
    const int64_t t = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
    if (t >= T) return;
    int64_t o = -1;
    if (fflag[t]) {
        const int s = fpre[t];
        o = keep ? (keep[s] ? opre[s] : -1) : s;
        if (o >= t_cap) o = -1;                                      // (excluded by the host's check of the capacity)
        if (o >= 0) {
            int w[3];
            ms_corners(tris, t, cellid, upre, w);
            out[3 * o] = w[0];
            out[3 * o + 1] = w[1];
            out[3 * o + 2] = w[2];
        }
    }
    if (fmap) fmap[t] = (int)o;
}

__global__ void ms_final_kernel(const int* __restrict__ opre, int64_t n, u64* hdr, int64_t* __restrict__ n_out) {
    if (threadIdx.x != 0) return;
    const long long x = opre ? opre[n] : (long long)n;
    hdr[H_TOUT] = (u64)x;
    if (n_out) *n_out = x;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= MS_MAX_V && T <= MS_MAX_T; }

struct Layout {
    size_t hdr, vkey_a, vkey_b, vval_a, vval_b, cellid, hflag, hpre, vstart, used, upre, fflag, fpre, ckey_a, ckey_b, cval_a, cval_b,
        cstart, cend, dkey_a, dkey_b, dval_a, dval_b, akey_a, akey_b, surv_t, keep, opre, temp, temp_bytes, total;
};

Layout layout(int64_t V, int64_t T) {
    Layout w{};
    Carve c;
    const size_t v1 = (size_t)(V + 1) * sizeof(int), t1 = (size_t)(T + 1) * sizeof(int), n3 = (size_t)(3 * T);
    w.hdr = c.take(H_WORDS * sizeof(u64));
    w.vkey_a = c.take((size_t)V * 8);
    w.vkey_b = c.take((size_t)V * 8);
    w.vval_a = c.take((size_t)V * 4);
    w.vval_b = c.take((size_t)V * 4);
    w.cellid = c.take(v1);
    w.hflag = c.take(v1);
    w.hpre = c.take(v1);
    w.vstart = c.take(v1);
    w.used = c.take(v1);
    w.upre = c.take(v1);
    w.fflag = c.take(t1);
    w.fpre = c.take(t1);
    w.ckey_a = c.take(n3 * 4);
    w.ckey_b = c.take(n3 * 4);
    w.cval_a = c.take(n3 * 4);
    w.cval_b = c.take(n3 * 4);
    w.cstart = c.take(v1);
    w.cend = c.take(v1);
    w.dkey_a = c.take((size_t)T * 8);
    w.dkey_b = c.take((size_t)T * 8);
    w.dval_a = c.take((size_t)T * 4);
    w.dval_b = c.take((size_t)T * 4);
    w.akey_a = c.take((size_t)T * 4);
    w.akey_b = c.take((size_t)T * 4);
    w.surv_t = c.take((size_t)T * 4);
    w.keep = c.take(t1);
    w.opre = c.take(t1);
    const size_t a = sort_temp_bound(V + 1, 12), b = sort_temp_bound(3 * T + 1, 8);
    w.temp_bytes = a > b ? a : b;
    w.temp = c.take(w.temp_bytes);
    w.total = c.at;
    return w;
}

bool params_ok(double cell, const double* origin) {
    return cell > 0.0 && isfinite(cell) && origin && isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2]);
}

}  // namespace

size_t nero_mesh_simplify_workspace_bytes(int64_t V, int64_t T) {
    if (!sizes_ok(V, T)) return 0;
    return layout(V, T).total;
}

int nero_mesh_simplify_count(const float* verts, const int* tris, int64_t T, int64_t V, double cell, const double* origin, int faces_only,
                             void* ws, int* totals, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_simplify_count: V must be in [0, 2^31) and 3 T in [0, 2^31)");
    if (!ws || !totals || (V > 0 && !verts) || (T > 0 && !tris)) return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_count: null pointer");
    if (!params_ok(cell, origin))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_count: the cell must be positive and finite, the origin three finite numbers");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    const Layout L = layout(V, T);
    const MsParams p{cell, origin[0], origin[1], origin[2]};
    u64* hdr = (u64*)(w + L.hdr);
    u64* vkey = (u64*)(w + L.vkey_a);
    u64* skey = (u64*)(w + L.vkey_b);
    unsigned* vval = (unsigned*)(w + L.vval_a);
    unsigned* sval = (unsigned*)(w + L.vval_b);
    int* fflag = (int*)(w + L.fflag);
    int* fpre = (int*)(w + L.fpre);
    int* hflag = (int*)(w + L.hflag);
    int* hpre = (int*)(w + L.hpre);
    int* used = (int*)(w + L.used);
    int* upre = (int*)(w + L.upre);
    int* cellid = (int*)(w + L.cellid);
    int* vstart = (int*)(w + L.vstart);
    if (hipMemsetAsync(hdr, 0, H_WORDS * sizeof(u64), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_simplify_count: hipMemsetAsync failed");
    if (V > 0) {
        hipLaunchKernelGGL(ms_key_kernel, dim3(blocks_of(V)), dim3(MS_THREADS), 0, s, verts, (int)V, p, vkey, vval, hdr);
        if (int rc = nero_check_launch("nero_mesh_simplify_count: keys")) return rc;
    }
    hipLaunchKernelGGL(ms_survivor_kernel, dim3(blocks_of(T + 1)), dim3(MS_THREADS), 0, s, tris, T, (int)V, (const u64*)vkey, fflag, hdr);
    if (int rc = nero_check_launch("nero_mesh_simplify_count: survivors")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)fflag, fpre, T + 1, s, "nero_mesh_simplify_count: survivor scan failed")) return rc;
    const int full = !faces_only;
    if (full) {
        if (V > 0)
            if (int rc = sort_pairs<u64>(w + L.temp, L.temp_bytes, vkey, skey, vval, sval, V, 64, s, "nero_mesh_simplify_count: vertex sort failed")) return rc;
        hipLaunchKernelGGL(ms_head_kernel, dim3(blocks_of(V + 1)), dim3(MS_THREADS), 0, s, (const u64*)skey, (int)V, hflag);
        if (int rc = nero_check_launch("nero_mesh_simplify_count: head flags")) return rc;
        if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)hflag, hpre, V + 1, s, "nero_mesh_simplify_count: cell scan failed")) return rc;
        hipLaunchKernelGGL(ms_cell_kernel, dim3(blocks_of(V + 1)), dim3(MS_THREADS), 0, s, (const u64*)skey, (const unsigned*)sval,
                           (const int*)hflag, (const int*)hpre, (int)V, cellid, vstart);
        if (int rc = nero_check_launch("nero_mesh_simplify_count: cells")) return rc;
        if (hipMemsetAsync(used, 0, (size_t)(V + 1) * sizeof(int), s) != hipSuccess)
            return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_simplify_count: hipMemsetAsync failed");
        if (T > 0) {
            hipLaunchKernelGGL(ms_used_kernel, dim3(blocks_of(T)), dim3(MS_THREADS), 0, s, tris, T, (const int*)fflag, (const int*)cellid, used);
            if (int rc = nero_check_launch("nero_mesh_simplify_count: used cells")) return rc;
        }
        if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)used, upre, V + 1, s, "nero_mesh_simplify_count: used-cell scan failed")) return rc;
    }
    hipLaunchKernelGGL(ms_totals_kernel, dim3(1), dim3(64), 0, s, (const int*)fpre, T, (const int*)hpre, (const int*)upre, (int)V, full, hdr,
                       totals);
    return nero_check_launch("nero_mesh_simplify_count");
}

int nero_mesh_simplify_emit(const float* verts, const int* tris, int64_t T, int64_t V, double cell, const double* origin, int placement,
                            int dedup, void* ws, double* positions, float* verts_out, int64_t* cell_key, int64_t v_cap, int* tris_out,
                            int64_t t_cap, int* vmap, int* fmap, int64_t* n_tris, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_simplify_emit: V must be in [0, 2^31) and 3 T in [0, 2^31)");
    if (!ws || v_cap < 0 || t_cap < 0 || (V > 0 && !verts) || (T > 0 && !tris))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_emit: null pointer or negative capacity");
    if (!params_ok(cell, origin))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_emit: the cell must be positive and finite, the origin three finite numbers");
    if (placement != NERO_SIMPLIFY_MEAN && placement != NERO_SIMPLIFY_QUADRIC)
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_emit: unknown placement");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    const Layout L = layout(V, T);
    const MsParams p{cell, origin[0], origin[1], origin[2]};
    u64* hdr = (u64*)(w + L.hdr);
    // the one synchronisation: the totals nero_mesh_simplify_count left in the workspace, so that outputs that are too small, or input the
    // count refused, are an error code and not a write out of range
    long long h[H_WORDS];
    if (int rc = read_back(h, hdr, sizeof(h), s, "nero_mesh_simplify_emit: reading the totals of nero_mesh_simplify_count failed")) return rc;
    const int64_t V2 = h[H_VOUT], S = h[H_SURV], C = h[H_CELLS];
    if (h[H_FULL] != 1 || V2 < 0 || S < 0 || C < 0 || V2 > C || C > V || S > T)
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_emit: the workspace holds no complete totals of nero_mesh_simplify_count for this mesh");
    if (h[H_BADV] || h[H_BADT]) {
        static thread_local char msg[200];
        snprintf(msg, sizeof(msg), "nero_mesh_simplify_emit: the count refused %lld vertices (non-finite or outside 2^21 cells) and %lld "
                 "triangles (index out of range)", h[H_BADV], h[H_BADT]);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (V2 > v_cap || S > t_cap) {
        static thread_local char msg[200];
        snprintf(msg, sizeof(msg), "nero_mesh_simplify_emit: mesh of %lld vertices / %lld surviving triangles exceeds the capacity %lld / %lld",
                 (long long)V2, (long long)S, (long long)v_cap, (long long)t_cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if ((V2 > 0 && (!positions || !verts_out || !cell_key)) || (S > 0 && !tris_out))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_simplify_emit: null output pointer");
    const int* cellid = (const int*)(w + L.cellid);
    const int* used = (const int*)(w + L.used);
    const int* upre = (const int*)(w + L.upre);
    const int* fflag = (const int*)(w + L.fflag);
    const int* fpre = (const int*)(w + L.fpre);
    const int64_t n3 = 3 * T;
    if (V2 > 0) {
        unsigned* ckey_a = (unsigned*)(w + L.ckey_a);
        unsigned* ckey_b = (unsigned*)(w + L.ckey_b);
        unsigned* cval_a = (unsigned*)(w + L.cval_a);
        unsigned* cval_b = (unsigned*)(w + L.cval_b);
        int* cstart = (int*)(w + L.cstart);
        int* cend = (int*)(w + L.cend);
        const int quadric = placement == NERO_SIMPLIFY_QUADRIC;
        if (quadric) {                                               // (V' > 0: there is a survivor, T > 0)
            hipLaunchKernelGGL(ms_contrib_key_kernel, dim3(blocks_of(n3)), dim3(MS_THREADS), 0, s, tris, n3, (int)V, cellid, ckey_a, cval_a);
            if (int rc = nero_check_launch("nero_mesh_simplify_emit: contribution keys")) return rc;
            if (int rc = sort_pairs<unsigned>(w + L.temp, L.temp_bytes, ckey_a, ckey_b, cval_a, cval_b, n3, bit_length(V), s,
                                              "nero_mesh_simplify_emit: contribution sort failed"))
                return rc;
            if (hipMemsetAsync(cstart, 0, (size_t)(V + 1) * sizeof(int), s) != hipSuccess ||
                hipMemsetAsync(cend, 0, (size_t)(V + 1) * sizeof(int), s) != hipSuccess)
                return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_simplify_emit: hipMemsetAsync failed");
            hipLaunchKernelGGL(ms_contrib_range_kernel, dim3(blocks_of(n3)), dim3(MS_THREADS), 0, s, (const unsigned*)ckey_b, n3, cstart, cend);
            if (int rc = nero_check_launch("nero_mesh_simplify_emit: contribution runs")) return rc;
        }
        hipLaunchKernelGGL(ms_place_kernel, dim3(blocks_of(64 * C)), dim3(MS_THREADS), 0, s, verts, tris, (const u64*)(w + L.vkey_b),
                           (const unsigned*)(w + L.vval_b), (const int*)(w + L.vstart), (const unsigned*)cval_b, (const int*)cstart,
                           (const int*)cend, used, upre, C, p, quadric, positions, verts_out, (long long*)cell_key, v_cap);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: placement")) return rc;
    }
    if (V > 0 && vmap) {
        hipLaunchKernelGGL(ms_vmap_kernel, dim3(blocks_of(V)), dim3(MS_THREADS), 0, s, cellid, used, upre, (int)V, vmap);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: vertex map")) return rc;
    }
    const int* keep = nullptr;
    const int* opre = nullptr;
    if (dedup && S > 0) {
        u64* dkey_a = (u64*)(w + L.dkey_a);
        u64* dkey_b = (u64*)(w + L.dkey_b);
        unsigned* dval_a = (unsigned*)(w + L.dval_a);
        unsigned* dval_b = (unsigned*)(w + L.dval_b);
        unsigned* akey_a = (unsigned*)(w + L.akey_a);
        unsigned* akey_b = (unsigned*)(w + L.akey_b);
        unsigned* surv_t = (unsigned*)(w + L.surv_t);
        int* keep_w = (int*)(w + L.keep);
        int* opre_w = (int*)(w + L.opre);
        const int bits = bit_length(V2);
        hipLaunchKernelGGL(ms_triple_kernel, dim3(blocks_of(T)), dim3(MS_THREADS), 0, s, tris, T, fflag, fpre, cellid, upre, surv_t, dkey_a, dval_a);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: triples")) return rc;
        if (int rc = sort_pairs<u64>(w + L.temp, L.temp_bytes, dkey_a, dkey_b, dval_a, dval_b, S, 32 + bits, s, "nero_mesh_simplify_emit: first triple sort failed"))
            return rc;
        hipLaunchKernelGGL(ms_second_key_kernel, dim3(blocks_of(S)), dim3(MS_THREADS), 0, s, tris, (const unsigned*)dval_b, S,
                           (const unsigned*)surv_t, cellid, upre, akey_a);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: second keys")) return rc;
        if (int rc = sort_pairs<unsigned>(w + L.temp, L.temp_bytes, akey_a, akey_b, dval_b, dval_a, S, bits, s, "nero_mesh_simplify_emit: second triple sort failed"))
            return rc;
        hipLaunchKernelGGL(ms_first_kernel, dim3(blocks_of(S + 1)), dim3(MS_THREADS), 0, s, tris, (const unsigned*)dval_a, S,
                           (const unsigned*)surv_t, cellid, upre, keep_w);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: first of each triple")) return rc;
        if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)keep_w, opre_w, S + 1, s, "nero_mesh_simplify_emit: output scan failed")) return rc;
        keep = keep_w;
        opre = opre_w;
    }
    if (T > 0 && (S > 0 || fmap)) {
        hipLaunchKernelGGL(ms_emit_tris_kernel, dim3(blocks_of(T)), dim3(MS_THREADS), 0, s, tris, T, fflag, fpre, cellid, upre, keep, opre,
                           tris_out, t_cap, fmap);
        if (int rc = nero_check_launch("nero_mesh_simplify_emit: triangles")) return rc;
    }
    hipLaunchKernelGGL(ms_final_kernel, dim3(1), dim3(64), 0, s, opre, S, hdr, n_tris);
    return nero_check_launch("nero_mesh_simplify_emit");
}
