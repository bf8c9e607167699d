// mesh_clean.hip -- connected components of the extracted Stage-I mesh and the removal of the unwanted ones (include/nero_hip.h,
// nero_mesh_*).  The marching-cubes surface of a learned SDF holds floaters, hidden inner shells and scraps of the support surface; the
// reference leaves them to a mesh editor.  Three steps, all on the mesh where nero_mcubes_emit left it:
//   label    concurrent union-find over the triangle edges (device_prims.h: why it is correct under stale loads and incoherent L2
//            caches): every triangle unites its vertices.  A second launch, behind the kernel boundary, points every vertex at its root and
//            counts the roots.  The labels are the smallest vertex of each component whatever order the atomics landed in.
//   stats    components numbered by a prefix sum over the root flags (ascending smallest vertex); vertex / face counts and boxes by integer
//            atomics (sums and extrema of integers do not depend on arrival order), one per wave and component; areas by a stable radix
//            sort of the faces by component and a fixed two-level float64 sum per component (no float atomics).
//   compact  flags of the surviving faces and of the vertices they use, exclusive scans, the 16-byte totals, and an emit pass: the
//            survivors keep their relative order.
// Work and traffic are linear in V + T (the union-find's inverse-Ackermann factor aside), whatever the diameter of the mesh graph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip.h"
#include "common.h"
#include "cub_calls.h"
#include "device_prims.h"
#include "ws_plan.h"

namespace {

using namespace nero_cub;
using namespace nero_prims;
using namespace nero_ws;

constexpr int CC_THREADS = 256;
constexpr int CC_PIECE = 2048;                                      // faces a wave sums into one partial area
constexpr int64_t CC_MAX_ITEMS = ((int64_t)1 << 31) - 1;           // V, T < 2^31: int32 ids, int item counts of hipCUB

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(int* __restrict__ parent, int V) {
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (v < V) parent[v] = (int)v;
}

__global__ __launch_bounds__(CC_THREADS) void cc_hook_kernel(const int* __restrict__ tris, int64_t T, int V, int* parent,
                                                             unsigned long long* info) {
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (t >= T) return;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    if (!(in_range(a, V) && in_range(b, V) && in_range(c, V))) {
        atomicAdd(info + 1, 1ull);                                   // reported by the call; the triangle is never dereferenced
        return;
    }
    if (a != b) uf_unite(parent, a, b);
    if (b != c) uf_unite(parent, b, c);
}

// after the kernel boundary: every store of the hook pass is visible.  Vertices that are rewritten while another lane walks through them
// go from one ancestor to another (the root), so the walk still ends at the root.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* parent, int V, unsigned long long* info) {
    __shared__ int part[CC_THREADS / 64];
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    int is_root = 0;
    if (v < V) {
        int r = (int)v, p = parent[r];
        while (p != r) {
            r = p;
            p = parent[r];
        }
        is_root = r == (int)v;
        if (!is_root) parent[v] = r;
    }
    const int n = block_sum<CC_THREADS>(is_root, part);
    if (threadIdx.x == 0 && n) atomicAdd(info, (unsigned long long)n);
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_rootflag_kernel(const int* __restrict__ label, int V, int* __restrict__ flag) {
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (v < V) flag[v] = label[v] == (int)v;
    else if (v == V) flag[v] = 0;                                    // the scan's trailing entry: rank[V] = K
}

// comp[v] = rank of v's root; vertex counts and boxes.  A label outside [0, V) (not written by nero_mesh_cc_label) gives comp -1.
__global__ __launch_bounds__(CC_THREADS) void cc_vertex_kernel(const float* __restrict__ verts, const int* __restrict__ label,
                                                               const int* __restrict__ rank, int V, int K, int* __restrict__ comp,
                                                               int* n_verts, unsigned* bmin, unsigned* bmax) {
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    int c = -1;
    unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
    if (v < V) {
        const int r = label[v];
        if (in_range(r, V)) {
            c = rank[r];
            if (!in_range(c, K)) c = -1;
        }
        comp[v] = c;
        if (c >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a] = hi[a] = f2o(verts[3 * v + a]);
        }
    }
    const int lane = threadIdx.x & 63;
    for (unsigned long long todo = __ballot(c >= 0); todo;) {
        int cl, leader;
        const unsigned long long m = next_group(c, todo, &cl, &leader);
        todo &= ~m;
        unsigned l[3], h[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            l[a] = lo[a];
            h[a] = hi[a];
        }
        if (m & (m - 1)) {                                           // (wave-uniform) more than one lane: their extrema first
            const bool mine = (m >> lane) & 1;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                l[a] = wave_min(mine ? lo[a] : 0xFFFFFFFFu);
                h[a] = wave_max(mine ? hi[a] : 0u);
            }
        }
        if (lane == leader) {
            atomicAdd(n_verts + cl, __popcll(m));
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                atomicMin(bmin + 3 * (int64_t)cl + a, l[a]);
                atomicMax(bmax + 3 * (int64_t)cl + a, h[a]);
            }
        }
    }
}

// sort key of a face = the component of its first vertex (K for a triangle with an index out of range: behind every component)
__global__ __launch_bounds__(CC_THREADS) void cc_face_kernel(const int* __restrict__ tris, int64_t T, int V, int K,
                                                             const int* __restrict__ comp, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ val, int* n_faces) {
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    int c = -1;
    if (t < T) {
        const int a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
        if (in_range(a, V) && in_range(b, V) && in_range(d, V)) c = comp[a];
        key[t] = c >= 0 ? (unsigned)c : (unsigned)K;
        val[t] = (unsigned)t;
    }
    for (unsigned long long todo = __ballot(c >= 0); todo;) {
        int cl, leader;
        const unsigned long long m = next_group(c, todo, &cl, &leader);
        todo &= ~m;
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(n_faces + cl, __popcll(m));
    }
}

// The area of a component is summed in two fixed levels, so that it is the same bits every run and a component of millions of faces is
// not one workgroup's job: the sorted faces of a component are cut into pieces of CC_PIECE; a wave sums a piece (each lane its faces in
// ascending order, then a butterfly), and a wave sums the pieces of a component the same way.  pbase[c] = first piece of component c.
struct CcPieces {
    __host__ __device__ int operator()(int n) const { return (n + CC_PIECE - 1) / CC_PIECE; }
};

__device__ __forceinline__ double cc_face_area(const float* __restrict__ verts, const int* __restrict__ tris, int64_t t) {
    const float* pa = verts + 3 * (int64_t)tris[3 * t];
    const float* pb = verts + 3 * (int64_t)tris[3 * t + 1];
    const float* pc = verts + 3 * (int64_t)tris[3 * t + 2];
    const double ax = pa[0], ay = pa[1], az = pa[2];
    const double ux = (double)pb[0] - ax, uy = (double)pb[1] - ay, uz = (double)pb[2] - az;
    const double wx = (double)pc[0] - ax, wy = (double)pc[1] - ay, wz = (double)pc[2] - az;
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    return 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
}

// one wave per piece.  face = the face ids sorted by component (only faces that passed the range check lie below offsets[K]).
__global__ __launch_bounds__(CC_THREADS) void cc_area_piece_kernel(const float* __restrict__ verts, const int* __restrict__ tris,
                                                                   const unsigned* __restrict__ face, const int* __restrict__ offsets,
                                                                   const int* __restrict__ pbase, int K, double* __restrict__ partial) {
    const int64_t p = (int64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
    if (p >= pbase[K]) return;
    int lo = 0, hi = K;                                              // the last component whose first piece is not behind p
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (pbase[mid] <= p) lo = mid; else hi = mid;
    }
    const int64_t begin = offsets[lo] + (p - pbase[lo]) * CC_PIECE;
    const int64_t end = begin + CC_PIECE < offsets[lo + 1] ? begin + CC_PIECE : offsets[lo + 1];
    double s = 0.0;
    for (int64_t i = begin + (threadIdx.x & 63); i < end; i += 64) s += cc_face_area(verts, tris, face[i]);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) partial[p] = s;
}

// one wave per component
__global__ __launch_bounds__(CC_THREADS) void cc_area_sum_kernel(const double* __restrict__ partial, const int* __restrict__ pbase, int K,
                                                                 double* __restrict__ area) {
    const int64_t c = (int64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
    if (c >= K) return;
    double s = 0.0;
    for (int64_t i = pbase[c] + (threadIdx.x & 63); i < pbase[c + 1]; i += 64) s += partial[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) area[c] = s;
}

__global__ __launch_bounds__(CC_THREADS) void cc_box_decode_kernel(unsigned* bmin, unsigned* bmax, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (i >= n) return;
    ((float*)bmin)[i] = o2f(bmin[i]);
    ((float*)bmax)[i] = o2f(bmax[i]);
}

// ---- compaction -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void cc_mark_kernel(const int* __restrict__ tris, int64_t T, int V, int K,
                                                             const int* __restrict__ comp, const unsigned char* __restrict__ keep,
                                                             int* __restrict__ fflag, int* vflag) {
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (t > T) return;
    int k = 0;
    if (t < T) {
        const int a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
        if (in_range(a, V) && in_range(b, V) && in_range(d, V)) {
            const int c = comp[a];
            if (in_range(c, K) && keep[c]) {
                k = 1;
                vflag[a] = 1;                                        // (every writer stores the same value)
                vflag[b] = 1;
                vflag[d] = 1;
            }
        }
    }
    fflag[t] = k;                                                    // t == T: the scan's trailing entry
}

__global__ void cc_totals_kernel(const int* __restrict__ vpre, const int* __restrict__ fpre, int V, int64_t T, int64_t* __restrict__ hdr,
                                 int64_t* __restrict__ totals) {
    const int q = threadIdx.x;
    if (q < 2) {
        const int64_t x = q == 0 ? vpre[V] : fpre[T];
        hdr[q] = x;
        if (totals) totals[q] = x;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_verts_kernel(const float* __restrict__ verts, const int* __restrict__ vflag,
                                                                   const int* __restrict__ vpre, int V, float* __restrict__ out,
                                                                   int64_t v_cap, int* __restrict__ vmap) {
    const int64_t v = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (v >= V) return;
    const int64_t o = vflag[v] ? vpre[v] : -1;
    if (vmap) vmap[v] = (int)o;
    if (o >= 0 && o < v_cap) {
        out[3 * o] = verts[3 * v];
        out[3 * o + 1] = verts[3 * v + 1];
        out[3 * o + 2] = verts[3 * v + 2];
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_emit_tris_kernel(const int* __restrict__ tris, const int* __restrict__ fflag,
                                                                  const int* __restrict__ fpre, const int* __restrict__ vpre, int64_t T,
                                                                  int* __restrict__ out, int64_t t_cap) {
    const int64_t t = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (t >= T || !fflag[t]) return;                                 // (a flagged face passed the range check of the mark pass)
    const int64_t o = fpre[t];
    if (o >= t_cap) return;
    out[3 * o] = vpre[tris[3 * t]];
    out[3 * o + 1] = vpre[tris[3 * t + 1]];
    out[3 * o + 2] = vpre[tris[3 * t + 2]];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= CC_MAX_ITEMS && T <= CC_MAX_ITEMS; }

struct StatsLayout {
    size_t rank, tmp, pbase, key_a, key_b, val_a, val_b, partial, temp, temp_bytes, total;
};

int64_t max_pieces(int64_t V, int64_t T) { return T / CC_PIECE + V + 1; }     // (every component with a face: one piece that is not full)

int stats_layout(int64_t V, int64_t T, StatsLayout* w) {
    size_t a = 0, b = 0;
    if (scan_temp<int>(V + 1, &a) != hipSuccess || sort_pairs_temp<unsigned>(T, 32, &b) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_cc_stats: the scratch-size query of the rank scan or the face sort failed");
    Carve c;
    const size_t vi = (size_t)(V + 1) * sizeof(int), ti = (size_t)T * sizeof(unsigned);
    w->rank = c.take(vi);
    w->tmp = c.take(vi);                                             // the root flags, then the face offsets of the components
    w->pbase = c.take(vi);
    w->key_a = c.take(ti);
    w->key_b = c.take(ti);
    w->val_a = c.take(ti);
    w->val_b = c.take(ti);
    w->partial = c.take((size_t)max_pieces(V, T) * sizeof(double));
    w->temp_bytes = a > b ? a : b;
    w->temp = c.take(w->temp_bytes);
    w->total = c.at;
    return NERO_OK;
}

struct CompactLayout {
    size_t hdr, vflag, vpre, fflag, fpre, temp, temp_bytes, total;
};

int compact_layout(int64_t V, int64_t T, CompactLayout* w) {
    size_t a = 0, b = 0;
    if (scan_temp<int>(V + 1, &a) != hipSuccess || scan_temp<int>(T + 1, &b) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_compact: the scratch-size query of the vertex or the triangle scan failed");
    Carve c;
    const size_t vi = (size_t)(V + 1) * sizeof(int), ti = (size_t)(T + 1) * sizeof(int);
    w->hdr = c.take(256);                                            // header: int64 {V', T'}
    w->vflag = c.take(vi);
    w->vpre = c.take(vi);
    w->fflag = c.take(ti);
    w->fpre = c.take(ti);
    w->temp_bytes = a > b ? a : b;
    w->temp = c.take(w->temp_bytes);
    w->total = c.at;
    return NERO_OK;
}

}  // namespace

int nero_mesh_cc_label(const int* tris, int64_t T, int64_t V, int* label, int64_t* info, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_cc_label: V and T must be in [0, 2^31)");
    if (!info || (V > 0 && !label) || (T > 0 && !tris)) return nero_fail(NERO_ERR_ARG, "nero_mesh_cc_label: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(info, 0, 2 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_cc_label: hipMemsetAsync failed");
    unsigned long long* inf = (unsigned long long*)info;
    if (V > 0) {
        hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_of(V)), dim3(CC_THREADS), 0, s, label, (int)V);
        if (int rc = nero_check_launch("nero_mesh_cc_label: init")) return rc;
    }
    if (T > 0) {                                                    // (V == 0: every triangle is out of range)
        hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_of(T)), dim3(CC_THREADS), 0, s, tris, T, (int)V, label, inf);
        if (int rc = nero_check_launch("nero_mesh_cc_label: hook pass")) return rc;
    }
    if (V > 0) {
        hipLaunchKernelGGL(cc_flatten_kernel, dim3(blocks_of(V)), dim3(CC_THREADS), 0, s, label, (int)V, inf);
        if (int rc = nero_check_launch("nero_mesh_cc_label: flatten pass")) return rc;
    }
    return NERO_OK;
}

size_t nero_mesh_cc_stats_workspace_bytes(int64_t V, int64_t T) {
    if (!sizes_ok(V, T)) return no_workspace("nero_mesh_cc_stats_workspace_bytes: V and T must be in [0, 2^31)");
    StatsLayout L;
    return stats_layout(V, T, &L) == NERO_OK ? L.total : 0;
}

int nero_mesh_cc_stats(const float* verts, const int* tris, int64_t T, int64_t V, const int* label, int64_t K, void* ws, int* comp,
                       int* n_verts, int* n_faces, double* area, float* bbox_min, float* bbox_max, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_cc_stats: V and T must be in [0, 2^31)");
    if (K < 0 || K > V || (V > 0 && K == 0)) return nero_fail(NERO_ERR_ARG, "nero_mesh_cc_stats: K is not the component count of V vertices");
    if (V == 0) return NERO_OK;
    if (!verts || !label || !ws || !comp || !n_verts || !n_faces || !area || !bbox_min || !bbox_max || (T > 0 && !tris))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_cc_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    StatsLayout L;
    if (int rc = stats_layout(V, T, &L)) return rc;
    int* rank = (int*)(w + L.rank);
    int* tmp = (int*)(w + L.tmp);
    if (hipMemsetAsync(n_verts, 0, (size_t)K * sizeof(int), s) != hipSuccess ||
        hipMemsetAsync(n_faces, 0, (size_t)K * sizeof(int), s) != hipSuccess ||
        hipMemsetAsync(area, 0, (size_t)K * sizeof(double), s) != hipSuccess ||
        hipMemsetAsync(bbox_min, 0xFF, (size_t)K * 3 * sizeof(float), s) != hipSuccess ||
        hipMemsetAsync(bbox_max, 0, (size_t)K * 3 * sizeof(float), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_cc_stats: hipMemsetAsync failed");
    hipLaunchKernelGGL(cc_rootflag_kernel, dim3(blocks_of(V + 1)), dim3(CC_THREADS), 0, s, label, (int)V, tmp);
    if (int rc = nero_check_launch("nero_mesh_cc_stats: root flags")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)tmp, rank, V + 1, s, "nero_mesh_cc_stats: rank scan failed")) return rc;
    hipLaunchKernelGGL(cc_vertex_kernel, dim3(blocks_of(V)), dim3(CC_THREADS), 0, s, verts, label, (const int*)rank, (int)V, (int)K, comp,
                       n_verts, (unsigned*)bbox_min, (unsigned*)bbox_max);
    if (int rc = nero_check_launch("nero_mesh_cc_stats: vertex pass")) return rc;
    hipLaunchKernelGGL(cc_box_decode_kernel, dim3(blocks_of(3 * K)), dim3(CC_THREADS), 0, s, (unsigned*)bbox_min, (unsigned*)bbox_max, 3 * K);
    if (int rc = nero_check_launch("nero_mesh_cc_stats: box decode")) return rc;
    if (T == 0) return NERO_OK;
    unsigned* key_a = (unsigned*)(w + L.key_a);
    unsigned* key_b = (unsigned*)(w + L.key_b);
    unsigned* val_a = (unsigned*)(w + L.val_a);
    unsigned* val_b = (unsigned*)(w + L.val_b);
    int* pbase = (int*)(w + L.pbase);
    double* partial = (double*)(w + L.partial);
    hipLaunchKernelGGL(cc_face_kernel, dim3(blocks_of(T)), dim3(CC_THREADS), 0, s, tris, T, (int)V, (int)K, (const int*)comp, key_a, val_a,
                       n_faces);
    if (int rc = nero_check_launch("nero_mesh_cc_stats: face pass")) return rc;
    // offsets[c] = first sorted face of component c, offsets[K] = the faces that belong to a component; pbase likewise for the pieces
    if (hipMemsetAsync(tmp, 0, sizeof(int), s) != hipSuccess || hipMemsetAsync(pbase, 0, sizeof(int), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_cc_stats: hipMemsetAsync failed");
    if (int rc = inclusive_sum(w + L.temp, L.temp_bytes, (const int*)n_faces, tmp + 1, K, s, "nero_mesh_cc_stats: offset scan failed")) return rc;
    hipcub::TransformInputIterator<int, CcPieces, const int*> pieces((const int*)n_faces, CcPieces());
    if (int rc = inclusive_sum(w + L.temp, L.temp_bytes, pieces, pbase + 1, K, s, "nero_mesh_cc_stats: piece scan failed")) return rc;
    if (int rc = sort_pairs<unsigned>(w + L.temp, L.temp_bytes, key_a, key_b, val_a, val_b, T, bit_length(K), s,
                                      "nero_mesh_cc_stats: face sort failed"))
        return rc;
    const int64_t waves = T / CC_PIECE + K;                          // at least as many as there are pieces
    hipLaunchKernelGGL(cc_area_piece_kernel, dim3(blocks_of(64 * waves)), dim3(CC_THREADS), 0, s, verts, tris, (const unsigned*)val_b,
                       (const int*)tmp, (const int*)pbase, (int)K, partial);
    if (int rc = nero_check_launch("nero_mesh_cc_stats: area pass")) return rc;
    hipLaunchKernelGGL(cc_area_sum_kernel, dim3(blocks_of(64 * K)), dim3(CC_THREADS), 0, s, (const double*)partial, (const int*)pbase, (int)K,
                       area);
    return nero_check_launch("nero_mesh_cc_stats: area sum");
}

size_t nero_mesh_compact_workspace_bytes(int64_t V, int64_t T) {
    if (!sizes_ok(V, T)) return no_workspace("nero_mesh_compact_workspace_bytes: V and T must be in [0, 2^31)");
    CompactLayout L;
    return compact_layout(V, T, &L) == NERO_OK ? L.total : 0;
}

int nero_mesh_compact_count(const int* tris, int64_t T, int64_t V, const int* comp, const unsigned char* keep, int64_t K, void* ws,
                            int64_t* totals, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_compact_count: V and T must be in [0, 2^31)");
    if (K < 0 || K > V) return nero_fail(NERO_ERR_ARG, "nero_mesh_compact_count: K outside [0, V]");
    if (!ws || !totals || (V > 0 && !comp) || (K > 0 && !keep) || (T > 0 && !tris))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_compact_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    CompactLayout L;
    if (int rc = compact_layout(V, T, &L)) return rc;
    int* vflag = (int*)(w + L.vflag);
    int* fflag = (int*)(w + L.fflag);
    if (hipMemsetAsync(vflag, 0, (size_t)(V + 1) * sizeof(int), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_compact_count: hipMemsetAsync failed");
    hipLaunchKernelGGL(cc_mark_kernel, dim3(blocks_of(T + 1)), dim3(CC_THREADS), 0, s, tris, T, (int)V, (int)K, comp, keep, fflag, vflag);
    if (int rc = nero_check_launch("nero_mesh_compact_count: mark pass")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)vflag, (int*)(w + L.vpre), V + 1, s,
                               "nero_mesh_compact_count: vertex scan failed"))
        return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)fflag, (int*)(w + L.fpre), T + 1, s,
                               "nero_mesh_compact_count: triangle scan failed"))
        return rc;
    hipLaunchKernelGGL(cc_totals_kernel, dim3(1), dim3(64), 0, s, (const int*)(w + L.vpre), (const int*)(w + L.fpre), (int)V, T,
                       (int64_t*)(w + L.hdr), totals);
    return nero_check_launch("nero_mesh_compact_count");
}

int nero_mesh_compact_emit(const float* verts, const int* tris, int64_t T, int64_t V, void* ws, float* verts_out, int64_t v_cap, int* tris_out,
                           int64_t t_cap, int* vmap, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_compact_emit: V and T must be in [0, 2^31)");
    if (!ws || v_cap < 0 || t_cap < 0 || (V > 0 && !verts) || (T > 0 && !tris))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_compact_emit: null pointer or negative capacity");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    CompactLayout L;
    if (int rc = compact_layout(V, T, &L)) return rc;
    // the one synchronisation: the totals nero_mesh_compact_count left in the workspace, so that outputs that are too small are an error
    // code and not a write out of range
    int64_t tot[2] = {-1, -1};
    if (int rc = read_back(tot, w + L.hdr, sizeof(tot), s, "nero_mesh_compact_emit: reading the totals of nero_mesh_compact_count failed")) return rc;
    const int64_t V2 = tot[0], T2 = tot[1];
    if (V2 < 0 || T2 < 0 || V2 > V || T2 > T)
        return nero_fail(NERO_ERR_ARG, "nero_mesh_compact_emit: the workspace holds no totals of nero_mesh_compact_count for this mesh");
    if (V2 > v_cap || T2 > t_cap) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_mesh_compact_emit: mesh of %lld vertices / %lld triangles exceeds the capacity %lld / %lld",
                 (long long)V2, (long long)T2, (long long)v_cap, (long long)t_cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if ((V2 > 0 && !verts_out) || (T2 > 0 && !tris_out)) return nero_fail(NERO_ERR_ARG, "nero_mesh_compact_emit: null output pointer");
    if (V > 0) {
        hipLaunchKernelGGL(cc_emit_verts_kernel, dim3(blocks_of(V)), dim3(CC_THREADS), 0, s, verts, (const int*)(w + L.vflag),
                           (const int*)(w + L.vpre), (int)V, verts_out, v_cap, vmap);
        if (int rc = nero_check_launch("nero_mesh_compact_emit: vertex pass")) return rc;
    }
    if (T2 > 0) {
        hipLaunchKernelGGL(cc_emit_tris_kernel, dim3(blocks_of(T)), dim3(CC_THREADS), 0, s, tris, (const int*)(w + L.fflag),
                           (const int*)(w + L.fpre), (const int*)(w + L.vpre), T, tris_out, t_cap);
        if (int rc = nero_check_launch("nero_mesh_compact_emit: triangle pass")) return rc;
    }
    return NERO_OK;
}
