// mesh_atlas.hip -- the projection atlas of the Stage-II asset export (include/nero_hip.h, nero_mesh_face_adjacency / nero_mesh_chart_*):
// the UV unwrap the texture bake (texture.hip) starts from, which the reference takes from xatlas.  Charts are edge-connected sets of faces
// whose normals share a dominant signed axis; each is projected along that axis at one world-to-texel scale.  The definition is DESIGN.md
// 9.7.1; tests/mesh_atlas_ref.py restates it in numpy.  Steps, each on the mesh where the clean-up / simplification left it:
//   adjacency  the 3T edges (min << 32 | max) of the valid faces, stable radix sort, and a look at the two entries behind every group head:
//              a key held exactly twice joins two faces, once is a boundary edge, three times or more a non-manifold edge.
//   label      class of every face from its float64 normal; the concurrent union-find of device_prims.h over FACES (a chart's root is its
//              smallest face whatever order the atomics land in; flatten behind the kernel boundary); charts numbered by a prefix sum over
//              the root flags.
//   stats      class, face count and the exact fp32 box of the two projected coordinates per chart: integer atomics on order-preserving
//              bit images, one per wave and chart.
//   corners    one UV vertex per (chart, mesh vertex) pair: stable sort of the 3T corner keys, head flags, a scan; two-phase, the totals
//              read back once in emit.
//   uv         U, V of every UV vertex from the packed chart origins (host) and the scale: float64, no fused multiply-add.
// No floating-point atomics and no atomic that decides a position or a label: every output is bit-identical run to run.
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

constexpr int AT_THREADS = 256;
constexpr int64_t AT_MAX_ITEMS = ((int64_t)1 << 31) - 1;           // V, 3T < 2^31: int32 ids, int item counts of hipCUB
constexpr unsigned long long AT_NO_KEY = ~0ull;                    // sorts behind every real key (a real key's high word is < 2^31)
constexpr int AT_MAX_SIZE = 16384;

__device__ __forceinline__ bool at_valid_face(int a, int b, int c, int V) {
    return in_range(a, V) && in_range(b, V) && in_range(c, V) && a != b && b != c && c != a;
}

// ---- adjacency --------------------------------------------------------------------------------------------------------------------------
// one lane per corner i = 3 t + e: the key of the edge (v_e, v_(e+1)%3), AT_NO_KEY for the corners of a face that is not valid
__global__ __launch_bounds__(AT_THREADS) void at_edge_key_kernel(const int* __restrict__ tris, int64_t n3, int V,
                                                                 unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= n3) return;
    const int64_t t = i / 3;
    const int e = (int)(i - 3 * t);
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    unsigned long long k = AT_NO_KEY;
    if (at_valid_face(a, b, c, V)) {
        const int p = e == 0 ? a : (e == 1 ? b : c), q = e == 0 ? b : (e == 1 ? c : a);
        const unsigned lo = (unsigned)(p < q ? p : q), hi = (unsigned)(p < q ? q : p);
        k = ((unsigned long long)lo << 32) | hi;
    }
    key[i] = k;
    val[i] = (unsigned)i;
}

// one lane per sorted entry; the head of a group decides for the group.  nbr was set to -1 beforehand.
__global__ __launch_bounds__(AT_THREADS) void at_edge_group_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                                                   int64_t n3, int* __restrict__ nbr, unsigned long long* counts) {
    __shared__ int part[AT_THREADS / 64];
    const int64_t j = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    int boundary = 0, nonmanifold = 0;
    if (j < n3) {
        const unsigned long long k = key[j];
        if (k != AT_NO_KEY && (j == 0 || key[j - 1] != k)) {
            const bool two = j + 1 < n3 && key[j + 1] == k;
            const bool three = two && j + 2 < n3 && key[j + 2] == k;
            if (!two) {
                boundary = 1;
            } else if (three) {
                nonmanifold = 1;
            } else {
                const unsigned c0 = val[j], c1 = val[j + 1];
                if (c0 / 3 != c1 / 3) {
                    nbr[c0] = (int)(c1 / 3);
                    nbr[c1] = (int)(c0 / 3);
                } else {
                    nonmanifold = 1;                                 // (cannot happen: the three edges of a valid face have three keys)
                }
            }
        }
    }
    const int nb = block_sum<AT_THREADS>(boundary, part);
    const int nm = block_sum<AT_THREADS>(nonmanifold, part);
    if (threadIdx.x == 0) {
        if (nb) atomicAdd(counts, (unsigned long long)nb);
        if (nm) atomicAdd(counts + 1, (unsigned long long)nm);
    }
}

// ---- classes and charts -----------------------------------------------------------------------------------------------------------------
// 2 k + (n_k < 0), k = argmax |n_k| with ties to the lowest axis; 6 = chartless.  Every product and difference is rounded on its own.
__device__ __forceinline__ int at_face_class(const float* __restrict__ verts, int a, int b, int c) {
#pragma clang fp contract(off)
    const float* pa = verts + 3 * (int64_t)a;
    const float* pb = verts + 3 * (int64_t)b;
    const float* pc = verts + 3 * (int64_t)c;
    const double ax = pa[0], ay = pa[1], az = pa[2];
    const double ux = (double)pb[0] - ax, uy = (double)pb[1] - ay, uz = (double)pb[2] - az;
    const double wx = (double)pc[0] - ax, wy = (double)pc[1] - ay, wz = (double)pc[2] - az;
    const double p0 = uy * wz, p1 = uz * wy, p2 = uz * wx, p3 = ux * wz, p4 = ux * wy, p5 = uy * wx;
    const double n[3] = {p0 - p1, p2 - p3, p4 - p5};
    if (!(isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]))) return 6;
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return 6;
    int k = 0;
    if (fabs(n[1]) > fabs(n[0])) k = 1;
    if (fabs(n[2]) > fabs(n[k])) k = 2;
    return 2 * k + (n[k] < 0.0 ? 1 : 0);
}

__global__ __launch_bounds__(AT_THREADS) void at_class_kernel(const float* __restrict__ verts, const int* __restrict__ tris, int64_t T, int V,
                                                              int* __restrict__ face_class, int* __restrict__ parent, unsigned long long* info) {
    __shared__ int part[AT_THREADS / 64];
    const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    int chartless = 0;
    if (t < T) {
        const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
        const int cls = at_valid_face(a, b, c, V) ? at_face_class(verts, a, b, c) : 6;
        face_class[t] = cls;
        parent[t] = (int)t;
        chartless = cls == 6;
    }
    const int n = block_sum<AT_THREADS>(chartless, part);
    if (threadIdx.x == 0 && n) atomicAdd(info + 1, (unsigned long long)n);
}

// face_class is complete here (the launch before).  Every pair is joined from its smaller face; a neighbour entry that is not a face of
// this mesh (nbr not written by nero_mesh_face_adjacency) is never followed.  uf_unite: the union-find of device_prims.h, over faces.
__global__ __launch_bounds__(AT_THREADS) void at_hook_kernel(const int* __restrict__ nbr, const int* __restrict__ face_class, int64_t T,
                                                             int* parent) {
    const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (t >= T) return;
    const int cls = face_class[t];
    if (cls >= 6) return;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const int n = nbr[3 * t + e];
        if (n > (int)t && n < T && face_class[n] == cls) uf_unite(parent, (int)t, n);
    }
}

// behind the kernel boundary: every store of the hook pass is visible.  flag[t] = t is the root of a chart; flag[T] = 0 for the scan.
__global__ __launch_bounds__(AT_THREADS) void at_flatten_kernel(int* parent, const int* __restrict__ face_class, int64_t T, int* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (t > T) return;
    int is_root = 0;
    if (t < T) {
        int r = (int)t, p = parent[r];
        while (p != r) {
            r = p;
            p = parent[r];
        }
        is_root = r == (int)t && face_class[t] < 6;
        if (r != (int)t) parent[t] = r;
    }
    flag[t] = is_root;
}

// in place: chart[t] holds the root of t and becomes the rank of that root (lane t reads no other entry of chart[])
__global__ __launch_bounds__(AT_THREADS) void at_number_kernel(int* chart, const int* __restrict__ face_class, const int* __restrict__ rank, int64_t T,
                                                               unsigned long long* info) {
    const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (t == 0) info[0] = (unsigned long long)rank[T];
    if (t >= T) return;
    chart[t] = face_class[t] < 6 ? rank[chart[t]] : -1;
}

// ---- statistics -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AT_THREADS) void at_stats_init_kernel(int* __restrict__ chart_class, int* __restrict__ n_faces, unsigned* __restrict__ box,
                                                                   int K) {
    const int64_t c = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (c >= K) return;
    chart_class[c] = 6;
    n_faces[c] = 0;
    box[4 * c] = box[4 * c + 1] = 0xFFFFFFFFu;
    box[4 * c + 2] = box[4 * c + 3] = 0u;
}

// one atomic per wave and chart, not per lane: a smooth surface is a handful of charts that hold every face.  A chart, class or vertex index
// out of range (inputs not written by nero_mesh_chart_label) leaves the face out.
__global__ __launch_bounds__(AT_THREADS) void at_stats_kernel(const float* __restrict__ verts, const int* __restrict__ tris, int64_t T, int V,
                                                              const int* __restrict__ chart, const int* __restrict__ face_class, int K,
                                                              int* chart_class, int* n_faces, unsigned* box) {
    const int64_t t = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    int c = -1;
    unsigned lo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, hi[2] = {0u, 0u};
    if (t < T) {
        const int cc = chart[t], cls = face_class[t];
        const int v[3] = {tris[3 * t], tris[3 * t + 1], tris[3 * t + 2]};
        if (in_range(cc, K) && in_range(cls, 6) && at_valid_face(v[0], v[1], v[2], V)) {
            c = cc;
            const int k = cls >> 1, ax[2] = {(k + 1) % 3, (k + 2) % 3};
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const unsigned o = f2o(verts[3 * (int64_t)v[j] + ax[d]]);
                    lo[d] = o < lo[d] ? o : lo[d];
                    hi[d] = o > hi[d] ? o : hi[d];
                }
            chart_class[c] = cls;                                    // (every writer of a chart stores the same value)
        }
    }
    const int lane = threadIdx.x & 63;
    for (unsigned long long todo = __ballot(c >= 0); todo;) {
        int cl, leader;
        const unsigned long long m = next_group(c, todo, &cl, &leader);
        todo &= ~m;
        unsigned l[2] = {lo[0], lo[1]}, h[2] = {hi[0], hi[1]};
        if (m & (m - 1)) {                                           // (wave-uniform) more than one lane: their extrema first
            const bool mine = (m >> lane) & 1;
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                l[d] = wave_min(mine ? lo[d] : 0xFFFFFFFFu);
                h[d] = wave_max(mine ? hi[d] : 0u);
            }
        }
        if (lane == leader) {
            atomicAdd(n_faces + cl, __popcll(m));
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                atomicMin(box + 4 * (int64_t)cl + d, l[d]);
                atomicMax(box + 4 * (int64_t)cl + 2 + d, h[d]);
            }
        }
    }
}

__global__ __launch_bounds__(AT_THREADS) void at_box_decode_kernel(unsigned* box, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i < n) ((float*)box)[i] = o2f(box[i]);
}

// ---- UV vertices ------------------------------------------------------------------------------------------------------------------------
// one lane per corner i = 3 t + e: chart << 32 | vertex, AT_NO_KEY for the corners of a chartless face
__global__ __launch_bounds__(AT_THREADS) void at_corner_key_kernel(const int* __restrict__ tris, int64_t n3, int V, const int* __restrict__ chart,
                                                                   int K, unsigned long long* __restrict__ key, unsigned* __restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= n3) return;
    const int64_t t = i / 3;
    const int c = chart[t];
    const int a = tris[3 * t], b = tris[3 * t + 1], d = tris[3 * t + 2];
    unsigned long long k = AT_NO_KEY;
    if (in_range(c, K) && at_valid_face(a, b, d, V)) k = ((unsigned long long)(unsigned)c << 32) | (unsigned)tris[i];
    key[i] = k;
    val[i] = (unsigned)i;
}

__global__ __launch_bounds__(AT_THREADS) void at_corner_head_kernel(const unsigned long long* __restrict__ key, int64_t n3, int* __restrict__ head) {
    const int64_t j = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (j > n3) return;
    head[j] = j < n3 && key[j] != AT_NO_KEY && (j == 0 || key[j - 1] != key[j]) ? 1 : 0;        // head[n3] = 0: the scan's trailing entry
}

struct AtCornerHeader {           // first 256 bytes of the corner workspace
    int64_t n_vt;                 // distinct (chart, vertex) pairs, plus one when a face is chartless
    int64_t n_pairs;              // distinct (chart, vertex) pairs
    int64_t n_charted;            // corners of charted faces = the first sorted entry that holds AT_NO_KEY
    int64_t n3;                   // the corners the count was made for
};

__global__ void at_corner_totals_kernel(const unsigned long long* __restrict__ key, const int* __restrict__ pos, int64_t n3,
                                        AtCornerHeader* __restrict__ hdr, int64_t* __restrict__ totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t lo = 0, hi = n3;                                         // the first entry that holds AT_NO_KEY (n3 when there is none)
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (key[mid] == AT_NO_KEY) hi = mid; else lo = mid + 1;
    }
    const int64_t pairs = pos[n3];
    hdr->n_pairs = pairs;
    hdr->n_charted = lo;
    hdr->n_vt = pairs + (lo < n3 ? 1 : 0);
    hdr->n3 = n3;
    totals[0] = hdr->n_vt;
    totals[1] = n3 - lo;
}

__global__ __launch_bounds__(AT_THREADS) void at_corner_emit_kernel(const unsigned long long* __restrict__ key, const unsigned* __restrict__ val,
                                                                    const int* __restrict__ head, const int* __restrict__ pos, int64_t n3,
                                                                    int64_t n_pairs, int64_t n_charted, int* __restrict__ ft,
                                                                    int* __restrict__ vt_vertex, int* __restrict__ vt_chart) {
    const int64_t j = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (j >= n3) return;
    const unsigned long long k = key[j];
    if (k == AT_NO_KEY) {
        ft[val[j]] = (int)n_pairs;
        if (j == n_charted) {
            vt_vertex[n_pairs] = -1;
            vt_chart[n_pairs] = -1;
        }
        return;
    }
    const int h = head[j];
    const int id = pos[j] + h - 1;                                   // pos = exclusive scan of head: the heads at or before j, less one
    ft[val[j]] = id;
    if (h) {
        vt_vertex[id] = (int)(unsigned)(k & 0xFFFFFFFFull);
        vt_chart[id] = (int)(unsigned)(k >> 32);
    }
}

// ---- UV emission ------------------------------------------------------------------------------------------------------------------------
// origin + 0.5 + (coordinate - box) * scale, over size: the difference, ONE product, two sums, ONE division, each rounded on its own
__device__ __forceinline__ float at_uv(double origin, double d, double scale, double size) {
#pragma clang fp contract(off)
    const double prod = d * scale;
    const double at = (origin + 0.5) + prod;
    return (float)(at / size);
}

__global__ __launch_bounds__(AT_THREADS) void at_uv_kernel(const float* __restrict__ verts, int V, const int* __restrict__ vt_vertex,
                                                           const int* __restrict__ vt_chart, int64_t n_vt, const int* __restrict__ chart_class,
                                                           const float* __restrict__ box, const int* __restrict__ origin, int K, double scale,
                                                           double size, float* __restrict__ vt) {
    const int64_t i = (int64_t)blockIdx.x * AT_THREADS + threadIdx.x;
    if (i >= n_vt) return;
    const int v = vt_vertex[i], c = vt_chart[i];
    float u = 0.0f, w = 0.0f;                                        // the sentinel, and anything that is not a (chart, vertex) of this mesh
    if (in_range(v, V) && in_range(c, K)) {
        const int cls = chart_class[c];
        if (in_range(cls, 6)) {
            const int k = cls >> 1;
            const double xp = verts[3 * (int64_t)v + (k + 1) % 3], xq = verts[3 * (int64_t)v + (k + 2) % 3];
            const double dp = (cls & 1) ? (double)box[4 * (int64_t)c + 2] - xp : xp - (double)box[4 * (int64_t)c];
            const double dq = xq - (double)box[4 * (int64_t)c + 1];
            u = at_uv((double)origin[2 * (int64_t)c], dp, scale, size);
            w = at_uv((double)origin[2 * (int64_t)c + 1], dq, scale, size);
        }
    }
    vt[2 * i] = u;
    vt[2 * i + 1] = w;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
bool sizes_ok(int64_t V, int64_t T) { return V >= 0 && T >= 0 && V <= AT_MAX_ITEMS && T <= AT_MAX_ITEMS / 3; }

// adjacency and corners: two key and two value arrays of 3T entries, head flags and their scan (corners), the sort's / scan's scratch
struct SortLayout {
    size_t key_a, key_b, val_a, val_b, head, pos, temp, temp_bytes, total;
};

int sort_layout(int64_t T, bool corners, SortLayout* L) {
    const int64_t n3 = 3 * T;
    size_t tb = 0, sb = 0;
    if (sort_pairs_temp<unsigned long long>(n3, 64, &tb) != hipSuccess || (corners && scan_temp<int>(n3 + 1, &sb) != hipSuccess))
        return nero_fail(NERO_ERR_LAUNCH, corners ? "nero_mesh_chart_corners: the scratch-size query of the corner sort or the head scan failed"
                                                  : "nero_mesh_face_adjacency: the scratch-size query of the edge sort failed");
    *L = SortLayout{};
    Carve c{256};                                                   // AtCornerHeader
    L->key_a = c.take((size_t)n3 * sizeof(unsigned long long));
    L->key_b = c.take((size_t)n3 * sizeof(unsigned long long));
    L->val_a = c.take((size_t)n3 * sizeof(unsigned));
    L->val_b = c.take((size_t)n3 * sizeof(unsigned));
    if (corners) {
        L->head = c.take((size_t)(n3 + 1) * sizeof(int));
        L->pos = c.take((size_t)(n3 + 1) * sizeof(int));
    }
    L->temp_bytes = sb > tb ? sb : tb;
    L->temp = c.take(L->temp_bytes);
    L->total = c.at;
    return NERO_OK;
}

struct LabelLayout {
    size_t flag, rank, temp, temp_bytes, total;
};

int label_layout(int64_t T, LabelLayout* L) {
    if (scan_temp<int>(T + 1, &L->temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_chart_label: the scratch-size query of the rank scan failed");
    Carve c;
    L->flag = c.take((size_t)(T + 1) * sizeof(int));
    L->rank = c.take((size_t)(T + 1) * sizeof(int));
    L->temp = c.take(L->temp_bytes);
    L->total = c.at;
    return NERO_OK;
}

}  // namespace

size_t nero_mesh_face_adjacency_workspace_bytes(int64_t T) {
    SortLayout L;
    if (!sizes_ok(0, T)) return no_workspace("nero_mesh_face_adjacency_workspace_bytes: 3 T must be in [0, 2^31)");
    return sort_layout(T, false, &L) == NERO_OK ? L.total : 0;
}

int nero_mesh_face_adjacency(const int* tris, int64_t T, int64_t V, void* ws, int* nbr, int64_t* counts, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_face_adjacency: V and 3 T must be in [0, 2^31)");
    if (!counts || (T > 0 && (!tris || !nbr || !ws))) return nero_fail(NERO_ERR_ARG, "nero_mesh_face_adjacency: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_face_adjacency: hipMemsetAsync failed");
    if (T == 0) return NERO_OK;
    const int64_t n3 = 3 * T;
    uint8_t* w = (uint8_t*)ws;
    SortLayout L;
    if (int rc = sort_layout(T, false, &L)) return rc;
    unsigned long long* key_a = (unsigned long long*)(w + L.key_a);
    unsigned long long* key_b = (unsigned long long*)(w + L.key_b);
    unsigned* val_a = (unsigned*)(w + L.val_a);
    unsigned* val_b = (unsigned*)(w + L.val_b);
    if (hipMemsetAsync(nbr, 0xFF, (size_t)n3 * sizeof(int), s) != hipSuccess)                  // -1: no neighbour
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_face_adjacency: hipMemsetAsync failed");
    hipLaunchKernelGGL(at_edge_key_kernel, dim3(blocks_of(n3)), dim3(AT_THREADS), 0, s, tris, n3, (int)V, key_a, val_a);
    if (int rc = nero_check_launch("nero_mesh_face_adjacency: edge keys")) return rc;
    if (int rc = sort_pairs<unsigned long long>(w + L.temp, L.temp_bytes, key_a, key_b, val_a, val_b, n3, 32 + bit_length(V), s,
                                                "nero_mesh_face_adjacency: edge sort failed"))       // (AT_NO_KEY stays the largest under these bits)
        return rc;
    hipLaunchKernelGGL(at_edge_group_kernel, dim3(blocks_of(n3)), dim3(AT_THREADS), 0, s, (const unsigned long long*)key_b, (const unsigned*)val_b, n3,
                       nbr, (unsigned long long*)counts);
    return nero_check_launch("nero_mesh_face_adjacency: edge groups");
}

size_t nero_mesh_chart_label_workspace_bytes(int64_t T) {
    LabelLayout L;
    if (!sizes_ok(0, T)) return no_workspace("nero_mesh_chart_label_workspace_bytes: 3 T must be in [0, 2^31)");
    return label_layout(T, &L) == NERO_OK ? L.total : 0;
}

int nero_mesh_chart_label(const float* verts, const int* tris, int64_t T, int64_t V, const int* nbr, void* ws, int* face_class, int* chart,
                          int64_t* info, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_chart_label: V and 3 T must be in [0, 2^31)");
    if (!info || (T > 0 && (!tris || !nbr || !ws || !face_class || !chart)) || (T > 0 && V > 0 && !verts))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_label: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(info, 0, 2 * sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_chart_label: hipMemsetAsync failed");
    if (T == 0) return NERO_OK;
    uint8_t* w = (uint8_t*)ws;
    LabelLayout L;
    if (int rc = label_layout(T, &L)) return rc;
    int* flag = (int*)(w + L.flag);
    int* rank = (int*)(w + L.rank);
    unsigned long long* inf = (unsigned long long*)info;
    hipLaunchKernelGGL(at_class_kernel, dim3(blocks_of(T)), dim3(AT_THREADS), 0, s, verts, tris, T, (int)V, face_class, chart, inf);
    if (int rc = nero_check_launch("nero_mesh_chart_label: classes")) return rc;
    hipLaunchKernelGGL(at_hook_kernel, dim3(blocks_of(T)), dim3(AT_THREADS), 0, s, nbr, (const int*)face_class, T, chart);
    if (int rc = nero_check_launch("nero_mesh_chart_label: hook pass")) return rc;
    hipLaunchKernelGGL(at_flatten_kernel, dim3(blocks_of(T + 1)), dim3(AT_THREADS), 0, s, chart, (const int*)face_class, T, flag);
    if (int rc = nero_check_launch("nero_mesh_chart_label: flatten pass")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)flag, rank, T + 1, s, "nero_mesh_chart_label: rank scan failed")) return rc;
    hipLaunchKernelGGL(at_number_kernel, dim3(blocks_of(T)), dim3(AT_THREADS), 0, s, chart, (const int*)face_class, (const int*)rank, T, inf);
    return nero_check_launch("nero_mesh_chart_label: numbering");
}

int nero_mesh_chart_stats(const float* verts, const int* tris, int64_t T, int64_t V, const int* chart, const int* face_class, int64_t K,
                          int* chart_class, int* n_faces, float* box, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_chart_stats: V and 3 T must be in [0, 2^31)");
    if (K < 0 || K > T) return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_stats: K outside [0, T]");
    if (K == 0) return NERO_OK;
    if (!verts || !tris || !chart || !face_class || !chart_class || !n_faces || !box)
        return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_stats: null pointer");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(at_stats_init_kernel, dim3(blocks_of(K)), dim3(AT_THREADS), 0, s, chart_class, n_faces, (unsigned*)box, (int)K);
    if (int rc = nero_check_launch("nero_mesh_chart_stats: init")) return rc;
    hipLaunchKernelGGL(at_stats_kernel, dim3(blocks_of(T)), dim3(AT_THREADS), 0, s, verts, tris, T, (int)V, chart, face_class, (int)K, chart_class,
                       n_faces, (unsigned*)box);
    if (int rc = nero_check_launch("nero_mesh_chart_stats: face pass")) return rc;
    hipLaunchKernelGGL(at_box_decode_kernel, dim3(blocks_of(4 * K)), dim3(AT_THREADS), 0, s, (unsigned*)box, 4 * K);
    return nero_check_launch("nero_mesh_chart_stats: box decode");
}

size_t nero_mesh_chart_corners_workspace_bytes(int64_t T) {
    SortLayout L;
    if (!sizes_ok(0, T)) return no_workspace("nero_mesh_chart_corners_workspace_bytes: 3 T must be in [0, 2^31)");
    return sort_layout(T, true, &L) == NERO_OK ? L.total : 0;
}

int nero_mesh_chart_corners_count(const int* tris, int64_t T, int64_t V, const int* chart, int64_t K, void* ws, int64_t* totals, void* stream) {
    if (!sizes_ok(V, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_chart_corners_count: V and 3 T must be in [0, 2^31)");
    if (K < 0 || K > T) return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_corners_count: K outside [0, T]");
    if (!ws || !totals || (T > 0 && (!tris || !chart))) return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_corners_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    const int64_t n3 = 3 * T;
    if (T == 0) {
        if (hipMemsetAsync(w, 0, 256, s) != hipSuccess || hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s) != hipSuccess)
            return nero_fail(NERO_ERR_LAUNCH, "nero_mesh_chart_corners_count: hipMemsetAsync failed");
        return NERO_OK;
    }
    SortLayout L;
    if (int rc = sort_layout(T, true, &L)) return rc;
    unsigned long long* key_a = (unsigned long long*)(w + L.key_a);
    unsigned long long* key_b = (unsigned long long*)(w + L.key_b);
    unsigned* val_a = (unsigned*)(w + L.val_a);
    unsigned* val_b = (unsigned*)(w + L.val_b);
    int* head = (int*)(w + L.head);
    int* pos = (int*)(w + L.pos);
    hipLaunchKernelGGL(at_corner_key_kernel, dim3(blocks_of(n3)), dim3(AT_THREADS), 0, s, tris, n3, (int)V, chart, (int)K, key_a, val_a);
    if (int rc = nero_check_launch("nero_mesh_chart_corners_count: corner keys")) return rc;
    if (int rc = sort_pairs<unsigned long long>(w + L.temp, L.temp_bytes, key_a, key_b, val_a, val_b, n3, 32 + bit_length(K), s,
                                                "nero_mesh_chart_corners_count: corner sort failed"))
        return rc;
    hipLaunchKernelGGL(at_corner_head_kernel, dim3(blocks_of(n3 + 1)), dim3(AT_THREADS), 0, s, (const unsigned long long*)key_b, n3, head);
    if (int rc = nero_check_launch("nero_mesh_chart_corners_count: head flags")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int*)head, pos, n3 + 1, s, "nero_mesh_chart_corners_count: head scan failed")) return rc;
    hipLaunchKernelGGL(at_corner_totals_kernel, dim3(1), dim3(64), 0, s, (const unsigned long long*)key_b, (const int*)pos, n3, (AtCornerHeader*)w,
                       totals);
    return nero_check_launch("nero_mesh_chart_corners_count: totals");
}

int nero_mesh_chart_corners_emit(int64_t T, void* ws, int* ft, int* vt_vertex, int* vt_chart, int64_t vt_cap, void* stream) {
    if (!sizes_ok(0, T)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_chart_corners_emit: 3 T must be in [0, 2^31)");
    if (!ws || vt_cap < 0 || (T > 0 && !ft)) return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_corners_emit: null pointer or negative capacity");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    const int64_t n3 = 3 * T;
    // the one synchronisation: the totals nero_mesh_chart_corners_count left in the workspace, so that outputs that are too small are an
    // error code and not a write out of range
    AtCornerHeader h{-1, -1, -1, -1};
    if (int rc = read_back(&h, w, sizeof(h), s, "nero_mesh_chart_corners_emit: reading the totals of nero_mesh_chart_corners_count failed")) return rc;
    if (h.n3 != n3 || h.n_pairs < 0 || h.n_pairs > n3 || h.n_charted < 0 || h.n_charted > n3 || h.n_vt != h.n_pairs + (h.n_charted < n3 ? 1 : 0))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_corners_emit: the workspace holds no totals of nero_mesh_chart_corners_count for this mesh");
    if (h.n_vt > vt_cap) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_mesh_chart_corners_emit: %lld UV vertices exceed the capacity %lld", (long long)h.n_vt, (long long)vt_cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (h.n_vt > 0 && (!vt_vertex || !vt_chart)) return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_corners_emit: null output pointer");
    if (T == 0) return NERO_OK;
    SortLayout L;
    if (int rc = sort_layout(T, true, &L)) return rc;
    hipLaunchKernelGGL(at_corner_emit_kernel, dim3(blocks_of(n3)), dim3(AT_THREADS), 0, s, (const unsigned long long*)(w + L.key_b),
                       (const unsigned*)(w + L.val_b), (const int*)(w + L.head), (const int*)(w + L.pos), n3, h.n_pairs, h.n_charted, ft, vt_vertex,
                       vt_chart);
    return nero_check_launch("nero_mesh_chart_corners_emit");
}

int nero_mesh_chart_uv(const float* verts, int64_t V, const int* vt_vertex, const int* vt_chart, int64_t n_vt, const int* chart_class, const float* box,
                       const int* origin, int64_t K, double scale, int size, float* vt, void* stream) {
    if (V < 0 || V > AT_MAX_ITEMS || n_vt < 0 || n_vt > AT_MAX_ITEMS || K < 0 || K > AT_MAX_ITEMS)
        return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mesh_chart_uv: V, n_vt and K must be in [0, 2^31)");
    if (size < 1 || size > AT_MAX_SIZE || !(scale >= 0.0) || !(scale <= 1.7976931348623157e308)) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_mesh_chart_uv: size %d outside [1, %d] or scale %g negative or not finite", size, AT_MAX_SIZE, scale);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (n_vt == 0) return NERO_OK;
    if (!vt || !vt_vertex || !vt_chart || (V > 0 && !verts) || (K > 0 && (!chart_class || !box || !origin)))
        return nero_fail(NERO_ERR_ARG, "nero_mesh_chart_uv: null pointer");
    hipLaunchKernelGGL(at_uv_kernel, dim3(blocks_of(n_vt)), dim3(AT_THREADS), 0, (hipStream_t)stream, verts, (int)V, vt_vertex, vt_chart, n_vt,
                       chart_class, box, origin, (int)K, scale, (double)size, vt);
    return nero_check_launch("nero_mesh_chart_uv");
}
