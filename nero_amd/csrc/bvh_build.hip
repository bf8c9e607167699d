// bvh_build.hip -- builds the tree of bvh.hip's Builder::build on the device, from a device-resident mesh (gfx950).
//
// The host builder splits every range of n > 4 triangles at lo + n / 2 on the longest centroid axis, so the SHAPE of its tree -- node
// indices, ranges, leaf references, depth -- is a function of nT alone (bvh_build_plan.h); only the triangle order and the boxes depend on
// the geometry.  This build reproduces that tree: where std::nth_element partitions, it sorts the range (stable, ascending, -0 == +0),
// which fixes the one thing nth_element leaves open, the order of equal centroids.  Every quantity is a min, a max, a stable sort or one
// rounded fp32 operation: the nodes and triangle records are bit-reproducible, and the traversal kernels, their LDS stack and their
// launch orders carry over unchanged ("BVH build on the device").
//
// Schedule, all on the caller's stream:
//   prep          centroids, boxes, the identity order; bad triangles (index out of range, non-finite coordinate) counted with an integer
//                 atomic -- the count is read back, the build's one synchronisation;
//   wide levels   levels whose ranges exceed the LDS capacity S: per-range centroid extents by integer atomics on an order-preserving
//                 image of the floats (wave-reduced first), the axis per range, then ONE stable radix sort of (range << 32 | key) over the
//                 32 + level bits in use;
//   finish        one workgroup per range of the first level whose ranges fit S: all remaining levels in LDS (finish_kernel, the hot path);
//   emit          boxes and nodes level by level, bottom-up, then the triangle records in leaf order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include "../../include/nero_hip.h"
#include "bvh_build_plan.h"
#include "bvh_types.h"
#include "common.h"
#include "cub_calls.h"
#include "device_prims.h"

namespace {

using namespace nero_bvh;
using namespace nero_bvh_plan;
using namespace nero_cub;
using namespace nero_prims;
using nero_ws::blocks_of;
typedef unsigned long long u64;

// S, the LDS capacity of finish_kernel, in triangles.  34 bytes of LDS per triangle (key 8, two slot buffers 2 + 2, centroid 12, triangle 4,
// extents 6) and S / 4 threads: S = 2048 takes 68 KiB, two workgroups of 512 threads per CU of 160 KiB.  A larger S saves global sort levels
// (each ~0.3 ms at 360 k triangles: launch-bound), a smaller one shortens the bitonic network (log2(S)^2 / 2 barrier steps per level).
// Measured on one MI355X, sum of the build's phases / finish_kernel alone, ms (scripts/bench_bvh_build.py, median of 5):
//     S        512^3 mesh, 360 092 tris   icosphere(7), 327 680   256^3 mesh, 89 568   512^3 at 100 k faces, 98 276
//     512      3.217 / 0.145              2.879 / 0.141           1.162 / 0.108        1.205 / 0.110
//     1024     3.118 / 0.206              2.813 / 0.200           1.144 / 0.171        1.181 / 0.175
//     2048     3.028 / 0.270              2.745 / 0.263           1.143 / 0.262        1.186 / 0.269      <- chosen
//     4096     3.115 / 0.479              2.853 / 0.463           1.256 / 0.469        1.310 / 0.489      (one workgroup of 1024 threads per CU)
// The wide levels are the larger part at every S (2.3 - 3.0 ms of the ~3 ms at 360 k): the choice of S trades one of them against finish time.
#ifndef NERO_BVH_BUILD_S
#define NERO_BVH_BUILD_S 2048
#endif
constexpr int S_CAP = NERO_BVH_BUILD_S;
constexpr int FIN_PER = 4;                             // positions per thread
constexpr int FIN_THREADS = S_CAP / FIN_PER;
constexpr int POS_BITS = 12;                           // key of the LDS sort: range start << 44 | float key << 12 | position
static_assert(S_CAP >= 256 && S_CAP <= (1 << POS_BITS) && (S_CAP & (S_CAP - 1)) == 0, "S: a power of two in [256, 4096]");
static_assert(FIN_THREADS % 64 == 0 && FIN_THREADS <= 1024, "whole wavefronts");

// min and max in the order of f2o (-0 below +0): exact, and defined where the C library's are not (-0 is the smaller zero), so boxes are bit-reproducible
__device__ __forceinline__ float tmin(float a, float b) { return f2o(b) < f2o(a) ? b : a; }
__device__ __forceinline__ float tmax(float a, float b) { return f2o(b) > f2o(a) ? b : a; }
// the sort key of a centroid coordinate: the two zeros are one value
__device__ __forceinline__ unsigned sort_key(float c) {
    if (c == 0.f) c = 0.f;
    return f2o(c);
}
__device__ __forceinline__ int pick_axis(const unsigned* e) {          // e: min x y z, max x y z (order-preserving images)
#pragma clang fp contract(off)
    const float ex = o2f(e[3]) - o2f(e[0]), ey = o2f(e[4]) - o2f(e[1]), ez = o2f(e[5]) - o2f(e[2]);
    int axis = 0;
    float best = ex;
    if (ey > best) { axis = 1; best = ey; }
    if (ez > best) axis = 2;
    return axis;
}

// ---- prep -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void prep_kernel(const float* __restrict__ V, int nV, const int* __restrict__ F, int nT,
                                                   float* __restrict__ cen, float* __restrict__ bmin, float* __restrict__ bmax,
                                                   unsigned* __restrict__ order, int* __restrict__ bad) {
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nT) return;
    order[t] = (unsigned)t;
    const int i0 = F[t * 3], i1 = F[t * 3 + 1], i2 = F[t * 3 + 2];
    bool ok = in_range(i0, nV) && in_range(i1, nV) && in_range(i2, nV);
    float c[3] = {0.f, 0.f, 0.f}, mn[3] = {0.f, 0.f, 0.f}, mx[3] = {0.f, 0.f, 0.f};
    if (ok) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float x0 = V[(size_t)i0 * 3 + a], x1 = V[(size_t)i1 * 3 + a], x2 = V[(size_t)i2 * 3 + a];
            ok = ok && isfinite(x0) && isfinite(x1) && isfinite(x2);
            c[a] = __fdiv_rn(((0.f + x0) + x1) + x2, 3.f);
            mn[a] = tmin(tmin(x0, x1), x2);
            mx[a] = tmax(tmax(x0, x1), x2);
        }
    }
    if (!ok) {
        atomicAdd(bad, 1);
#pragma unroll
        for (int a = 0; a < 3; ++a) { c[a] = 0.f; mn[a] = 0.f; mx[a] = 0.f; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        cen[(size_t)a * nT + t] = c[a];
        bmin[(size_t)t * 3 + a] = mn[a];
        bmax[(size_t)t * 3 + a] = mx[a];
    }
}

// ---- wide levels ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ext_init_kernel(unsigned* __restrict__ ext, int n_ranges) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_ranges * 6) ext[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

// extents of the centroids of every range of level `l`.  A wavefront's 64 positions lie in one range almost always (ranges here hold more
// than S triangles): then it reduces in registers and issues six atomics; a wavefront that straddles a boundary lets every lane issue its own.
__global__ __launch_bounds__(256) void wide_extent_kernel(const float* __restrict__ cen, const unsigned* __restrict__ order, int nT, int l,
                                                          unsigned* __restrict__ ext) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < nT;
    int lo, n, lev, k = -1;
    unsigned v[3] = {0, 0, 0};
    if (live) {
        k = locate(nT, l, i, &lo, &n, &lev);
        const unsigned t = order[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = f2o(cen[(size_t)a * nT + t]);
    }
    const int k0 = __shfl(k, 0);
    if (__all(k == k0)) {                  // (lane 0 is live whenever any lane is: a dead lane makes the vote fail)
        unsigned mn[3], mx[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = wave_min(v[a]); mx[a] = wave_max(v[a]); }
        if ((threadIdx.x & 63) == 0 && live) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(&ext[(size_t)k * 6 + a], mn[a]); atomicMax(&ext[(size_t)k * 6 + 3 + a], mx[a]); }
        }
    } else if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { atomicMin(&ext[(size_t)k * 6 + a], v[a]); atomicMax(&ext[(size_t)k * 6 + 3 + a], v[a]); }
    }
}

__global__ __launch_bounds__(256) void wide_key_kernel(const float* __restrict__ cen, const unsigned* __restrict__ order, int nT, int l,
                                                       const unsigned* __restrict__ ext, u64* __restrict__ keys) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nT) return;
    int lo, n, lev;
    const int k = locate(nT, l, i, &lo, &n, &lev);
    unsigned e[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) e[a] = ext[(size_t)k * 6 + a];
    const int axis = pick_axis(e);
    keys[i] = ((u64)(unsigned)k << 32) | sort_key(cen[(size_t)axis * nT + order[i]]);
}

// ---- finish: all levels from `l0` on, one workgroup per range of level l0, in LDS -----------------------------------------------------
// A level: extents per range (LDS atomics on the order-preserving images), the axis, then a bitonic sort of the whole workgroup's array
// on 64-bit keys (start of the range | centroid key | position).  The position makes every key distinct -- the sort is the stable sort of
// the specification whatever the network does -- and the range start in the top bits keeps every triangle inside its range; positions of
// leaves keep a zero centroid key and stay where they are.  slot[] follows the triangles, which themselves never move in LDS.
template <int S>
__global__ __launch_bounds__(S / FIN_PER) void finish_kernel(const float* __restrict__ cen, unsigned* __restrict__ order, Plan plan) {
    constexpr int NT = S / FIN_PER;
    __shared__ u64 key[S];
    __shared__ float c_x[S], c_y[S], c_z[S];
    __shared__ unsigned tri[S];
    __shared__ unsigned ext[(S / 4) * 6];
    __shared__ unsigned short slot_a[S], slot_b[S];
    const int nT = plan.nT, l0 = plan.hand_off, tid = threadIdx.x;
    const Range wg = range_of(plan, l0, blockIdx.x);
    if (!wg.valid || wg.n <= LEAF_MAX) return;            // (workgroup-uniform)
    const int n = wg.n;                                  // <= S by the choice of l0
    int P = 2 * LEAF_MAX;
    while (P < n) P <<= 1;                               // the bitonic network's size, <= S
    int r_lo[FIN_PER], r_n[FIN_PER], r_k[FIN_PER];       // the range of this thread's positions p = tid + j NT on the current level
#pragma unroll
    for (int j = 0; j < FIN_PER; ++j) {
        const int p = tid + j * NT;
        r_lo[j] = 0; r_n[j] = n; r_k[j] = 0;
        if (p < n) {
            const unsigned t = order[wg.lo + p];
            tri[p] = t;
            c_x[p] = cen[t]; c_y[p] = cen[(size_t)nT + t]; c_z[p] = cen[(size_t)2 * nT + t];
            slot_a[p] = (unsigned short)p;
        }
    }
    unsigned short* slot = slot_a;
    unsigned short* slot_next = slot_b;
    __syncthreads();
    for (int l = l0; l < plan.n_levels; ++l) {
        const int n_ranges = 1 << (l - l0);              // ranges with more than 4 triangles: n_ranges < n / 4 <= S / 4
        for (int i = tid; i < n_ranges * 6 && i < (S / 4) * 6; i += NT) ext[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FIN_PER; ++j) {
            const int p = tid + j * NT;
            if (p < n && r_n[j] > LEAF_MAX) {
                const int s = slot[p];
                unsigned* e = ext + r_k[j] * 6;
                atomicMin(e + 0, f2o(c_x[s])); atomicMax(e + 3, f2o(c_x[s]));
                atomicMin(e + 1, f2o(c_y[s])); atomicMax(e + 4, f2o(c_y[s]));
                atomicMin(e + 2, f2o(c_z[s])); atomicMax(e + 5, f2o(c_z[s]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < FIN_PER; ++j) {
            const int p = tid + j * NT;
            if (p < P) {
                u64 kk = ~(u64)0;                        // padding sorts behind everything
                if (p < n) {
                    unsigned fk = 0;
                    if (r_n[j] > LEAF_MAX) {
                        const int axis = pick_axis(ext + r_k[j] * 6);
                        const int s = slot[p];
                        fk = sort_key(axis == 0 ? c_x[s] : (axis == 1 ? c_y[s] : c_z[s]));
                    }
                    kk = ((u64)(unsigned)r_lo[j] << (32 + POS_BITS)) | ((u64)fk << POS_BITS) | (u64)(unsigned)p;
                }
                key[p] = kk;
            }
        }
        __syncthreads();
        for (int kb = 2; kb <= P; kb <<= 1) {
            for (int jb = kb >> 1; jb > 0; jb >>= 1) {
                for (int q = tid; q < P / 2; q += NT) {
                    const int i = ((q & ~(jb - 1)) << 1) | (q & (jb - 1)), m = i | jb;
                    const u64 a = key[i], b = key[m];
                    const bool up = (i & kb) == 0;
                    if ((a > b) == up) { key[i] = b; key[m] = a; }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int j = 0; j < FIN_PER; ++j) {
            const int p = tid + j * NT;
            if (p < n) slot_next[p] = slot[(int)(key[p] & ((1u << POS_BITS) - 1))];
            if (p < n && r_n[j] > LEAF_MAX) {            // this position's range on the next level
                const int h = r_n[j] / 2;
                if (p >= r_lo[j] + h) { r_lo[j] += h; r_n[j] -= h; r_k[j] = 2 * r_k[j] + 1; }
                else { r_n[j] = h; r_k[j] = 2 * r_k[j]; }
            } else {
                r_k[j] = 0;                              // a leaf: its extents are not used again
            }
        }
        __syncthreads();
        unsigned short* const tmp = slot; slot = slot_next; slot_next = tmp;
    }
#pragma unroll
    for (int j = 0; j < FIN_PER; ++j) {
        const int p = tid + j * NT;
        if (p < n) order[wg.lo + p] = tri[slot[p]];
    }
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------------
struct Box { float mn[3], mx[3]; };

// level l, one thread per range: a leaf range takes its box from its triangles; an inner range writes its node from its children's boxes
// (level l + 1, written by the launch before) and keeps their union.  Launched for l = n_levels down to 0.
__global__ __launch_bounds__(256) void emit_level_kernel(Plan plan, int l, const unsigned* __restrict__ order, const float* __restrict__ bmin,
                                                         const float* __restrict__ bmax, Box* __restrict__ heap, Node* __restrict__ nodes) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1 << l)) return;
    const Range r = range_of(plan, l, k);
    if (!r.valid) return;
    Box b;
    if (r.n <= LEAF_MAX) {
        const unsigned t0 = order[r.lo];
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.mn[a] = bmin[(size_t)t0 * 3 + a]; b.mx[a] = bmax[(size_t)t0 * 3 + a]; }
        for (int i = 1; i < r.n; ++i) {
            const unsigned t = order[r.lo + i];
#pragma unroll
            for (int a = 0; a < 3; ++a) { b.mn[a] = tmin(b.mn[a], bmin[(size_t)t * 3 + a]); b.mx[a] = tmax(b.mx[a], bmax[(size_t)t * 3 + a]); }
        }
    } else {
        const size_t c = ((size_t)2 << l) - 1 + 2 * (size_t)k;
        const Box bl = heap[c], br = heap[c + 1];
        const int h = r.n / 2;
        Node nd;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            nd.lmin[a] = bl.mn[a]; nd.lmax[a] = bl.mx[a]; nd.rmin[a] = br.mn[a]; nd.rmax[a] = br.mx[a];
            b.mn[a] = tmin(bl.mn[a], br.mn[a]); b.mx[a] = tmax(bl.mx[a], br.mx[a]);
        }
        nd.left = h <= LEAF_MAX ? -(r.lo * 8 + h) - 1 : r.node + 1;
        nd.right = r.n - h <= LEAF_MAX ? -((r.lo + h) * 8 + (r.n - h)) - 1 : r.node + 1 + inner_count(plan, l + 1, h);
        nd.pad[0] = 0; nd.pad[1] = 0;
        nodes[r.node] = nd;
    }
    heap[((size_t)1 << l) - 1 + k] = b;
}

__global__ __launch_bounds__(256) void emit_tris_kernel(const float* __restrict__ V, const int* __restrict__ F, const unsigned* __restrict__ order,
                                                        int nT, Tri* __restrict__ out) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nT) return;
    const unsigned t = order[i];
    const float* a = V + (size_t)F[(size_t)t * 3] * 3;
    const float* b = V + (size_t)F[(size_t)t * 3 + 1] * 3;
    const float* c = V + (size_t)F[(size_t)t * 3 + 2] * 3;
    Tri r;
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.v0[k] = a[k]; r.e1[k] = b[k] - a[k]; r.e2[k] = c[k] - a[k]; r.pad[k] = 0.f; }
    out[i] = r;
}

// phase marks of the last build (nero_bvh_build_last_phase_ms): start | prep done || wide levels start | done | finish done | emit done
enum { EV_START = 0, EV_PREP, EV_WIDE0, EV_WIDE1, EV_FINISH, EV_EMIT, EV_COUNT };
hipEvent_t g_ev[EV_COUNT];
bool g_ev_made = false, g_ev_valid = false;
void mark(int which, hipStream_t s) {
    if (!g_ev_made) {
        for (int i = 0; i < EV_COUNT; ++i)
            if (hipEventCreate(&g_ev[i]) != hipSuccess) return;
        g_ev_made = true;
    }
    (void)hipEventRecord(g_ev[which], s);
}

}  // namespace

extern "C" {

size_t nero_bvh_build_workspace_bytes(int nV, int nT) {
    Plan p;
    if (nV < 3 || !make_plan(nT, S_CAP, &p)) return 0;
    return layout(p).total;
}

int nero_bvh_build_lds_capacity(void) { return S_CAP; }

int nero_bvh_create_device(const float* d_verts, int nV, const int* d_tris, int nT, void* ws, size_t ws_bytes, void* stream, void** handle) {
    if (!d_verts || !d_tris || !ws || !handle || nT < 1 || nV < 3) return nero_fail(NERO_ERR_ARG, "nero_bvh_create_device: bad argument");
    if (nT > MAX_TRIS) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_bvh_create_device: 2^27 triangles or more (leaf references would reach the sentinel)");
    Plan plan;
    if (!make_plan(nT, S_CAP, &plan)) return nero_fail(NERO_ERR_ARG, "nero_bvh_create_device: bad argument");
    const Layout L = layout(plan);
    if (ws_bytes < L.total) return nero_fail(NERO_ERR_ARG, "nero_bvh_create_device: workspace smaller than nero_bvh_build_workspace_bytes");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)(((uintptr_t)ws + 255) / 256 * 256);
    int* bad = (int*)(w + L.hdr);
    float* cen = (float*)(w + L.cen);
    float* bmin = (float*)(w + L.bmin);
    float* bmax = (float*)(w + L.bmax);
    unsigned* ord = (unsigned*)(w + L.order_a);
    unsigned* ord_alt = (unsigned*)(w + L.order_b);
    u64* key = (u64*)(w + L.key_a);
    u64* key_alt = (u64*)(w + L.key_b);
    unsigned* ext = (unsigned*)(w + L.ext);
    Box* heap = (Box*)(w + L.heap);

    g_ev_valid = false;
    mark(EV_START, s);
    if (hipMemsetAsync(bad, 0, sizeof(int), s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_create_device: hipMemsetAsync failed");
    hipLaunchKernelGGL(prep_kernel, dim3(blocks_of(nT)), dim3(256), 0, s, d_verts, nV, d_tris, nT, cen, bmin, bmax, ord, bad);
    if (nero_check_launch("nero_bvh_create_device (prep)") != NERO_OK) return NERO_ERR_LAUNCH;
    mark(EV_PREP, s);
    // the one synchronisation: a mesh with an index out of range or a non-finite coordinate is an error code, not a tree
    int n_bad = -1;
    if (int rc = read_back(&n_bad, bad, sizeof(int), s, "nero_bvh_create_device: reading the bad-triangle count failed")) return rc;
    if (n_bad != 0) {
        char msg[160];
        snprintf(msg, sizeof(msg), "nero_bvh_create_device: %d triangle(s) with a vertex index out of range or a non-finite coordinate", n_bad);
        return nero_fail(NERO_ERR_ARG, msg);
    }

    Handle* h = new Handle();
    h->root = plan.root;
    h->max_depth = plan.n_levels;
    h->mode = plan.n_levels <= PL_STACK ? 1 : 0;
    h->b.n_nodes = plan.n_nodes;
    h->b.n_tris = nT;
    const size_t nb = (plan.n_nodes > 0 ? (size_t)plan.n_nodes : 1) * sizeof(Node);
    if (hipMalloc(&h->b.d_nodes, nb) != hipSuccess || hipMalloc(&h->b.d_tris, (size_t)nT * sizeof(Tri)) != hipSuccess ||
        hipMalloc(&h->b.d_face, (size_t)nT * sizeof(int)) != hipSuccess) {
        (void)hipFree(h->b.d_nodes);
        (void)hipFree(h->b.d_tris);
        (void)hipFree(h->b.d_face);
        delete h;
        return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_create_device: hipMalloc failed");
    }
    auto drop = [h](int rc) {                                  // (the message is nero_fail's already)
        (void)hipFree(h->b.d_nodes);
        (void)hipFree(h->b.d_tris);
        (void)hipFree(h->b.d_face);
        delete h;
        return rc;
    };

    mark(EV_WIDE0, s);
    for (int l = 0; l < plan.hand_off; ++l) {
        const int n_ranges = 1 << l;
        hipLaunchKernelGGL(ext_init_kernel, dim3(blocks_of((size_t)n_ranges * 6)), dim3(256), 0, s, ext, n_ranges);
        hipLaunchKernelGGL(wide_extent_kernel, dim3(blocks_of(nT)), dim3(256), 0, s, cen, ord, nT, l, ext);
        hipLaunchKernelGGL(wide_key_kernel, dim3(blocks_of(nT)), dim3(256), 0, s, cen, ord, nT, l, ext, key);
        if (int rc = sort_pairs<u64>(w + L.temp, L.temp_bytes, key, key_alt, ord, ord_alt, nT, 32 + l, s,
                                     "nero_bvh_create_device: radix sort failed"))
            return drop(rc);
        unsigned* const t = ord; ord = ord_alt; ord_alt = t;
    }
    mark(EV_WIDE1, s);
    if (plan.n_levels > plan.hand_off)
        hipLaunchKernelGGL(finish_kernel<S_CAP>, dim3(1u << plan.hand_off), dim3(FIN_THREADS), 0, s, cen, ord, plan);
    mark(EV_FINISH, s);
    for (int l = plan.n_levels; l >= 0; --l)
        hipLaunchKernelGGL(emit_level_kernel, dim3(blocks_of((size_t)1 << l)), dim3(256), 0, s, plan, l, ord, bmin, bmax, heap, h->b.d_nodes);
    hipLaunchKernelGGL(emit_tris_kernel, dim3(blocks_of(nT)), dim3(256), 0, s, d_verts, d_tris, ord, nT, h->b.d_tris);
    mark(EV_EMIT, s);
    // the face table: the final leaf order (face indices below 2^27: the same bits as ints), copied on the build's stream before the caller
    // may reuse the workspace
    if (hipMemcpyAsync(h->b.d_face, ord, (size_t)nT * sizeof(int), hipMemcpyDeviceToDevice, s) != hipSuccess)
        return drop(nero_fail(NERO_ERR_LAUNCH, "nero_bvh_create_device: copying the face table failed"));
    if (hipGetLastError() != hipSuccess) return drop(nero_fail(NERO_ERR_LAUNCH, "nero_bvh_create_device: a kernel launch failed"));
    g_ev_valid = g_ev_made;
    *handle = h;
    return NERO_OK;
}

int nero_bvh_build_last_phase_ms(float* ms) {
    if (!ms) return nero_fail(NERO_ERR_ARG, "nero_bvh_build_last_phase_ms: bad argument");
    if (!g_ev_valid) return nero_fail(NERO_ERR_ARG, "nero_bvh_build_last_phase_ms: no successful device build to report on");
    if (hipEventSynchronize(g_ev[EV_EMIT]) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_build_last_phase_ms: hipEventSynchronize failed");
    const int from[4] = {EV_START, EV_WIDE0, EV_WIDE1, EV_FINISH}, to[4] = {EV_PREP, EV_WIDE1, EV_FINISH, EV_EMIT};
    for (int i = 0; i < 4; ++i)
        if (hipEventElapsedTime(&ms[i], g_ev[from[i]], g_ev[to[i]]) != hipSuccess)
            return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_build_last_phase_ms: hipEventElapsedTime failed");
    return NERO_OK;
}

int nero_bvh_info(void* handle, int* n_nodes, int* n_tris, int* max_depth, int* root) {
    if (!handle) return nero_fail(NERO_ERR_ARG, "nero_bvh_info: bad argument");
    const Handle* h = (const Handle*)handle;
    if (n_nodes) *n_nodes = h->b.n_nodes;
    if (n_tris) *n_tris = h->b.n_tris;
    if (max_depth) *max_depth = h->max_depth;
    if (root) *root = h->root;
    return NERO_OK;
}

int nero_bvh_export(void* handle, void* nodes_host, void* tris_host) {
    if (!handle || !nodes_host || !tris_host) return nero_fail(NERO_ERR_ARG, "nero_bvh_export: bad argument");
    const Handle* h = (const Handle*)handle;
    // hipMemcpy orders itself behind the work of the null stream only: wait for every stream, the build's included
    if (hipDeviceSynchronize() != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_export: hipDeviceSynchronize failed");
    hipError_t e0 = hipSuccess;
    if (h->b.n_nodes > 0) e0 = hipMemcpy(nodes_host, h->b.d_nodes, (size_t)h->b.n_nodes * sizeof(Node), hipMemcpyDeviceToHost);
    const hipError_t e1 = hipMemcpy(tris_host, h->b.d_tris, (size_t)h->b.n_tris * sizeof(Tri), hipMemcpyDeviceToHost);
    if (e0 != hipSuccess || e1 != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_bvh_export: hipMemcpy failed");
    return NERO_OK;
}

}  // extern "C"
