// mcubes.hip -- marching cubes on the device: the Stage-I SDF grid -> the triangle mesh Stage II traces (include/nero_hip.h, nero_mcubes_*).
//
// Replaces `mcubes.marching_cubes(u, threshold)` (PyMCubes, network/field.py:1110-1117, called from extract_mesh.py:24-31).  Two passes and a
// scan, with every output position fixed by a prefix sum over the grid's linear order (no atomics decide placement, so the mesh does not
// depend on the launch shape and two runs are bit-identical):
//   pass 1 (mc_count_kernel)  one lane per grid point p: the 3-bit mask of the crossing edges p owns (p -> p + e_x, e_y, e_z), p's "below"
//                             bit, and the case of the cell whose min corner is p.  Stores code[p] = mask | below << 3 and per-tile totals
//                             of vertices (popcount of the mask) and triangles (nero_mcubes_tri_count[case]).
//   scan                      exclusive prefix sums of the per-tile totals (hipCUB), a trailing zero entry giving {V, T}.
//   pass 2a (mc_vert_kernel)  per tile, the tile base plus an in-tile prefix (wave-64 ballots): vertex ids in (point, axis x<y<z) order,
//                             the interpolated vertices, and vbase[p] = id of p's first vertex (written only where p owns one).
//   pass 2b (mc_tri_kernel)   the same for triangles: a cell's case is rebuilt from the below bits of its 8 corner codes, and each of its
//                             triangle's edges resolves to vbase[owner] + popcount(code[owner] below the edge's axis).
// Tiles are MC_TILE = 2048 consecutive points (256 lanes x 8 rounds); workspace = 5 bytes per point + 32 bytes per tile + the scan's scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/nero_hip.h"
#include "common.h"
#include "cub_calls.h"
#include "device_prims.h"
#include "mcubes_tables.h"
#include "ws_plan.h"

namespace {

using namespace nero_cub;
using namespace nero_prims;
using namespace nero_ws;

constexpr int MC_THREADS = 256;
constexpr int MC_ROUNDS = 8;
constexpr int64_t MC_TILE = (int64_t)MC_THREADS * MC_ROUNDS;
constexpr uint64_t MC_MAX_POINTS = 0xFFFFFFFFull;      // linear indices are decomposed in 32-bit arithmetic (1024^3 = 2^30)

struct McGrid {
    int nx, ny, nz;
    int64_t syz;      // ny * nz: the x stride
    int64_t n;        // nx * ny * nz
};

__device__ __forceinline__ void mc_coords(int64_t L, const McGrid& g, int& i, int& j, int& k) {
    const uint32_t l = (uint32_t)L, nz = (uint32_t)g.nz, ny = (uint32_t)g.ny;
    const uint32_t ij = l / nz;
    k = (int)(l - ij * nz);
    i = (int)(ij / ny);
    j = (int)(ij - (uint32_t)i * ny);
}

// exclusive prefix of v (0 <= v < 2^NBITS) over the 256 lanes of the workgroup, in lane order; *total = the workgroup's sum.
// Ends with a barrier, so `part` may be reused by the next call.
template <int NBITS>
__device__ __forceinline__ int mc_block_excl(int v, int* part, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    int excl = 0, wsum = 0;
#pragma unroll
    for (int b = 0; b < NBITS; ++b) {
        const uint64_t m = __ballot((v >> b) & 1);
        excl += __popcll(m & lt) << b;
        wsum += __popcll(m) << b;
    }
    if (lane == 0) part[w] = wsum;
    __syncthreads();
    int before = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < MC_THREADS / 64; ++q) {
        const int s = part[q];
        before += q < w ? s : 0;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return before + excl;
}

__global__ __launch_bounds__(MC_THREADS) void mc_count_kernel(const float* __restrict__ u, McGrid g, float thr, uint8_t* __restrict__ code,
                                                              int64_t* __restrict__ tile_v, int64_t* __restrict__ tile_t) {
    __shared__ int part[MC_THREADS / 64];
    const int64_t base = (int64_t)blockIdx.x * MC_TILE;
    int sv = 0, st = 0;
    for (int r = 0; r < MC_ROUNDS; ++r) {
        const int64_t L = base + r * MC_THREADS + threadIdx.x;
        if (L >= g.n) break;
        int i, j, k;
        mc_coords(L, g, i, j, k);
        const bool hx = i + 1 < g.nx, hy = j + 1 < g.ny, hz = k + 1 < g.nz;
        const bool b0 = u[L] < thr;
        const bool bx = hx ? u[L + g.syz] < thr : b0;           // (an absent edge never crosses)
        const bool by = hy ? u[L + g.nz] < thr : b0;
        const bool bz = hz ? u[L + 1] < thr : b0;
        const unsigned mask = (unsigned)(bx != b0) | (unsigned)(by != b0) << 1 | (unsigned)(bz != b0) << 2;
        code[L] = (uint8_t)(mask | (unsigned)b0 << 3);
        sv += __popc(mask);
        if (hx && hy && hz) {
            const unsigned cube = (unsigned)b0 | (unsigned)bx << 1 | (unsigned)(u[L + g.syz + g.nz] < thr) << 2 | (unsigned)by << 3 |
                                  (unsigned)bz << 4 | (unsigned)(u[L + g.syz + 1] < thr) << 5 |
                                  (unsigned)(u[L + g.syz + g.nz + 1] < thr) << 6 | (unsigned)(u[L + g.nz + 1] < thr) << 7;
            if (cube != 0 && cube != 255) st += nero_mcubes_tri_count[cube];
        }
    }
    const int tv = block_sum<MC_THREADS>(sv, part);
    const int tt = block_sum<MC_THREADS>(st, part);
    if (threadIdx.x == 0) {
        tile_v[blockIdx.x] = tv;
        tile_t[blockIdx.x] = tt;
    }
}

// base_v / base_t: exclusive scans of the tile totals over n_tiles + 1 entries -> {V, T} = entry n_tiles
__global__ void mc_totals_kernel(const int64_t* __restrict__ base_v, const int64_t* __restrict__ base_t, int64_t n_tiles,
                                 int64_t* __restrict__ ws_totals, int64_t* __restrict__ totals) {
    const int q = threadIdx.x;
    if (q < 2) {
        const int64_t x = (q == 0 ? base_v : base_t)[n_tiles];
        ws_totals[q] = x;
        if (totals) totals[q] = x;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_vert_kernel(const float* __restrict__ u, McGrid g, float thr, const uint8_t* __restrict__ code,
                                                             const int64_t* __restrict__ base_v, int* __restrict__ vbase,
                                                             float* __restrict__ verts, int64_t v_cap) {
    __shared__ int part[MC_THREADS / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * MC_TILE;
    int64_t carry = base_v[blockIdx.x];
    for (int r = 0; r < MC_ROUNDS; ++r) {
        const int64_t L = tile0 + r * MC_THREADS + threadIdx.x;
        if (tile0 + r * MC_THREADS >= g.n) break;                // (uniform over the workgroup: the barriers below stay matched)
        const unsigned mask = L < g.n ? code[L] & 7u : 0u;
        int total;
        const int excl = mc_block_excl<2>(__popc(mask), part, &total);
        if (mask) {
            int64_t vid = carry + excl;
            vbase[L] = (int)vid;                                   // (V < 2^31: checked by nero_mcubes_emit before the launch)
            int i, j, k;
            mc_coords(L, g, i, j, k);
            const float u0 = u[L];
            const int64_t stride[3] = {g.syz, (int64_t)g.nz, 1};
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (!(mask >> a & 1u)) continue;
                const float t = (thr - u0) / (u[L + stride[a]] - u0);
                if (vid < v_cap) {
                    float* o = verts + 3 * vid;
                    o[0] = a == 0 ? (float)i + t : (float)i;
                    o[1] = a == 1 ? (float)j + t : (float)j;
                    o[2] = a == 2 ? (float)k + t : (float)k;
                }
                ++vid;
            }
        }
        carry += total;
    }
}

// linear offset of cell corner c from the cell's min corner: x for corners 1,2,5,6 (mask 0x66), y for 2,3,6,7 (0xCC), z for 4-7
__device__ __forceinline__ int64_t mc_corner_offset(int c, const McGrid& g) {
    return ((0x66 >> c) & 1) * g.syz + ((0xCC >> c) & 1) * (int64_t)g.nz + (c >> 2);
}

// edge e of a cell -> (corner owning it, axis), corners and edges numbered as in mcubes_tables.h; packed 3 + 2 bits per edge
constexpr uint64_t mc_edge_owner_bits() {
    const int corner[12] = {0, 1, 3, 0, 4, 5, 7, 4, 0, 1, 2, 3};
    const int axis[12] = {0, 1, 0, 1, 0, 1, 0, 1, 2, 2, 2, 2};
    uint64_t x = 0;
    for (int e = 0; e < 12; ++e) x |= (uint64_t)(corner[e] | axis[e] << 3) << (5 * e);
    return x;
}
constexpr uint64_t MC_EDGE_OWNER = mc_edge_owner_bits();

__global__ __launch_bounds__(MC_THREADS) void mc_tri_kernel(McGrid g, const uint8_t* __restrict__ code, const int* __restrict__ vbase,
                                                            const int64_t* __restrict__ base_t, int* __restrict__ tris, int64_t t_cap) {
    __shared__ int part[MC_THREADS / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * MC_TILE;
    int64_t carry = base_t[blockIdx.x];
    for (int r = 0; r < MC_ROUNDS; ++r) {
        const int64_t L = tile0 + r * MC_THREADS + threadIdx.x;
        if (tile0 + r * MC_THREADS >= g.n) break;
        unsigned cube = 0;
        uint64_t codes = 0;                                         // code byte of corner c at bits 8c..8c+7
        if (L < g.n) {
            int i, j, k;
            mc_coords(L, g, i, j, k);
            if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const unsigned cc = code[L + mc_corner_offset(c, g)];
                    codes |= (uint64_t)cc << (8 * c);
                    cube |= (cc >> 3 & 1u) << c;
                }
            }
        }
        const int nt = (cube != 0 && cube != 255) ? nero_mcubes_tri_count[cube] : 0;
        int total;
        const int excl = mc_block_excl<3>(nt, part, &total);
        const int64_t t0 = carry + excl;
        for (int q = 0; q < nt; ++q) {
            if (t0 + q >= t_cap) break;
            int* o = tris + 3 * (t0 + q);
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int edge = nero_mcubes_tri_table[cube][3 * q + e];
                const unsigned ow = (unsigned)(MC_EDGE_OWNER >> (5 * edge)) & 31u;
                const int c = ow & 7, a = ow >> 3;
                const unsigned cc = (unsigned)(codes >> (8 * c)) & 0xffu;
                o[e] = vbase[L + mc_corner_offset(c, g)] + __popc(cc & ((1u << a) - 1u));
            }
        }
        carry += total;
    }
}

bool degenerate(int nx, int ny, int nz) { return nx < 2 || ny < 2 || nz < 2; }

int64_t n_tiles_of(int64_t n) { return (n + MC_TILE - 1) / MC_TILE; }

struct McLayout {
    int64_t n, n_tiles;
    size_t hdr, code, vbase, tile_v, tile_t, base_v, base_t, temp, temp_bytes, total;
};

int layout(int nx, int ny, int nz, McLayout* w) {
    *w = McLayout{};
    w->n = (int64_t)nx * ny * nz;
    Carve c;
    w->hdr = c.take(256);                                           // header: int64 {V, T}
    if (!degenerate(nx, ny, nz)) {
        w->n_tiles = n_tiles_of(w->n);
        if (scan_temp<int64_t>(w->n_tiles + 1, &w->temp_bytes) != hipSuccess)
            return nero_fail(NERO_ERR_LAUNCH, "nero_mcubes: the scratch-size query of the tile scan failed");
        const size_t tiles = (size_t)(w->n_tiles + 1) * sizeof(int64_t);
        w->code = c.take((size_t)w->n);
        w->vbase = c.take((size_t)w->n * sizeof(int));
        w->tile_v = c.take(tiles);
        w->tile_t = c.take(tiles);
        w->base_v = c.take(tiles);
        w->base_t = c.take(tiles);
        w->temp = c.take(w->temp_bytes);
    }
    w->total = c.at;
    return NERO_OK;
}

McGrid grid_of(int nx, int ny, int nz) { return McGrid{nx, ny, nz, (int64_t)ny * nz, (int64_t)nx * ny * nz}; }

// NERO_OK, or the error of a grid the entry points refuse
int check_dims(const char* fn, int nx, int ny, int nz) {
    static thread_local char msg[160];
    if (nx < 1 || ny < 1 || nz < 1) {
        snprintf(msg, sizeof(msg), "%s: grid %d x %d x %d: every size must be >= 1", fn, nx, ny, nz);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if ((uint64_t)nx * (uint64_t)ny * (uint64_t)nz > MC_MAX_POINTS) {
        snprintf(msg, sizeof(msg), "%s: grid %d x %d x %d: 2^32 or more points", fn, nx, ny, nz);
        return nero_fail(NERO_ERR_UNSUPPORTED, msg);
    }
    return NERO_OK;
}

}  // namespace

size_t nero_mcubes_workspace_bytes(int nx, int ny, int nz) {
    if (check_dims("nero_mcubes_workspace_bytes", nx, ny, nz)) return 0;
    McLayout L;
    return layout(nx, ny, nz, &L) == NERO_OK ? L.total : 0;
}

int nero_mcubes_count(const float* u, int nx, int ny, int nz, float threshold, void* ws, int64_t* totals, void* stream) {
    if (int rc = check_dims("nero_mcubes_count", nx, ny, nz)) return rc;
    if (!u || !ws || !totals) return nero_fail(NERO_ERR_ARG, "nero_mcubes_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    if (degenerate(nx, ny, nz)) {                                   // no cell: the empty mesh
        if (hipMemsetAsync(w, 0, 2 * sizeof(int64_t), s) != hipSuccess || hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), s) != hipSuccess)
            return nero_fail(NERO_ERR_LAUNCH, "nero_mcubes_count: hipMemsetAsync failed");
        return NERO_OK;
    }
    McLayout L;
    if (int rc = layout(nx, ny, nz, &L)) return rc;
    const McGrid g = grid_of(nx, ny, nz);
    int64_t* tile_v = (int64_t*)(w + L.tile_v);
    int64_t* tile_t = (int64_t*)(w + L.tile_t);
    // the scans' trailing entry: exclusive prefix over n_tiles + 1 items ends in the grand total
    if (hipMemsetAsync(tile_v + L.n_tiles, 0, sizeof(int64_t), s) != hipSuccess || hipMemsetAsync(tile_t + L.n_tiles, 0, sizeof(int64_t), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_mcubes_count: hipMemsetAsync failed");
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)L.n_tiles), dim3(MC_THREADS), 0, s, u, g, threshold, w + L.code, tile_v, tile_t);
    if (int rc = nero_check_launch("nero_mcubes_count: count pass")) return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int64_t*)tile_v, (int64_t*)(w + L.base_v), L.n_tiles + 1, s, "nero_mcubes_count: vertex scan failed"))
        return rc;
    if (int rc = exclusive_sum(w + L.temp, L.temp_bytes, (const int64_t*)tile_t, (int64_t*)(w + L.base_t), L.n_tiles + 1, s, "nero_mcubes_count: triangle scan failed"))
        return rc;
    hipLaunchKernelGGL(mc_totals_kernel, dim3(1), dim3(64), 0, s, (const int64_t*)(w + L.base_v), (const int64_t*)(w + L.base_t), L.n_tiles,
                       (int64_t*)(w + L.hdr), totals);
    return nero_check_launch("nero_mcubes_count");
}

int nero_mcubes_emit(const float* u, int nx, int ny, int nz, float threshold, void* ws, float* verts, int64_t v_cap, int* tris, int64_t t_cap,
                     void* stream) {
    if (int rc = check_dims("nero_mcubes_emit", nx, ny, nz)) return rc;
    if (!u || !ws || v_cap < 0 || t_cap < 0) return nero_fail(NERO_ERR_ARG, "nero_mcubes_emit: null pointer or negative capacity");
    if (degenerate(nx, ny, nz)) return NERO_OK;                    // the empty mesh: nothing to write
    hipStream_t s = (hipStream_t)stream;
    uint8_t* w = (uint8_t*)ws;
    McLayout L;
    if (int rc = layout(nx, ny, nz, &L)) return rc;
    const McGrid g = grid_of(nx, ny, nz);
    // the one synchronisation of this file: the 16-byte totals nero_mcubes_count left in the workspace, so that a mesh that does not fit the
    // caller's buffers (or whose ids would not fit int32) is an error code and not a write out of range
    int64_t tot[2] = {-1, -1};
    if (int rc = read_back(tot, w + L.hdr, sizeof(tot), s, "nero_mcubes_emit: reading the totals of nero_mcubes_count failed")) return rc;
    const int64_t V = tot[0], T = tot[1];
    if (V < 0 || T < 0 || V > 3 * L.n || T > 5 * L.n)
        return nero_fail(NERO_ERR_ARG, "nero_mcubes_emit: the workspace holds no totals of nero_mcubes_count for this grid");
    if (V >= ((int64_t)1 << 31) || T >= ((int64_t)1 << 31))
        return nero_fail(NERO_ERR_UNSUPPORTED, "nero_mcubes_emit: the mesh has 2^31 or more vertices or triangles (int32 ids)");
    if (V > v_cap || T > t_cap) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_mcubes_emit: mesh of %lld vertices / %lld triangles exceeds the capacity %lld / %lld", (long long)V,
                 (long long)T, (long long)v_cap, (long long)t_cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if ((V > 0 && !verts) || (T > 0 && !tris)) return nero_fail(NERO_ERR_ARG, "nero_mcubes_emit: null output pointer");
    if (V == 0) return NERO_OK;                                     // (no crossing edge: no vertex, no triangle)
    const dim3 grid((unsigned)L.n_tiles);
    hipLaunchKernelGGL(mc_vert_kernel, grid, dim3(MC_THREADS), 0, s, u, g, threshold, (const uint8_t*)(w + L.code),
                       (const int64_t*)(w + L.base_v), (int*)(w + L.vbase), verts, v_cap);
    if (int rc = nero_check_launch("nero_mcubes_emit: vertex pass")) return rc;
    if (T == 0) return NERO_OK;
    hipLaunchKernelGGL(mc_tri_kernel, grid, dim3(MC_THREADS), 0, s, g, (const uint8_t*)(w + L.code), (const int*)(w + L.vbase),
                       (const int64_t*)(w + L.base_t), tris, t_cap);
    return nero_check_launch("nero_mcubes_emit: triangle pass");
}
