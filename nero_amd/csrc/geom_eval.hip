// geom_eval.hip -- the geometry evaluation of the extracted mesh on the device (include/nero_hip.h, "geometry evaluation").
//
// Replaces the reference's Chamfer procedure (eval_synthetic_shape.py, eval_real_shape.py, dataset/database.py:435-458), which needs nvdiffrast,
// open3d and trimesh:
//   nero_nn_dist           eval_synthetic_shape.py:16-25 (nearest_dist): exact brute-force nearest neighbour.  Reference points staged in LDS
//                          tiles and read at wave-uniform addresses (broadcast), NN_Q query points per lane in registers, the reference set
//                          split over gridDim.y workgroups with a second pass taking the minimum over the splits.  The squared distance of a
//                          pair is one fixed fp32 expression and ties go to the lowest j, so the result does not depend on the launch shape.
//   nero_voxel_downsample  open3d's voxel_down_sample (eval_synthetic_shape.py:79-82, database.py:451-456) made deterministic: float64 keys,
//                          a stable radix sort of (key, input index), head flags + exclusive scan, one sequential float64 sum per voxel.
//   nero_view_rays /       primary rays through the pixel centres of a view (their hit distances from nero_bvh_trace stand in for
//   nero_view_points /     rasterize_depth_map, eval_synthetic_shape.py:39-60), camera-space depth + mask, and mask_depth_to_pts + pose_inverse +
//   nero_depth_points      pose_apply (utils/base_utils.py:44-52, 562-565, 583-584) with the points compacted in row-major pixel order by a
//                          prefix sum.
// No atomics decide a value or a position anywhere in this file: two runs are bit-identical.
#include <hip/hip_runtime.h>
#include <math.h>
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

// ---- nearest neighbour ---------------------------------------------------------------------------------------------------------------------
constexpr int NN_THREADS = 256;
constexpr int NN_Q = 8;                                  // query points per lane
constexpr int NN_QBLOCK = NN_THREADS * NN_Q;             // query points per workgroup
constexpr int NN_TILE = 1024;                            // reference points per LDS tile (16 KiB as float4)
constexpr int NN_MAX_SPLITS = 4096;
constexpr int64_t NN_TARGET_BLOCKS = 2048;               // 256 CUs x 8 workgroups of 4 waves: two rounds of 4 resident workgroups per CU

// One workgroup: the NN_QBLOCK queries from blockIdx.x * NN_QBLOCK against the reference points [blockIdx.y * per_split, + per_split).
// Lane l holds queries base + l + 256 k (coalesced loads and stores).  best2 / besti [gridDim.y][nq].
template <bool WANT_IDX>
__global__ __launch_bounds__(NN_THREADS) void nn_partial_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ r, int64_t nr,
                                                                int64_t per_split, float* __restrict__ best2, int* __restrict__ besti) {
    __shared__ float4 tile[NN_TILE];
    const int64_t q0 = (int64_t)blockIdx.x * NN_QBLOCK + threadIdx.x;
    const int64_t r_begin = (int64_t)blockIdx.y * per_split;
    const int64_t r_end = r_begin + per_split < nr ? r_begin + per_split : nr;
    float qx[NN_Q], qy[NN_Q], qz[NN_Q], best[NN_Q];
    int bi[NN_Q];
#pragma unroll
    for (int k = 0; k < NN_Q; ++k) {
        int64_t i = q0 + (int64_t)k * NN_THREADS;
        i = i < nq ? i : nq - 1;                                        // (lanes past the end repeat the last query and store nothing)
        qx[k] = q[3 * i];
        qy[k] = q[3 * i + 1];
        qz[k] = q[3 * i + 2];
        best[k] = INFINITY;
        bi[k] = (int)r_begin;
    }
    for (int64_t t0 = r_begin; t0 < r_end; t0 += NN_TILE) {
        const int cnt = (int)(r_end - t0 < NN_TILE ? r_end - t0 : NN_TILE);
        __syncthreads();                                                // the previous tile has been read by every wave
        for (int j = threadIdx.x; j < cnt; j += NN_THREADS) {
            const float* p = r + 3 * (t0 + j);
            tile[j] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; ++j) {
            const float4 p = tile[j];                                   // one address for the whole wave: an LDS broadcast
#pragma unroll
            for (int k = 0; k < NN_Q; ++k) {
                const float dx = qx[k] - p.x, dy = qy[k] - p.y, dz = qz[k] - p.z;
                const float d2 = fmaf(dz, dz, fmaf(dy, dy, nero_mul_rn(dx, dx)));
                if constexpr (WANT_IDX) {
                    const bool lt = d2 < best[k];                       // strict: the lowest j among equal squared distances stays
                    best[k] = lt ? d2 : best[k];
                    bi[k] = lt ? (int)(t0 + j) : bi[k];
                } else {
                    best[k] = fminf(best[k], d2);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_Q; ++k) {
        const int64_t i = q0 + (int64_t)k * NN_THREADS;
        if (i < nq) {
            best2[(int64_t)blockIdx.y * nq + i] = best[k];
            if constexpr (WANT_IDX) besti[(int64_t)blockIdx.y * nq + i] = bi[k];
        }
    }
}

// minimum over the splits in ascending order of their reference ranges (strict <: the lowest j among equals), then the one square root
__global__ __launch_bounds__(256) void nn_final_kernel(const float* __restrict__ best2, const int* __restrict__ besti, int64_t nq, int splits,
                                                       float* __restrict__ dist, int* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    float b = best2[i];
    int s_best = 0;
    for (int s = 1; s < splits; ++s) {
        const float v = best2[(int64_t)s * nq + i];
        if (v < b) {
            b = v;
            s_best = s;
        }
    }
    dist[i] = __fsqrt_rn(b);
    if (idx) idx[i] = besti[(int64_t)s_best * nq + i];
}

int nn_auto_splits(int64_t nq, int64_t nr) {
    const int64_t qblocks = (nq + NN_QBLOCK - 1) / NN_QBLOCK;
    const int64_t tiles = (nr + NN_TILE - 1) / NN_TILE;
    int64_t s = (NN_TARGET_BLOCKS + qblocks - 1) / qblocks;
    if (s > tiles) s = tiles;
    if (s > NN_MAX_SPLITS) s = NN_MAX_SPLITS;
    return s < 1 ? 1 : (int)s;
}

// ---- voxel down-sample ---------------------------------------------------------------------------------------------------------------------
constexpr int VX_THREADS = 256;
constexpr int VX_MAX_PARTIALS = 1024;
constexpr int VX_AXIS_BITS = 21;
constexpr double VX_AXIS_LIMIT = 2097152.0;              // 2^21 voxels per axis

struct VxHeader {                 // first 256 bytes of the workspace
    float mn[3];
    int overflow;                 // some axis spans more than 2^21 voxels
    int64_t n_out;
};

struct VxLayout {
    size_t hdr, partial, keys_a, keys_b, vals_a, vals_b, temp, temp_bytes, total;
    // after the sort: head flags live in keys_a, their exclusive scan in vals_a
};

int vx_layout(int64_t n, VxLayout* w) {
    *w = VxLayout{};
    size_t a = 0, b = 0;
    if (n > 0 && (sort_pairs_temp<uint64_t>(n, 3 * VX_AXIS_BITS, &a) != hipSuccess || scan_temp<int>(n + 1, &b) != hipSuccess))
        return nero_fail(NERO_ERR_LAUNCH, "nero_voxel_downsample: the scratch-size query of the radix sort or the scan failed");
    Carve c{256};
    w->partial = c.take((size_t)VX_MAX_PARTIALS * 6 * sizeof(float));
    if (n > 0) {
        w->keys_a = c.take((size_t)(n + 1) * sizeof(uint64_t));
        w->keys_b = c.take((size_t)n * sizeof(uint64_t));
        w->vals_a = c.take((size_t)(n + 1) * sizeof(uint32_t));
        w->vals_b = c.take((size_t)n * sizeof(uint32_t));
        w->temp_bytes = a > b ? a : b;
        w->temp = c.take(w->temp_bytes);
    }
    w->total = c.at;
    return NERO_OK;
}

// block-wide {min x, y, z, max x, y, z} of m[6] -> thread 0's m (minimum / maximum do not depend on the order they are taken in)
__device__ __forceinline__ void vx_block_bounds(float* m, float (*part)[6]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        m[a] = wave_min(m[a]);
        m[3 + a] = wave_max(m[3 + a]);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
        for (int a = 0; a < 6; ++a) part[w][a] = m[a];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < VX_THREADS / 64; ++q)
            for (int a = 0; a < 3; ++a) {
                m[a] = fminf(m[a], part[q][a]);
                m[3 + a] = fmaxf(m[3 + a], part[q][3 + a]);
            }
}

__global__ __launch_bounds__(VX_THREADS) void vx_bounds_kernel(const float* __restrict__ pts, int64_t n, float* __restrict__ partial) {
    __shared__ float part[VX_THREADS / 64][6];
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * VX_THREADS)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * i + a];
            m[a] = fminf(m[a], v);
            m[3 + a] = fmaxf(m[3 + a], v);
        }
    vx_block_bounds(m, part);
    if (threadIdx.x == 0)
        for (int a = 0; a < 6; ++a) partial[6 * blockIdx.x + a] = m[a];
}

__device__ __forceinline__ double vx_index(float p, float mn, double voxel) {
    const double o = (double)mn - voxel * 0.5;
    return floor(((double)p - o) / voxel);
}

__global__ __launch_bounds__(VX_THREADS) void vx_bounds_final_kernel(const float* __restrict__ partial, int n_partial, double voxel,
                                                                     VxHeader* __restrict__ hdr) {
    __shared__ float part[VX_THREADS / 64][6];
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < n_partial; i += VX_THREADS)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            m[a] = fminf(m[a], partial[6 * i + a]);
            m[3 + a] = fmaxf(m[3 + a], partial[6 * i + 3 + a]);
        }
    vx_block_bounds(m, part);
    if (threadIdx.x == 0) {
        int over = 0;
        for (int a = 0; a < 3; ++a) {
            hdr->mn[a] = m[a];
            const double top = vx_index(m[3 + a], m[a], voxel);
            if (!(top < VX_AXIS_LIMIT)) over = 1;                       // (also a NaN / infinite extent)
        }
        hdr->overflow = over;
        hdr->n_out = 0;
    }
}

__global__ __launch_bounds__(VX_THREADS) void vx_key_kernel(const float* __restrict__ pts, int64_t n, double voxel, const VxHeader* __restrict__ hdr,
                                                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double f = vx_index(pts[3 * i + a], hdr->mn[a], voxel);
        f = f >= 0.0 ? f : 0.0;                                         // (NaN -> 0; a range that does not fit is refused before the keys are used)
        f = f < VX_AXIS_LIMIT ? f : VX_AXIS_LIMIT - 1.0;
        key = key << VX_AXIS_BITS | (uint64_t)f;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// flag [n + 1]: 1 at the first point of every voxel in sorted order, flag[n] = 0 (its exclusive scan ends in the voxel count)
__global__ __launch_bounds__(VX_THREADS) void vx_head_kernel(const uint64_t* __restrict__ keys, int64_t n, int* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x;
    if (i > n) return;
    flag[i] = i == n ? 0 : (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ void vx_total_kernel(const int* __restrict__ seg, int64_t n, VxHeader* __restrict__ hdr, int64_t* __restrict__ n_out) {
    if (threadIdx.x == 0) {
        hdr->n_out = seg[n];
        if (n_out) *n_out = seg[n];
    }
}

// the lane at a voxel's first sorted point sums the voxel's points in sorted order -- the sort is stable, so in ascending input index -- in
// float64 and writes the mean as float32 at the voxel's rank
__global__ __launch_bounds__(VX_THREADS) void vx_mean_kernel(const float* __restrict__ pts, int64_t n, const int* __restrict__ flag,
                                                             const int* __restrict__ seg, const uint32_t* __restrict__ vals,
                                                             float* __restrict__ out, int64_t out_cap) {
    const int64_t i = (int64_t)blockIdx.x * VX_THREADS + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int64_t o = seg[i];
    if (o >= out_cap) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int64_t j = i;
    do {
        const float* p = pts + 3 * (int64_t)vals[j];
        sx += (double)p[0];
        sy += (double)p[1];
        sz += (double)p[2];
        ++j;
    } while (j < n && !flag[j]);
    const double cnt = (double)(j - i);
    out[3 * o] = (float)(sx / cnt);
    out[3 * o + 1] = (float)(sy / cnt);
    out[3 * o + 2] = (float)(sz / cnt);
}

// ---- views ---------------------------------------------------------------------------------------------------------------------------------
struct ViewCam {
    double iK[9];        // inv(K), row-major
    double R[9];         // world -> camera rotation, row-major
    double c[3];         // camera centre = pose_inverse's translation = -R^T t
};

bool view_cam(const double* K, const double* pose, ViewCam* cam) {
    const double a = K[0], b = K[1], c = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
    const double inv[9] = {(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det, (f * g - d * i) / det, (a * i - c * g) / det,
                           (c * d - a * f) / det, (d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det};
    for (int k = 0; k < 9; ++k) cam->iK[k] = inv[k];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) cam->R[3 * r + k] = pose[4 * r + k];
    for (int k = 0; k < 3; ++k) cam->c[k] = -(pose[k] * pose[3] + pose[4 + k] * pose[7] + pose[8 + k] * pose[11]);
    return true;
}

// inv(K) (x + 0.5, y + 0.5, 1): the camera-space direction through the centre of pixel (x, y), not normalised
__device__ __forceinline__ void view_dir_cam(const ViewCam& cam, int x, int y, double* d) {
    const double px = (double)x + 0.5, py = (double)y + 0.5;
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = cam.iK[3 * r] * px + cam.iK[3 * r + 1] * py + cam.iK[3 * r + 2];
}

__global__ __launch_bounds__(256) void view_rays_kernel(ViewCam cam, int w, int n, float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double dc[3], dw[3];
    view_dir_cam(cam, p % w, p / w, dc);
#pragma unroll
    for (int k = 0; k < 3; ++k) dw[k] = cam.R[k] * dc[0] + cam.R[3 + k] * dc[1] + cam.R[6 + k] * dc[2];      // R^T d
    const double inv = 1.0 / sqrt(dw[0] * dw[0] + dw[1] * dw[1] + dw[2] * dw[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        rays_o[3 * p + k] = (float)cam.c[k];
        rays_d[3 * p + k] = (float)(dw[k] * inv);
    }
}

// hit distance along the unit ray -> camera-space z; the tracer reports a miss as t = 10
__global__ __launch_bounds__(256) void view_depth_kernel(const float* __restrict__ t, ViewCam cam, int w, int n, float* __restrict__ depth,
                                                         unsigned char* __restrict__ mask) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    double dc[3];
    view_dir_cam(cam, p % w, p / w, dc);
    const float tt = t[p];
    const bool hit = tt < 10.0f;
    depth[p] = hit ? (float)((double)tt * (dc[2] / sqrt(dc[0] * dc[0] + dc[1] * dc[1] + dc[2] * dc[2]))) : 0.0f;
    mask[p] = hit ? 1 : 0;
}

__global__ __launch_bounds__(256) void view_flag_kernel(const unsigned char* __restrict__ mask, int n, int* __restrict__ flag) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    flag[p] = p < n && mask[p] ? 1 : 0;
}

// mask_depth_to_pts + pose_apply(pose_inverse(pose), .) for the masked pixels, at their rank in row-major order.  As the reference does:
// the pixel coordinates and the depth are float32, x z and y z are float32 products (utils/base_utils.py:47-48), everything after that float64.
__global__ __launch_bounds__(256) void view_points_kernel(const float* __restrict__ depth, const int* __restrict__ flag, const int* __restrict__ rank,
                                                          ViewCam cam, int w, int n, float offset, float* __restrict__ pts, int64_t cap,
                                                          int64_t* __restrict__ n_pts) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && n_pts) *n_pts = rank[n];
    if (p >= n || !flag[p]) return;
    const int64_t o = rank[p];
    if (o >= cap) return;
    const float z = depth[p];
    const double v[3] = {(double)nero_mul_rn((float)(p % w) + offset, z), (double)nero_mul_rn((float)(p / w) + offset, z), (double)z};
    double pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = v[0] * cam.iK[3 * r] + v[1] * cam.iK[3 * r + 1] + v[2] * cam.iK[3 * r + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) pts[3 * o + k] = (float)(pc[0] * cam.R[k] + pc[1] * cam.R[3 + k] + pc[2] * cam.R[6 + k] + cam.c[k]);
}

struct ViewLayout {
    size_t flag, rank, temp, temp_bytes, total;
};

int view_layout(int64_t n, ViewLayout* w) {
    if (scan_temp<int>(n + 1, &w->temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_view_points, nero_depth_points: the scratch-size query of the scan of the mask failed");
    Carve c;
    w->flag = c.take((size_t)(n + 1) * sizeof(int));
    w->rank = c.take((size_t)(n + 1) * sizeof(int));
    w->temp = c.take(w->temp_bytes);
    w->total = c.at;
    return NERO_OK;
}

int check_view(const char* fn, const double* K, const double* pose, int h, int w, ViewCam* cam) {
    static thread_local char msg[160];
    if (!K || !pose) {
        snprintf(msg, sizeof(msg), "%s: null K or pose", fn);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31) - 1) {
        snprintf(msg, sizeof(msg), "%s: view of %d x %d pixels: both sizes >= 1 and fewer than 2^31 - 1 pixels", fn, h, w);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (!view_cam(K, pose, cam)) {
        snprintf(msg, sizeof(msg), "%s: K is singular", fn);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
}

int depth_points(const char* fn, const float* depth, const unsigned char* mask, const ViewCam& cam, int h, int w, float offset, void* ws,
                 float* pts, int64_t cap, int64_t* n_pts, hipStream_t s) {
    const int n = h * w;
    ViewLayout L;
    if (int rc = view_layout(n, &L)) return rc;
    uint8_t* b = (uint8_t*)ws;
    int* flag = (int*)(b + L.flag);
    int* rank = (int*)(b + L.rank);
    const unsigned blocks = (unsigned)((n + 1 + 255) / 256);
    hipLaunchKernelGGL(view_flag_kernel, dim3(blocks), dim3(256), 0, s, mask, n, flag);
    if (int rc = nero_check_launch(fn)) return rc;
    if (int rc = exclusive_sum(b + L.temp, L.temp_bytes, (const int*)flag, rank, n + 1, s, "geometry evaluation: the scan of the mask failed")) return rc;
    hipLaunchKernelGGL(view_points_kernel, dim3(blocks), dim3(256), 0, s, depth, (const int*)flag, (const int*)rank, cam, w, n, offset, pts, cap,
                       n_pts);
    return nero_check_launch(fn);
}

}  // namespace

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
int nero_nn_dist_splits(int64_t nq, int64_t nr) {
    if (nq <= 0 || nr <= 0) return 1;
    return nn_auto_splits(nq, nr);
}

size_t nero_nn_dist_workspace_bytes(int64_t nq, int64_t nr, int splits) {
    if (nq <= 0 || nr <= 0) return 256;
    if (splits <= 0) splits = nn_auto_splits(nq, nr);
    if (splits > NN_MAX_SPLITS) return 0;
    return 2 * align256((size_t)splits * (size_t)nq * sizeof(float));
}

int nero_nn_dist(const float* q, int64_t nq, const float* r, int64_t nr, void* ws, int splits, float* dist, int* idx, void* stream) {
    static thread_local char msg[200];
    if (nq < 0 || nr < 0) return nero_fail(NERO_ERR_ARG, "nero_nn_dist: negative count");
    if (nq == 0) return NERO_OK;
    if (nr == 0) return nero_fail(NERO_ERR_ARG, "nero_nn_dist: no reference point (nr = 0): the nearest distance is undefined");
    if (!q || !r || !dist || !ws) return nero_fail(NERO_ERR_ARG, "nero_nn_dist: null pointer");
    if (idx && nr >= ((int64_t)1 << 31)) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_nn_dist: 2^31 or more reference points with int32 indices");
    if (splits <= 0) splits = nn_auto_splits(nq, nr);
    const int64_t qblocks = (nq + NN_QBLOCK - 1) / NN_QBLOCK;
    if (splits > NN_MAX_SPLITS || qblocks >= ((int64_t)1 << 31)) {
        snprintf(msg, sizeof(msg), "nero_nn_dist: %d splits (at most %d) / %lld query blocks", splits, NN_MAX_SPLITS, (long long)qblocks);
        return nero_fail(NERO_ERR_UNSUPPORTED, msg);
    }
    if ((int64_t)splits > nr) splits = (int)nr;
    // per_split: whole tiles, so that no split is empty
    int64_t per_split = (nr + splits - 1) / splits;
    per_split = (per_split + NN_TILE - 1) / NN_TILE * NN_TILE;
    splits = (int)((nr + per_split - 1) / per_split);
    hipStream_t s = (hipStream_t)stream;
    const size_t half = align256((size_t)splits * (size_t)nq * sizeof(float));
    float* best2 = (float*)ws;
    int* besti = (int*)((uint8_t*)ws + half);
    const dim3 grid((unsigned)qblocks, (unsigned)splits);
    if (idx)
        hipLaunchKernelGGL(nn_partial_kernel<true>, grid, dim3(NN_THREADS), 0, s, q, nq, r, nr, per_split, best2, besti);
    else
        hipLaunchKernelGGL(nn_partial_kernel<false>, grid, dim3(NN_THREADS), 0, s, q, nq, r, nr, per_split, best2, besti);
    if (int rc = nero_check_launch("nero_nn_dist: distance pass")) return rc;
    hipLaunchKernelGGL(nn_final_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const float*)best2, (const int*)besti, nq, splits,
                       dist, idx);
    return nero_check_launch("nero_nn_dist: minimum over the splits");
}

size_t nero_voxel_downsample_workspace_bytes(int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31) - 1) return no_workspace("nero_voxel_downsample_workspace_bytes: n must be in [0, 2^31 - 1)");
    VxLayout L;
    return vx_layout(n, &L) == NERO_OK ? L.total : 0;
}

int nero_voxel_downsample(const float* pts, int64_t n, double voxel, void* ws, float* out, int64_t out_cap, int64_t* n_out, void* stream) {
    static thread_local char msg[200];
    if (n < 0 || out_cap < 0) return nero_fail(NERO_ERR_ARG, "nero_voxel_downsample: negative count or capacity");
    if (!(voxel > 0.0) || !isfinite(voxel)) return nero_fail(NERO_ERR_ARG, "nero_voxel_downsample: the voxel size must be positive and finite");
    if (n >= ((int64_t)1 << 31) - 1) return nero_fail(NERO_ERR_UNSUPPORTED, "nero_voxel_downsample: 2^31 - 1 or more points");
    if (!ws) return nero_fail(NERO_ERR_ARG, "nero_voxel_downsample: null workspace");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    VxHeader* hdr = (VxHeader*)b;
    if (n == 0) {
        if (hipMemsetAsync(hdr, 0, sizeof(VxHeader), s) != hipSuccess || (n_out && hipMemsetAsync(n_out, 0, sizeof(int64_t), s) != hipSuccess))
            return nero_fail(NERO_ERR_LAUNCH, "nero_voxel_downsample: hipMemsetAsync failed");
        return NERO_OK;
    }
    if (!pts) return nero_fail(NERO_ERR_ARG, "nero_voxel_downsample: null points");
    VxLayout L;
    if (int rc = vx_layout(n, &L)) return rc;
    float* partial = (float*)(b + L.partial);
    uint64_t* keys_a = (uint64_t*)(b + L.keys_a);
    uint64_t* keys_b = (uint64_t*)(b + L.keys_b);
    uint32_t* vals_a = (uint32_t*)(b + L.vals_a);
    uint32_t* vals_b = (uint32_t*)(b + L.vals_b);
    const unsigned blocks = (unsigned)((n + VX_THREADS - 1) / VX_THREADS);
    const int n_partial = blocks < (unsigned)VX_MAX_PARTIALS ? (int)blocks : VX_MAX_PARTIALS;
    hipLaunchKernelGGL(vx_bounds_kernel, dim3(n_partial), dim3(VX_THREADS), 0, s, pts, n, partial);
    hipLaunchKernelGGL(vx_bounds_final_kernel, dim3(1), dim3(VX_THREADS), 0, s, (const float*)partial, n_partial, voxel, hdr);
    hipLaunchKernelGGL(vx_key_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, pts, n, voxel, (const VxHeader*)hdr, keys_a, vals_a);
    if (int rc = nero_check_launch("nero_voxel_downsample: keys")) return rc;
    if (int rc = sort_pairs<uint64_t>(b + L.temp, L.temp_bytes, keys_a, keys_b, vals_a, vals_b, n, 3 * VX_AXIS_BITS, s,
                                      "nero_voxel_downsample: the radix sort failed"))
        return rc;
    int* flag = (int*)keys_a;                                           // (n + 1 ints in the (n + 1) x 8 bytes of the unsorted keys)
    int* seg = (int*)vals_a;
    hipLaunchKernelGGL(vx_head_kernel, dim3((unsigned)((n + 1 + VX_THREADS - 1) / VX_THREADS)), dim3(VX_THREADS), 0, s, (const uint64_t*)keys_b, n,
                       flag);
    if (int rc = nero_check_launch("nero_voxel_downsample: head flags")) return rc;
    if (int rc = exclusive_sum(b + L.temp, L.temp_bytes, (const int*)flag, seg, n + 1, s, "nero_voxel_downsample: the scan failed")) return rc;
    hipLaunchKernelGGL(vx_total_kernel, dim3(1), dim3(64), 0, s, (const int*)seg, n, hdr, n_out);
    if (int rc = nero_check_launch("nero_voxel_downsample: total")) return rc;
    // the one synchronisation: the voxel count and the range flag, so that a cloud that does not fit is an error code and not a truncated result
    VxHeader host{};
    host.n_out = -1;
    if (int rc = read_back(&host, hdr, sizeof(VxHeader), s, "nero_voxel_downsample: reading the voxel count failed")) return rc;
    if (host.overflow)
        return nero_fail(NERO_ERR_UNSUPPORTED, "nero_voxel_downsample: the cloud spans more than 2^21 voxels on an axis (or holds a non-finite point)");
    if (host.n_out < 0 || host.n_out > n) return nero_fail(NERO_ERR_LAUNCH, "nero_voxel_downsample: implausible voxel count");
    if (host.n_out > out_cap) {
        snprintf(msg, sizeof(msg), "nero_voxel_downsample: %lld occupied voxels exceed the capacity %lld", (long long)host.n_out, (long long)out_cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (!out) return nero_fail(NERO_ERR_ARG, "nero_voxel_downsample: null output");
    hipLaunchKernelGGL(vx_mean_kernel, dim3(blocks), dim3(VX_THREADS), 0, s, pts, n, (const int*)flag, (const int*)seg, (const uint32_t*)vals_b, out,
                       out_cap);
    return nero_check_launch("nero_voxel_downsample: means");
}

int nero_view_rays(const double* K, const double* pose, int h, int w, float* rays_o, float* rays_d, void* stream) {
    ViewCam cam;
    if (int rc = check_view("nero_view_rays", K, pose, h, w, &cam)) return rc;
    if (!rays_o || !rays_d) return nero_fail(NERO_ERR_ARG, "nero_view_rays: null output");
    const int n = h * w;
    hipLaunchKernelGGL(view_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cam, w, n, rays_o, rays_d);
    return nero_check_launch("nero_view_rays");
}

size_t nero_view_points_workspace_bytes(int h, int w) {
    if (h < 1 || w < 1 || (int64_t)h * w >= ((int64_t)1 << 31) - 1)
        return no_workspace("nero_view_points_workspace_bytes: both sizes >= 1 and fewer than 2^31 - 1 pixels");
    ViewLayout L;
    return view_layout((int64_t)h * w, &L) == NERO_OK ? L.total : 0;
}

int nero_view_points(const float* t, const double* K, const double* pose, int h, int w, float unproject_offset, void* ws, float* depth,
                     unsigned char* mask, float* pts, int64_t pts_cap, int64_t* n_pts, void* stream) {
    ViewCam cam;
    if (int rc = check_view("nero_view_points", K, pose, h, w, &cam)) return rc;
    if (!t || !ws || !depth || !mask || (!pts && pts_cap > 0) || pts_cap < 0) return nero_fail(NERO_ERR_ARG, "nero_view_points: null pointer or negative capacity");
    const int n = h * w;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(view_depth_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, cam, w, n, depth, mask);
    if (int rc = nero_check_launch("nero_view_points: depth")) return rc;
    return depth_points("nero_view_points", depth, mask, cam, h, w, unproject_offset, ws, pts, pts_cap, n_pts, s);
}

int nero_depth_points(const float* depth, const unsigned char* mask, const double* K, const double* pose, int h, int w, float unproject_offset,
                      void* ws, float* pts, int64_t pts_cap, int64_t* n_pts, void* stream) {
    ViewCam cam;
    if (int rc = check_view("nero_depth_points", K, pose, h, w, &cam)) return rc;
    if (!depth || !mask || !ws || (!pts && pts_cap > 0) || pts_cap < 0) return nero_fail(NERO_ERR_ARG, "nero_depth_points: null pointer or negative capacity");
    return depth_points("nero_depth_points", depth, mask, cam, h, w, unproject_offset, ws, pts, pts_cap, n_pts, (hipStream_t)stream);
}
