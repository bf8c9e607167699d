// texture.hip -- baking the Stage-II materials into UV texture maps (include/nero_hip.h, nero_uv_* / nero_tex_*).
//
// Replaces the device-arithmetic steps of the reference's extract_materials_texture_map.py:
//   nero_uv_raster        dr.rasterize(glctx, uv, ft, (h, w))                                   (:89-99)
//   nero_uv_interp        dr.interpolate(v, rast, f), the mask and xyzs[mask]                   (:100-113)
//   nero_tex_quantize     feats[mask] = ...; linear_to_srgb; (feats * 255).astype(np.uint8)     (:127-133)
//   nero_tex_regions      binary_dilation(iterations=32) / binary_erosion(iterations=3)         (:136-141)
//   nero_tex_fill         NearestNeighbors(1, 'kd_tree').fit / kneighbors and the copy          (:143-149)
//   nero_tex_downsample2  cv2.resize(..., INTER_LINEAR) at an exact factor of two               (:157-160)
// The raster is binned by bounding-box size: a triangle whose clipped bounding box holds at most UV_SMALL texel centres is finished by the
// lane that set it up (a sub-texel triangle between centres costs one set-up and no store); every other triangle is cut into 8 x 8-texel
// blocks, the block counts are prefix-summed, and a fixed grid of waves walks the blocks, one texel per lane -- two triangles over a 4096^2
// map are 2 x 262144 equal work items.  Overlaps resolve by an unsigned atomicMin on the id (lowest triangle wins; order independent).
// Compaction (nero_uv_interp) is by prefix sum.  Nothing here uses floating-point atomics; every result is bit-identical run to run.
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

constexpr int TX_MAX_SIZE = 16384;
constexpr int TX_MAX_PAD = 64;
constexpr int TX_MAX_BORDER = 16;
constexpr int UV_SMALL = 16;                        // texel centres one lane still walks itself
constexpr int UV_BLOCK = 8;                         // a wave's work item: UV_BLOCK x UV_BLOCK texels
constexpr int UV_WALK_BLOCKS = 2048;                // fixed grid of the block walk: 256 CUs x 8 workgroups of 4 waves
constexpr double UV_COORD_LIMIT = 1073741824.0;     // |snapped coordinate| <= 2^30: every edge function stays below 2^63
constexpr int FILL_TILE = 16;

struct TxHeader {                 // first 256 bytes of the raster / interpolation workspaces
    int bad;                      // an index out of range was seen
    int pad_;
    int64_t count;                // covered texels (interpolation)
};

// ---- the coverage rule ---------------------------------------------------------------------------------------------------------------------
struct UvTri {
    int64_t x[3], y[3];           // snapped vertices, 1/256 texel units, wound so that a > 0
    int64_t a;                    // twice the area
    int x_lo, x_hi, y_lo, y_hi;   // texels whose centres lie in the bounding box, clipped to the map (empty when lo > hi)
    bool swapped;                 // vertices 1 and 2 were exchanged
};

// false: the triangle covers nothing (an index out of range, a coordinate that is not finite or beyond 2^30, zero area, an empty box)
__device__ __forceinline__ bool uv_setup(const float* __restrict__ vt, int64_t nvt, const int* __restrict__ ft, int64_t t, int h, int w,
                                         UvTri& s) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t i = ft[3 * t + k];
        if (i < 0 || i >= nvt) return false;
        const double fx = rint((double)vt[2 * i] * (double)w * 256.0);
        const double fy = rint((double)vt[2 * i + 1] * (double)h * 256.0);
        if (!(fabs(fx) <= UV_COORD_LIMIT) || !(fabs(fy) <= UV_COORD_LIMIT)) return false;
        s.x[k] = (int64_t)fx;
        s.y[k] = (int64_t)fy;
    }
    s.a = (s.x[1] - s.x[0]) * (s.y[2] - s.y[0]) - (s.x[2] - s.x[0]) * (s.y[1] - s.y[0]);
    if (s.a == 0) return false;
    s.swapped = s.a < 0;
    if (s.swapped) {
        const int64_t tx = s.x[1], ty = s.y[1];
        s.x[1] = s.x[2]; s.y[1] = s.y[2];
        s.x[2] = tx;     s.y[2] = ty;
        s.a = -s.a;
    }
    const int64_t mnx = min(s.x[0], min(s.x[1], s.x[2])), mxx = max(s.x[0], max(s.x[1], s.x[2]));
    const int64_t mny = min(s.y[0], min(s.y[1], s.y[2])), mxy = max(s.y[0], max(s.y[1], s.y[2]));
    // centre 256 i + 128 inside [mn, mx]  <=>  ceil((mn - 128) / 256) <= i <= floor((mx - 128) / 256); >> floors (arithmetic shift)
    s.x_lo = (int)max((int64_t)0, (mnx - 128 + 255) >> 8);
    s.x_hi = (int)min((int64_t)w - 1, (mxx - 128) >> 8);
    s.y_lo = (int)max((int64_t)0, (mny - 128 + 255) >> 8);
    s.y_hi = (int)min((int64_t)h - 1, (mxy - 128) >> 8);
    return s.x_lo <= s.x_hi && s.y_lo <= s.y_hi;
}

// edge function of the directed edge a -> b at p, and whether p counts as inside of it
__device__ __forceinline__ bool uv_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py, int64_t& e) {
    const int64_t dx = bx - ax, dy = by - ay;
    e = dx * (py - ay) - dy * (px - ax);
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

// texel (row y, column x): e[k] = the edge function opposite vertex k (the weight of vertex k; e[0] + e[1] + e[2] = a)
__device__ __forceinline__ bool uv_inside(const UvTri& s, int x, int y, int64_t* e) {
    const int64_t px = 256 * (int64_t)x + 128, py = 256 * (int64_t)y + 128;
    const bool i0 = uv_edge(s.x[1], s.y[1], s.x[2], s.y[2], px, py, e[0]);
    const bool i1 = uv_edge(s.x[2], s.y[2], s.x[0], s.y[0], px, py, e[1]);
    const bool i2 = uv_edge(s.x[0], s.y[0], s.x[1], s.y[1], px, py, e[2]);
    return i0 && i1 && i2;
}

__global__ __launch_bounds__(256) void tx_index_check_kernel(const int* __restrict__ idx, int64_t n, int64_t limit, TxHeader* __restrict__ hdr) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t v = idx[i];
    if (v < 0 || v >= limit) hdr->bad = 1;
}

// one lane per triangle: small boxes are rasterised here, the others counted in blocks of UV_BLOCK^2 texels (cnt[nt] = 0 for the scan)
// COUNT: the same walk adds one to the texel's cover count instead (nero_uv_overlap_count; sums of integers do not depend on arrival order)
template <bool COUNT>
__device__ __forceinline__ void uv_cover(unsigned* __restrict__ map, int64_t texel, int64_t t) {
    if (COUNT) atomicAdd(map + texel, 1u);
    else atomicMin(map + texel, (unsigned)t);
}

template <bool COUNT>
__global__ __launch_bounds__(256) void uv_small_kernel(const float* __restrict__ vt, int64_t nvt, const int* __restrict__ ft, int64_t nt, int h,
                                                       int w, unsigned* __restrict__ tri_id, int64_t* __restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > nt) return;
    int64_t blocks = 0;
    UvTri s;
    if (t < nt && uv_setup(vt, nvt, ft, t, h, w, s)) {
        const int bw = s.x_hi - s.x_lo + 1, bh = s.y_hi - s.y_lo + 1;
        if ((int64_t)bw * bh <= UV_SMALL) {
            for (int y = s.y_lo; y <= s.y_hi; ++y)
                for (int x = s.x_lo; x <= s.x_hi; ++x) {
                    int64_t e[3];
                    if (uv_inside(s, x, y, e)) uv_cover<COUNT>(tri_id, (int64_t)y * w + x, t);
                }
        } else {
            blocks = (int64_t)((bw + UV_BLOCK - 1) / UV_BLOCK) * ((bh + UV_BLOCK - 1) / UV_BLOCK);
        }
    }
    cnt[t] = blocks;
}

// base: exclusive scan of cnt over nt + 1 entries.  Wave g takes the blocks g, g + waves, ...; block b belongs to the last triangle whose
// base is <= b (an upper bound search: the triangles without blocks in between share the base of the next one and are skipped by it).
template <bool COUNT>
__global__ __launch_bounds__(256) void uv_walk_kernel(const float* __restrict__ vt, int64_t nvt, const int* __restrict__ ft, int64_t nt, int h,
                                                      int w, const int64_t* __restrict__ base, unsigned* __restrict__ tri_id) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    const int64_t total = base[nt];
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < total; b += waves) {
        int64_t lo = 0, hi = nt;                      // first entry > b lies in (lo, hi]; base[0] = 0 <= b < base[nt]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (base[mid] <= b) lo = mid; else hi = mid;
        }
        const int64_t t = lo;
        UvTri s;
        if (!uv_setup(vt, nvt, ft, t, h, w, s)) continue;       // (cannot happen: the same set-up counted the blocks)
        const int nbx = (s.x_hi - s.x_lo + UV_BLOCK) / UV_BLOCK;
        const int64_t k = b - base[t];
        const int x = s.x_lo + (int)(k % nbx) * UV_BLOCK + (lane & (UV_BLOCK - 1));
        const int y = s.y_lo + (int)(k / nbx) * UV_BLOCK + (lane >> 3);
        int64_t e[3];
        if (x <= s.x_hi && y <= s.y_hi && uv_inside(s, x, y, e)) uv_cover<COUNT>(tri_id, (int64_t)y * w + x, t);
    }
}

// texels whose cover count exceeds one: a sum per workgroup, then one integer atomic
__global__ __launch_bounds__(256) void uv_overlap_sum_kernel(const unsigned* __restrict__ cover, int64_t n, unsigned long long* count) {
    __shared__ int part[4];
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int v = wave_sum(p < n && cover[p] > 1u ? 1 : 0);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = part[0] + part[1] + part[2] + part[3];
        if (tot) atomicAdd(count, (unsigned long long)tot);
    }
}

// ---- interpolation + compaction -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uv_flag_kernel(const int* __restrict__ tri_id, int n, int64_t nt, int* __restrict__ flag) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    flag[p] = p < n && tri_id[p] >= 0 && tri_id[p] < nt ? 1 : 0;
}

__global__ void uv_count_kernel(const int* __restrict__ rank, int n, TxHeader* __restrict__ hdr) {
    if (threadIdx.x == 0) hdr->count = rank[n];
}

// (e0 a0 + e1 a1 + e2 a2) / a in float64, one rounding to fp32; no contraction, so that numpy restates it bit for bit
__device__ __forceinline__ float uv_blend(double e0, double e1, double e2, double a, float a0, float a1, float a2) {
#pragma clang fp contract(off)
    return (float)((e0 * (double)a0 + e1 * (double)a1 + e2 * (double)a2) / a);
}

__global__ __launch_bounds__(256) void uv_interp_kernel(const int* __restrict__ tri_id, const int* __restrict__ flag, const int* __restrict__ rank,
                                                        const float* __restrict__ vt, int64_t nvt, const int* __restrict__ ft, int64_t nt,
                                                        const float* __restrict__ attr, int64_t nv, int C, const int* __restrict__ fa, int h,
                                                        int w, int* __restrict__ texel, float* __restrict__ out, int64_t cap,
                                                        unsigned char* __restrict__ mask, int64_t* __restrict__ n_out) {
    const int n = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && n_out) *n_out = rank[n];
    if (p >= n) return;
    const int f = flag[p];
    if (mask) mask[p] = (unsigned char)f;
    if (!f) return;
    const int64_t o = rank[p];
    if (o >= cap) return;
    texel[o] = p;
    const int64_t t = tri_id[p];
    UvTri s;
    int64_t e[3] = {0, 0, 0};
    bool ok = uv_setup(vt, nvt, ft, t, h, w, s);
    if (ok) (void)uv_inside(s, p % w, p / w, e);
    int64_t ia[3] = {0, 0, 0};
    if (ok) {
        ia[0] = fa[3 * t];
        ia[1] = fa[3 * t + (s.swapped ? 2 : 1)];
        ia[2] = fa[3 * t + (s.swapped ? 1 : 2)];
        ok = ia[0] >= 0 && ia[0] < nv && ia[1] >= 0 && ia[1] < nv && ia[2] >= 0 && ia[2] < nv;
    }
    float* dst = out + o * C;
    if (!ok) {                                        // an id that does not belong to this (vt, ft, fa): zeros, never a read out of range
        for (int c = 0; c < C; ++c) dst[c] = 0.0f;
        return;
    }
    const double e0 = (double)e[0], e1 = (double)e[1], e2 = (double)e[2], a = (double)s.a;
    for (int c = 0; c < C; ++c) dst[c] = uv_blend(e0, e1, e2, a, attr[ia[0] * C + c], attr[ia[1] * C + c], attr[ia[2] * C + c]);
}

// ---- quantisation ---------------------------------------------------------------------------------------------------------------------------
// utils/raw_utils.py:11-15 on a value clamped to [0, 1] (NaN -> 0), then * 255 truncated toward zero -- in float64, as the reference's numpy
// branch computes it (feats is a float64 array there), so that a level only differs from numpy's where the two pow() differ in the last bit
__device__ __forceinline__ unsigned char tx_quant(float xf) {
    const double x = xf > 0.0f ? (xf < 1.0f ? (double)xf : 1.0) : 0.0;
    const double s = x <= 0.0031308 ? (323.0 / 25.0) * x : (211.0 * pow(fmax(x, (double)1.1920929e-07f), 5.0 / 12.0) - 11.0) / 200.0;
    const int q = (int)(s * 255.0);
    return (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

__global__ __launch_bounds__(256) void tx_quantize_kernel(const float* __restrict__ feat, const int* __restrict__ texel, int64_t n, int C,
                                                          int64_t n_tex, unsigned char* __restrict__ tex) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * C) return;
    const int64_t r = i / C;
    const int c = (int)(i - r * C);
    const int64_t p = texel[r];
    if (p < 0 || p >= n_tex) return;
    tex[p * C + c] = tx_quant(feat[i]);
}

// ---- regions: separable clamped city-block distances ---------------------------------------------------------------------------------------
// Row pass, one byte per texel: a covered texel stores 0x80 | (distance to the nearest uncovered texel of its row, the image edge counting
// as uncovered, clamped to border + 1); an uncovered texel the distance to the nearest covered texel of its row, clamped to pad + 1.
constexpr int REG_SEG = 256;
__global__ __launch_bounds__(REG_SEG) void tx_region_row_kernel(const unsigned char* __restrict__ mask, int h, int w, int pad, int border,
                                                                unsigned char* __restrict__ d) {
    __shared__ unsigned char row[REG_SEG + 2 * (TX_MAX_PAD + 1)];
    const int halo = (pad > border ? pad : border) + 1;
    const int y = blockIdx.y, x0 = blockIdx.x * REG_SEG;
    for (int i = threadIdx.x; i < REG_SEG + 2 * halo; i += REG_SEG) {
        const int x = x0 - halo + i;
        row[i] = (x >= 0 && x < w) ? (mask[(int64_t)y * w + x] ? 1 : 0) : 2;       // 2: outside the image
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    const unsigned char* c = row + halo + threadIdx.x;
    int k = 1;
    unsigned char v;
    if (c[0] == 1) {
        while (k <= border && c[-k] == 1 && c[k] == 1) ++k;
        v = (unsigned char)(0x80 | k);
    } else {
        while (k <= pad && c[-k] != 1 && c[k] != 1) ++k;
        v = (unsigned char)k;
    }
    d[(int64_t)y * w + x] = v;
}

// Column pass: city-block distance = min over rows of |dy| + the row distance; region codes 0 nothing, 1 interior, 2 search band, 3 fill
__global__ __launch_bounds__(256) void tx_region_col_kernel(const unsigned char* __restrict__ d, int h, int w, int pad, int border,
                                                            unsigned char* __restrict__ region) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const unsigned char* col = d + x;
    const int own = col[(int64_t)y * w];
    unsigned char r;
    if (own & 0x80) {
        int best = own & 0x7f;
        best = min(best, min(y + 1, h - y));                  // the rows outside the image are uncovered
        for (int k = 1; k <= border && k < best; ++k) {
            if (y - k >= 0) { const int v = col[(int64_t)(y - k) * w]; best = min(best, k + ((v & 0x80) ? (v & 0x7f) : 0)); }
            if (y + k < h) { const int v = col[(int64_t)(y + k) * w]; best = min(best, k + ((v & 0x80) ? (v & 0x7f) : 0)); }
        }
        r = best <= border ? 2 : 1;
    } else {
        int best = own;
        for (int k = 1; k <= pad && k < best; ++k) {
            if (y - k >= 0) { const int v = col[(int64_t)(y - k) * w]; best = min(best, k + ((v & 0x80) ? 0 : v)); }
            if (y + k < h) { const int v = col[(int64_t)(y + k) * w]; best = min(best, k + ((v & 0x80) ? 0 : v)); }
        }
        r = best <= pad ? 3 : 0;
    }
    region[(int64_t)y * w + x] = r;
}

// ---- gutter fill ------------------------------------------------------------------------------------------------------------------------------
// One workgroup per FILL_TILE^2 output tile; the region bytes of a tile that holds a fill texel, plus a halo of `pad` texels, live in LDS.
// A fill texel visits the rows of its window by growing |dy| and each row by growing |dx|, and stops as soon as no remaining texel can beat (or tie) the best key
// (squared distance, row-major index) -- the minimum over the whole (2 pad + 1)^2 window, at a fraction of its reads.
// Measured (icosphere atlas, 4096^2): the time grows with the window area, 0.13 / 0.58 / 1.9 / 4.1 ms at pad 4 / 16 / 32 / 64, and is the same
// for 1 and 5 channels; a map without fill texels takes 0.035 ms.
__global__ __launch_bounds__(FILL_TILE* FILL_TILE) void tx_fill_kernel(unsigned char* __restrict__ tex, const unsigned char* __restrict__ region,
                                                                        int h, int w, int C, int pad, int* __restrict__ src) {
    extern __shared__ unsigned char win[];
    const int side = FILL_TILE + 2 * pad;
    const int tx0 = blockIdx.x * FILL_TILE, ty0 = blockIdx.y * FILL_TILE;
    {   // a tile without a fill texel skips the window: its own 256 bytes decide
        const int ox = tx0 + (threadIdx.x & (FILL_TILE - 1)), oy = ty0 + threadIdx.x / FILL_TILE;
        const bool in = ox < w && oy < h;
        const bool wants = in && region[(int64_t)oy * w + ox] == 3;
        if (!__syncthreads_or(wants)) {
            if (src && in) src[(int64_t)oy * w + ox] = -1;
            return;
        }
    }
    unsigned char* row_has = win + side * side;                // per window row: it holds a search texel at all
    if ((int)threadIdx.x < side) row_has[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < side * side; i += FILL_TILE * FILL_TILE) {
        const int wy = i / side, wx = i - wy * side;
        const int gx = tx0 - pad + wx, gy = ty0 - pad + wy;
        const unsigned char v = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? region[(int64_t)gy * w + gx] : 0;
        win[i] = v;
        if (v == 2) row_has[wy] = 1;                           // (every writer stores the same value)
    }
    __syncthreads();
    const int lx = threadIdx.x & (FILL_TILE - 1), ly = threadIdx.x / FILL_TILE;
    const int x = tx0 + lx, y = ty0 + ly;
    if (x >= w || y >= h) return;
    const int64_t p = (int64_t)y * w + x;
    const unsigned char* c = win + (ly + pad) * side + (lx + pad);
    if (c[0] != 3) {
        if (src) src[p] = -1;
        return;
    }
    const int64_t none = INT64_MAX;
    int64_t best = none;                                       // d2 << 32 | row-major index of the source
    int best_d2 = 2 * pad * pad;                               // the window's corner: every texel of the window qualifies
    for (int ady = 0; ady <= pad && ady * ady <= best_d2; ++ady) {
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            if (ady == 0 && sgn > 0) continue;
            const int dy = sgn * ady;
            if (!row_has[ly + pad + dy]) continue;             // far from every chart the near rows are empty: one read instead of a row scan
            const unsigned char* rowp = c + dy * side;
            for (int adx = 0; adx <= pad && adx * adx + ady * ady <= best_d2; ++adx) {
                const bool l = rowp[-adx] == 2, r = rowp[adx] == 2;
                if (l || r) {
                    const int d2 = adx * adx + ady * ady;
                    const int64_t key = ((int64_t)d2 << 32) | (int64_t)((int64_t)(y + dy) * w + (l ? x - adx : x + adx));
                    if (key < best) { best = key; best_d2 = d2; }
                    break;                                     // farther texels of this row are strictly worse
                }
            }
        }
    }
    if (best == none) {                                        // an inconsistent region map: leave the texel
        if (src) src[p] = -1;
        return;
    }
    const int64_t q = best & 0xffffffffll;
    if (src) src[p] = (int)q;
    for (int k = 0; k < C; ++k) tex[p * C + k] = tex[q * C + k];
}

__global__ __launch_bounds__(256) void tx_down2_kernel(const unsigned char* __restrict__ in, int h, int w, int C, unsigned char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)h * w * C) return;
    const int c = (int)(i % C);
    const int64_t px = i / C;
    const int x = (int)(px % w), y = (int)(px / w);
    const int64_t rs = (int64_t)2 * w * C;
    const unsigned char* s = in + (int64_t)(2 * y) * rs + (int64_t)(2 * x) * C + c;
    out[i] = (unsigned char)(((int)s[0] + (int)s[C] + (int)s[rs] + (int)s[rs + C] + 2) >> 2);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------------
bool size_ok(int h, int w) { return h >= 1 && h <= TX_MAX_SIZE && w >= 1 && w <= TX_MAX_SIZE; }
bool count_ok(int64_t n) { return n >= 0 && n < ((int64_t)1 << 31) - 1; }

int check_size(const char* fn, int h, int w) {
    if (size_ok(h, w)) return NERO_OK;
    static thread_local char msg[160];
    snprintf(msg, sizeof(msg), "%s: map of %d x %d texels: both sizes must be in [1, %d]", fn, h, w, TX_MAX_SIZE);
    return nero_fail(NERO_ERR_ARG, msg);
}

struct RasterLayout {
    size_t cnt, base, temp, temp_bytes, total;
};

int raster_layout(int64_t nt, RasterLayout* L) {
    if (scan_temp<int64_t>(nt + 1, &L->temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_uv_raster: the scratch-size query of the block scan failed");
    Carve c{256};                                                 // TxHeader
    L->cnt = c.take((size_t)(nt + 1) * sizeof(int64_t));
    L->base = c.take((size_t)(nt + 1) * sizeof(int64_t));
    L->temp = c.take(L->temp_bytes);
    L->total = c.at;
    return NERO_OK;
}

struct InterpLayout {
    size_t flag, rank, temp, temp_bytes, total;
};

int interp_layout(int64_t n, InterpLayout* L) {
    if (scan_temp<int>(n + 1, &L->temp_bytes) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_uv_interp: the scratch-size query of the scan of the coverage failed");
    Carve c{256};                                                 // TxHeader
    L->flag = c.take((size_t)(n + 1) * sizeof(int));
    L->rank = c.take((size_t)(n + 1) * sizeof(int));
    L->temp = c.take(L->temp_bytes);
    L->total = c.at;
    return NERO_OK;
}

}  // namespace

size_t nero_uv_raster_workspace_bytes(int64_t nt) {
    RasterLayout L;
    if (!count_ok(nt)) return no_workspace("nero_uv_raster_workspace_bytes: nt must be in [0, 2^31 - 1)");
    return raster_layout(nt, &L) == NERO_OK ? L.total : 0;
}

int nero_uv_raster(const float* vt, int64_t nvt, const int* ft, int64_t nt, int h, int w, void* ws, int* tri_id, void* stream) {
    if (int rc = check_size("nero_uv_raster", h, w)) return rc;
    if (!count_ok(nt) || !count_ok(nvt)) return nero_fail(NERO_ERR_ARG, "nero_uv_raster: a count is negative or 2^31 - 1 or more");
    if (!tri_id || !ws || (nt > 0 && (!ft || (nvt > 0 && !vt)))) return nero_fail(NERO_ERR_ARG, "nero_uv_raster: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    const int64_t n = (int64_t)h * w;
    if (nt > 0) {                                                 // refuse a face index outside [0, nvt) before anything is written
        if (hipMemsetAsync(b, 0, 256, s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_uv_raster: hipMemsetAsync failed");
        hipLaunchKernelGGL(tx_index_check_kernel, dim3(blocks_of(3 * nt)), dim3(256), 0, s, ft, 3 * nt, nvt, (TxHeader*)b);
        if (int rc = nero_check_launch("nero_uv_raster: index check")) return rc;
        TxHeader host{};
        if (int rc = read_back(&host, ws, sizeof(host), s, "nero_uv_raster: reading the index check back failed")) return rc;
        if (host.bad) return nero_fail(NERO_ERR_ARG, "nero_uv_raster: ft holds an index outside [0, nvt)");
    }
    if (hipMemsetAsync(tri_id, 0xff, (size_t)n * sizeof(int), s) != hipSuccess)        // -1 = 0xffffffff: the identity of the unsigned minimum
        return nero_fail(NERO_ERR_LAUNCH, "nero_uv_raster: hipMemsetAsync failed");
    if (nt == 0) return NERO_OK;
    RasterLayout L;
    if (int rc = raster_layout(nt, &L)) return rc;
    int64_t* cnt = (int64_t*)(b + L.cnt);
    int64_t* base = (int64_t*)(b + L.base);
    hipLaunchKernelGGL(uv_small_kernel<false>, dim3(blocks_of(nt + 1)), dim3(256), 0, s, vt, nvt, ft, nt, h, w, (unsigned*)tri_id, cnt);
    if (int rc = nero_check_launch("nero_uv_raster: small-triangle pass")) return rc;
    if (int rc = exclusive_sum(b + L.temp, L.temp_bytes, (const int64_t*)cnt, base, nt + 1, s, "nero_uv_raster: block scan failed")) return rc;
    hipLaunchKernelGGL(uv_walk_kernel<false>, dim3(UV_WALK_BLOCKS), dim3(256), 0, s, vt, nvt, ft, nt, h, w, (const int64_t*)base, (unsigned*)tri_id);
    return nero_check_launch("nero_uv_raster: block walk");
}

size_t nero_uv_overlap_count_workspace_bytes(int64_t nt, int h, int w) {
    RasterLayout L;
    if (!count_ok(nt)) return no_workspace("nero_uv_overlap_count_workspace_bytes: nt must be in [0, 2^31 - 1)");
    if (check_size("nero_uv_overlap_count_workspace_bytes", h, w) || raster_layout(nt, &L) != NERO_OK) return 0;
    return L.total + align256((size_t)h * w * sizeof(unsigned));
}

int nero_uv_overlap_count(const float* vt, int64_t nvt, const int* ft, int64_t nt, int h, int w, void* ws, int64_t* count, void* stream) {
    if (int rc = check_size("nero_uv_overlap_count", h, w)) return rc;
    if (!count_ok(nt) || !count_ok(nvt)) return nero_fail(NERO_ERR_ARG, "nero_uv_overlap_count: a count is negative or 2^31 - 1 or more");
    if (!count || !ws || (nt > 0 && (!ft || (nvt > 0 && !vt)))) return nero_fail(NERO_ERR_ARG, "nero_uv_overlap_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(count, 0, sizeof(int64_t), s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_uv_overlap_count: hipMemsetAsync failed");
    if (nt == 0) return NERO_OK;
    uint8_t* b = (uint8_t*)ws;
    const int64_t n = (int64_t)h * w;
    RasterLayout L;
    if (int rc = raster_layout(nt, &L)) return rc;
    int64_t* cnt = (int64_t*)(b + L.cnt);
    int64_t* base = (int64_t*)(b + L.base);
    unsigned* cover = (unsigned*)(b + L.total);
    if (hipMemsetAsync(cover, 0, (size_t)n * sizeof(unsigned), s) != hipSuccess)
        return nero_fail(NERO_ERR_LAUNCH, "nero_uv_overlap_count: hipMemsetAsync failed");
    hipLaunchKernelGGL(uv_small_kernel<true>, dim3(blocks_of(nt + 1)), dim3(256), 0, s, vt, nvt, ft, nt, h, w, cover, cnt);
    if (int rc = nero_check_launch("nero_uv_overlap_count: small-triangle pass")) return rc;
    if (int rc = exclusive_sum(b + L.temp, L.temp_bytes, (const int64_t*)cnt, base, nt + 1, s, "nero_uv_overlap_count: block scan failed")) return rc;
    hipLaunchKernelGGL(uv_walk_kernel<true>, dim3(UV_WALK_BLOCKS), dim3(256), 0, s, vt, nvt, ft, nt, h, w, (const int64_t*)base, cover);
    if (int rc = nero_check_launch("nero_uv_overlap_count: block walk")) return rc;
    hipLaunchKernelGGL(uv_overlap_sum_kernel, dim3(blocks_of(n)), dim3(256), 0, s, (const unsigned*)cover, n, (unsigned long long*)count);
    return nero_check_launch("nero_uv_overlap_count: sum");
}

size_t nero_uv_interp_workspace_bytes(int h, int w) {
    InterpLayout L;
    if (check_size("nero_uv_interp_workspace_bytes", h, w)) return 0;
    return interp_layout((int64_t)h * w, &L) == NERO_OK ? L.total : 0;
}

int nero_uv_interp(const int* tri_id, const float* vt, int64_t nvt, const int* ft, int64_t nt, const float* attr, int64_t nv, int C, const int* fa,
                   int h, int w, void* ws, int* texel, float* out, int64_t cap, unsigned char* mask, int64_t* n_out, void* stream) {
    if (int rc = check_size("nero_uv_interp", h, w)) return rc;
    if (!count_ok(nt) || !count_ok(nvt) || !count_ok(nv) || C < 1 || cap < 0)
        return nero_fail(NERO_ERR_ARG, "nero_uv_interp: a count is negative or 2^31 - 1 or more, C < 1 or cap < 0");
    if (!tri_id || !ws || (nt > 0 && (!ft || !fa || !vt || !attr))) return nero_fail(NERO_ERR_ARG, "nero_uv_interp: null pointer");
    hipStream_t s = (hipStream_t)stream;
    uint8_t* b = (uint8_t*)ws;
    const int n = h * w;
    InterpLayout L;
    if (int rc = interp_layout(n, &L)) return rc;
    int* flag = (int*)(b + L.flag);
    int* rank = (int*)(b + L.rank);
    if (hipMemsetAsync(b, 0, 256, s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_uv_interp: hipMemsetAsync failed");
    if (nt > 0) {
        hipLaunchKernelGGL(tx_index_check_kernel, dim3(blocks_of(3 * nt)), dim3(256), 0, s, ft, 3 * nt, nvt, (TxHeader*)b);
        hipLaunchKernelGGL(tx_index_check_kernel, dim3(blocks_of(3 * nt)), dim3(256), 0, s, fa, 3 * nt, nv, (TxHeader*)b);
    }
    hipLaunchKernelGGL(uv_flag_kernel, dim3(blocks_of((int64_t)n + 1)), dim3(256), 0, s, tri_id, n, nt, flag);
    if (int rc = nero_check_launch("nero_uv_interp: flags")) return rc;
    if (int rc = exclusive_sum(b + L.temp, L.temp_bytes, (const int*)flag, rank, n + 1, s, "nero_uv_interp: the scan of the coverage failed")) return rc;
    hipLaunchKernelGGL(uv_count_kernel, dim3(1), dim3(64), 0, s, (const int*)rank, n, (TxHeader*)b);
    if (int rc = nero_check_launch("nero_uv_interp: count")) return rc;
    TxHeader host{};
    if (int rc = read_back(&host, ws, sizeof(host), s, "nero_uv_interp: reading the count back failed")) return rc;
    if (host.bad) return nero_fail(NERO_ERR_ARG, "nero_uv_interp: ft or fa holds an index out of range");
    if (host.count > cap) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_uv_interp: %lld covered texels exceed the capacity %lld", (long long)host.count, (long long)cap);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (host.count > 0 && (!texel || !out)) return nero_fail(NERO_ERR_ARG, "nero_uv_interp: null output pointer");
    hipLaunchKernelGGL(uv_interp_kernel, dim3(blocks_of(n)), dim3(256), 0, s, tri_id, (const int*)flag, (const int*)rank, vt, nvt, ft, nt, attr, nv, C,
                       fa, h, w, texel, out, cap, mask, n_out);
    return nero_check_launch("nero_uv_interp");
}

int nero_tex_quantize(const float* feat, const int* texel, int64_t n, int C, int h, int w, unsigned char* tex, void* stream) {
    if (int rc = check_size("nero_tex_quantize", h, w)) return rc;
    if (n < 0 || n > (int64_t)h * w || C < 1 || C > 64) return nero_fail(NERO_ERR_ARG, "nero_tex_quantize: n outside [0, h w] or C outside [1, 64]");
    if (!tex || (n > 0 && (!feat || !texel))) return nero_fail(NERO_ERR_ARG, "nero_tex_quantize: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(tex, 0, (size_t)h * w * C, s) != hipSuccess) return nero_fail(NERO_ERR_LAUNCH, "nero_tex_quantize: hipMemsetAsync failed");
    if (n == 0) return NERO_OK;
    hipLaunchKernelGGL(tx_quantize_kernel, dim3(blocks_of(n * C)), dim3(256), 0, s, feat, texel, n, C, (int64_t)h * w, tex);
    return nero_check_launch("nero_tex_quantize");
}

size_t nero_tex_regions_workspace_bytes(int h, int w) { return size_ok(h, w) ? align256((size_t)h * w) : 0; }

int nero_tex_regions(const unsigned char* mask, int h, int w, int pad, int border, void* ws, unsigned char* region, void* stream) {
    if (int rc = check_size("nero_tex_regions", h, w)) return rc;
    if (pad < 0 || pad > TX_MAX_PAD || border < 1 || border > TX_MAX_BORDER) {
        static thread_local char msg[160];
        snprintf(msg, sizeof(msg), "nero_tex_regions: pad %d outside [0, %d] or border %d outside [1, %d]", pad, TX_MAX_PAD, border, TX_MAX_BORDER);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    if (!mask || !ws || !region) return nero_fail(NERO_ERR_ARG, "nero_tex_regions: null pointer");
    hipStream_t s = (hipStream_t)stream;
    unsigned char* d = (unsigned char*)ws;
    hipLaunchKernelGGL(tx_region_row_kernel, dim3((unsigned)((w + REG_SEG - 1) / REG_SEG), (unsigned)h), dim3(REG_SEG), 0, s, mask, h, w, pad, border, d);
    if (int rc = nero_check_launch("nero_tex_regions: row pass")) return rc;
    hipLaunchKernelGGL(tx_region_col_kernel, dim3((unsigned)((w + 63) / 64), (unsigned)((h + 3) / 4)), dim3(256), 0, s, (const unsigned char*)d, h, w, pad,
                       border, region);
    return nero_check_launch("nero_tex_regions: column pass");
}

int nero_tex_fill(unsigned char* tex, const unsigned char* region, int h, int w, int C, int pad, int* src, void* stream) {
    if (int rc = check_size("nero_tex_fill", h, w)) return rc;
    if (pad < 0 || pad > TX_MAX_PAD || C < 1 || C > 64) return nero_fail(NERO_ERR_ARG, "nero_tex_fill: pad outside [0, 64] or C outside [1, 64]");
    if (!tex || !region) return nero_fail(NERO_ERR_ARG, "nero_tex_fill: null pointer");
    const int side = FILL_TILE + 2 * pad;
    hipLaunchKernelGGL(tx_fill_kernel, dim3((unsigned)((w + FILL_TILE - 1) / FILL_TILE), (unsigned)((h + FILL_TILE - 1) / FILL_TILE)),
                       dim3(FILL_TILE * FILL_TILE), (size_t)side * side + side, (hipStream_t)stream, tex, region, h, w, C, pad, src);
    return nero_check_launch("nero_tex_fill");
}

int nero_tex_downsample2(const unsigned char* in, int h, int w, int C, unsigned char* out, void* stream) {
    if (int rc = check_size("nero_tex_downsample2", h, w)) return rc;
    if (2 * h > TX_MAX_SIZE || 2 * w > TX_MAX_SIZE || C < 1 || C > 64)
        return nero_fail(NERO_ERR_ARG, "nero_tex_downsample2: the input map exceeds 16384 texels on a side or C is outside [1, 64]");
    if (!in || !out) return nero_fail(NERO_ERR_ARG, "nero_tex_downsample2: null pointer");
    hipLaunchKernelGGL(tx_down2_kernel, dim3(blocks_of((int64_t)h * w * C)), dim3(256), 0, (hipStream_t)stream, in, h, w, C, out);
    return nero_check_launch("nero_tex_downsample2");
}
