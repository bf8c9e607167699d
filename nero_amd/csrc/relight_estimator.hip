// relight_estimator.hip -- the relighter's estimator: the four fused entry points nero_bvh_relight (include/nero_hip_relight.h),
// nero_bvh_relight_mis (include/nero_hip_envsample.h), nero_bvh_relight_bounce and nero_bvh_relight_mis_bounce, and the bounce's ray
// export nero_relight_bounce_rays (include/nero_hip_bounce.h); DESIGN.md 9.12 - 9.12.2.
//   relight_kernel<MIS, BOUNCE, OVERLAP, RAYS>   ONE template.  A lane forms its sample's ray (relight_ray of relight_dev.h, or mis_ray of
//                                       envsample_dev.h with MIS), walks it on the stack OVERLAP selects, looks the map up and weighs the
//                                       radiance by the estimator of shade_mixed, field.py:950-998 (two_strategy_terms, or the
//                                       balance-heuristic mixture mis_terms with MIS); the rays are never stored.
//     BOUNCE off: the ray is a shadow ray (any hit within the miss distance), and a sample that meets the mesh is black.
//     BOUNCE on:  that ray is walked as a closest hit, the surface at the hit y is rebuilt from the caller's mesh (face through Bvh::d_face,
//                 (u, v) by hit_bary, materials and normal interpolated, the record terms of nero_mc_point_setup), y draws ONE sample of its
//                 own direct lighting from the mixture of the primary's strategies -- its variates a counter hash of (point key, sample
//                 index), so a lane's bounce does not depend on the chunking -- walks that sample's shadow ray as an any hit on the same
//                 stack, and hands L_o(y, -w) to the primary estimator in the place of the map's radiance.
//     RAYS (with BOUNCE): write what the lane decides (nero_relight_bounce_rays) instead of tracing the secondary and reducing.
//   finish_kernel<BOUNCE>               a point's partials added in index order, and the means.
// The reduction has a fixed order: shuffle butterfly inside the wavefront, one partial per wavefront (six floats, twelve with BOUNCE), the
// finishing pass.  No float atomics; every store is an ordinary vector store.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/nero_hip.h"
#include "../../include/nero_hip_relight.h"
#include "../../include/nero_hip_envsample.h"
#include "../../include/nero_hip_bounce.h"
#include "bvh_types.h"
#include "bvh_walk.h"
#include "common.h"
#include "relight_plan.h"
#include "relight_dev.h"
#include "envsample_dev.h"

namespace {

using namespace nero_bvh;
using nero_relight::EnvMap; using nero_relight::env_sample; using nero_relight::relight_ray; using nero_relight::dotp;
using nero_relight::two_strategy_terms; using nero_relight::hit_bary; using nero_relight::check_env; using nero_relight::check_samples;
using nero_relight::MISS_DEPTH; using nero_relight::PRIV_THREADS; using nero_relight::with_walk;
using nero_relight::PARTIAL_DIRECT; using nero_relight::PARTIAL_BOUNCE; using nero_relight::grid_blocks;
using nero_relight::samples_ok; using nero_relight::mis_samples_ok; using nero_relight::total_ok; using nero_relight::total_lanes;
using nero_relight::waves_per_point; using nero_relight::workspace_bytes;
using nero_envsample::LightTab; using nero_envsample::u64; using nero_envsample::mis_ray; using nero_envsample::mis_terms;
using nero_envsample::env_draw; using nero_envsample::env_lookup_cell; using nero_envsample::check_mis_samples;
using nero_envsample::check_table_size; using nero_envsample::map_ok;
using nero_shade::sat;

enum : int { FREE = 0, DEAD = 1, BOUNCED = 2, BOUNCED_DEAD = 3, BAD_FACE = 4 };        // nero_hip_bounce.h, nero_relight_bounce_rays: state

struct Samples {                           // what the primary estimator takes (tab_l .. info, gh, gw: MIS only; key: BOUNCE only)
    const float *pt, *tab_d, *tab_s, *tab_l, *rand_l;
    const unsigned* key;
    const int64_t *cdf, *info;
    int P, Dd, Ds, Dl, wpp, geom, gh, gw;
};
struct Mesh { const float* verts; const int* tris; const float* mat5; const float* normals; const int* face_of; int V, T; };
struct RayOut { unsigned char* state; int* face; float* bary; float* sec_o; float* sec_d; int* strategy; float* pdf_l; int* cell; };
struct Absent {};                          // the Mesh and the RayOut of a kernel without BOUNCE
template <bool BOUNCE, class T> using If = std::conditional_t<BOUNCE, T, Absent>;

// ---- the surface at y -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void norm3(const float* a, float* o) {
#pragma clang fp contract(off)
    const float n = fmaxf(sqrtf(dotp(a, a)), 1e-12f);
    o[0] = a[0] / n; o[1] = a[1] / n; o[2] = a[2] / n;
}
// get_orthogonal_directions (ortho3 of mc_shade.hip), the candidate chosen component by component: no pointer to a local array is selected
__device__ __forceinline__ void ortho3(const float* d, float* o) {
#pragma clang fp contract(off)
    const float o0[3] = {d[1], -d[0], 0.f}, o1[3] = {-d[2], 0.f, d[0]};
    const bool m0 = sqrtf(dotp(o0, o0)) > sqrtf(dotp(o1, o1));
    const float pick[3] = {m0 ? o0[0] : o1[0], m0 ? o0[1] : o1[1], m0 ? o0[2] : o1[2]};
    norm3(pick, o);
}
__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
#pragma clang fp contract(off)
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// The point record of y = the hit of direction w on `face` at (u, v), in the layout of nero_mc_point_setup (every index below is a
// compile-time constant: the record lives in registers).  false: the face names a vertex outside [0, V) -- nothing of the mesh is read.
__device__ __forceinline__ bool surface_record(const Mesh& M, int face, float u, float v, const float* w, float* rec) {
#pragma clang fp contract(off)
    if (face < 0 || face >= M.T) return false;
    const int i0 = M.tris[(size_t)face * 3], i1 = M.tris[(size_t)face * 3 + 1], i2 = M.tris[(size_t)face * 3 + 2];
    if (i0 < 0 || i0 >= M.V || i1 < 0 || i1 >= M.V || i2 < 0 || i2 >= M.V) return false;
    const float w0 = 1.0f - u - v;
    float V0[3], V1[3], V2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        V0[c] = M.verts[(size_t)i0 * 3 + c]; V1[c] = M.verts[(size_t)i1 * 3 + c]; V2[c] = M.verts[(size_t)i2 * 3 + c];
        rec[29 + c] = (w0 * V0[c] + u * V1[c]) + v * V2[c];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
        rec[9 + k] = (w0 * M.mat5[(size_t)i0 * 5 + k] + u * M.mat5[(size_t)i1 * 5 + k]) + v * M.mat5[(size_t)i2 * 5 + k];
    rec[10] = rec[10] * rec[10];                                       // perceptual roughness -> alpha, once
    float g[3];
    if (M.normals) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            g[c] = (w0 * M.normals[(size_t)i0 * 3 + c] + u * M.normals[(size_t)i1 * 3 + c]) + v * M.normals[(size_t)i2 * 3 + c];
    } else {
        const float e1[3] = {V1[0] - V0[0], V1[1] - V0[1], V1[2] - V0[2]}, e2[3] = {V2[0] - V0[0], V2[1] - V0[1], V2[2] - V0[2]};
        cross3(e1, e2, g);
        if (dotp(g, w) > 0.f) { g[0] = -g[0]; g[1] = -g[1]; g[2] = -g[2]; }     // the side the ray came from
    }
    float n1[3], n[3], vw[3];
    norm3(g, n1);
    norm3(n1, n);                                                      // (Relighter.surface normalises, nero_mc_point_setup again)
    const float neg[3] = {-w[0], -w[1], -w[2]};
    norm3(neg, vw);
    const float nv = dotp(vw, n);
    float refl[3], x[3], y[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { rec[c] = vw[c]; rec[3 + c] = n[c]; refl[c] = nv * n[c] * 2.f - vw[c]; rec[6 + c] = refl[c]; }
    rec[14] = sat(nv);
    ortho3(n, x); cross3(n, x, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) { rec[15 + c] = x[c]; rec[18 + c] = y[c]; }
    ortho3(refl, x); cross3(refl, x, y);
#pragma unroll
    for (int c = 0; c < 3; ++c) { rec[21 + c] = x[c]; rec[24 + c] = y[c]; }
    rec[27] = -1.f; rec[28] = -1.f;                                    // no azimuth rotation: the variates are the point's own already
    return true;
}

// ---- the secondary sample ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lowbias32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// The one sample of the record `rec` for lane j of a point with `key` (header, THE SECONDARY SAMPLE) -> the strategy; w2, o2, dead2, and p_l
// of w2 with its cell (0 and -1 without a table)
template <bool MIS>
__device__ __forceinline__ int secondary_sample(const float* rec, unsigned key, int j, int Dd, int Ds, int Dl, int geom, const LightTab& T,
                                                float* w2, float* o2, bool& dead2, float& pl2, int& cell) {
#pragma clang fp contract(off)
    const unsigned k1 = lowbias32(key + (unsigned)j * 0x9E3779B9u), k2 = lowbias32(k1 + 0x68E31DA4u), k3 = lowbias32(k2 + 0x68E31DA4u);
    const float u1 = (float)(k1 >> 8) * 0x1p-24f;
    const float tab[2] = {(float)(k2 >> 8) * 0x1p-24f, (float)(k3 >> 8) * 0x1p-24f};
    const float D = (float)(Dd + Ds + Dl);
    const float cd = (float)Dd / D, cs = (float)Ds / D;
    const int s = u1 < cd ? 0 : ((!MIS || u1 < cd + cs) ? 1 : 2);
    pl2 = 0.f;
    cell = -1;
    if (s < 2) {
        dead2 = relight_ray(rec, tab, tab, 0, s == 0 ? 1 : 0, geom, w2, o2);         // sample 0 of a one-row table: cosine (Dd = 1) or GGX (Dd = 0)
        if constexpr (MIS) env_lookup_cell(T, w2, cell, pl2);
    } else {
        env_draw(T, tab[0], tab[1], w2, cell, pl2);
#pragma unroll
        for (int c = 0; c < 3; ++c) o2[c] = rec[29 + c] + w2[c] * 1e-5f;
        dead2 = geom == 0 && dotp(rec + 3, w2) < -1e-6f;
    }
    return s;
}

// L_o(y, -w) from the one sample w2 that fetched Le: both terms of the mixture estimator, capped per channel when the map is
__device__ __forceinline__ void bounce_radiance(const float* rec, const float* w2, float pl2, int Dd, int Ds, int Dl, int geom, const float* Le,
                                                float clamp_max, float* L) {
#pragma clang fp contract(off)
    float df[3], sp[3];
    mis_terms(rec, w2, pl2, Dd, Ds, Dl, geom, Le, df, sp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        L[c] = df[c] + sp[c];
        if (clamp_max > 0.f) L[c] = fminf(L[c], clamp_max);
    }
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------------------
// One lane per (point, sample): wavefront W of the grid is chunk W % wpp of point W / wpp, lane l its sample (W % wpp) 64 + l; samples at or
// past D are padding.  partial [P wpp, 6]: the wavefront's sums of the diffuse and the specular terms, added by a shuffle butterfly (the
// same order on every run); with BOUNCE [P wpp, 12], the sums of the indirect diffuse and indirect specular terms behind them.  With BOUNCE
// a lane whose primary ray is free never walks a second time: it waits for the bounced lanes of its wavefront.
// OVERLAP: PL_THREADS threads and the LDS stack (trees no deeper than PL_STACK), else PRIV_THREADS threads and the private stack
template <bool MIS, bool BOUNCE, bool OVERLAP, bool RAYS>
__global__ __launch_bounds__(OVERLAP ? PL_THREADS : PRIV_THREADS) void relight_kernel(const Node* __restrict__ nodes, const Tri* __restrict__ tris,
                                                                                      int root, Samples S, If<BOUNCE, Mesh> M, EnvMap E,
                                                                                      float* __restrict__ partial, If<BOUNCE, RayOut> R) {
    static_assert(BOUNCE || !RAYS, "RAYS exports what a bounce decides");
    __shared__ int lds_stack[OVERLAP ? PL_STACK * PL_THREADS : 1];
    int* const st = lds_stack + (OVERLAP ? threadIdx.x : 0);
    (void)st;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;               // below 2^31 (relight_plan.h)
    const int wave = g >> 6, lane = threadIdx.x & 63;
    const int p = wave / S.wpp;
    if (p >= S.P) return;                                              // a whole wavefront of the last workgroup
    const int Dd = S.Dd, Ds = S.Ds, Dl = MIS ? S.Dl : 0, geom = S.geom;
    const int D = Dd + Ds + Dl;
    const int j = (wave - p * S.wpp) * 64 + lane;
    const float* q = S.pt + (size_t)p * 32;
    float dir_d[3] = {0.f, 0.f, 0.f}, dir_s[3] = {0.f, 0.f, 0.f}, ind_d[3] = {0.f, 0.f, 0.f}, ind_s[3] = {0.f, 0.f, 0.f};
    if (j < D) {
        // the table's grid is the map's (nero_hip_envsample.h: gh x gw = eh x ew); with BOUNCE the caller's gh, gw, which RAYS has without a map
        const LightTab T = {S.cdf, BOUNCE ? S.gh : E.h, BOUNCE ? S.gw : E.w, MIS ? (u64)S.info[0] : 0ull};
        float d[3], o[3], pl = 0.f;
        bool dead;
        if constexpr (MIS) {
            int cell;
            dead = mis_ray(q, S.tab_d, S.tab_s, S.tab_l, S.rand_l ? S.rand_l + (size_t)p * 2 : nullptr, j, Dd, Ds, geom, T, d, o, cell, pl);
        } else {
            dead = relight_ray(q, S.tab_d, S.tab_s, j, Dd, geom, d, o);
        }
        if constexpr (!BOUNCE) {                                       // a shadow ray: a blocked or dead sample adds nothing
            NERO_RELIGHT_ANY_HIT(blocked, MISS_DEPTH, dead ? NONE : root)
            if (!dead && !blocked) {
                float L[3];
                env_sample(E, d, L);
                if constexpr (MIS) mis_terms(q, d, pl, Dd, Ds, Dl, geom, L, dir_d, dir_s);
                else two_strategy_terms(q, d, j, Dd, Ds, geom, L, dir_d, dir_s);
            }
        } else {
            int slot;                                                     // the primary walk: closest hit within the miss distance
            {
                float inv[3];
                ray_inverse(d, inv);
                if constexpr (OVERLAP) {
                    NERO_WALK_OVERLAP(false, MISS_DEPTH, dead ? NONE : root)
                    slot = best;
                } else {
                    NERO_WALK_PRIVATE(false, MISS_DEPTH, dead ? NONE : root)
                    slot = best;
                }
            }
            int state = dead ? DEAD : FREE, face = -1, strat = -1, cell2 = -1;
            float bu = 0.f, bv = 0.f, pl2 = 0.f;
            float o2[3] = {0.f, 0.f, 0.f}, w2[3] = {0.f, 0.f, 0.f};
            float rec[32];
            if (slot >= 0) {
                hit_bary(tris, slot, o, d, bu, bv);
                face = M.face_of[slot];
                state = BAD_FACE;
                if (surface_record(M, face, bu, bv, d, rec)) {
                    bool dead2;
                    strat = secondary_sample<MIS>(rec, S.key ? S.key[p] : 0u, j, Dd, Ds, Dl, geom, T, w2, o2, dead2, pl2, cell2);
                    state = dead2 ? BOUNCED_DEAD : BOUNCED;
                }
            }
            if constexpr (RAYS) {
                const size_t row = (size_t)p * D + j;
                const bool sec = state == BOUNCED || state == BOUNCED_DEAD;
                if (R.state) R.state[row] = (unsigned char)state;
                if (R.face) R.face[row] = face;
                if (R.bary) { R.bary[row * 2] = bu; R.bary[row * 2 + 1] = bv; }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (R.sec_o) R.sec_o[row * 3 + c] = sec ? o2[c] : 0.f;
                    if (R.sec_d) R.sec_d[row * 3 + c] = sec ? w2[c] : 0.f;
                }
                if (R.strategy) R.strategy[row] = sec ? strat : -1;
                if (R.pdf_l) R.pdf_l[row] = sec ? pl2 : 0.f;
                if (R.cell) R.cell[row] = sec ? cell2 : -1;
            } else {
                bool blocked2;                                             // the secondary walk: any hit, on the same stack
                {
                    const float *o = o2, *d = w2;                          // (the names the walks expand over)
                    NERO_RELIGHT_ANY_HIT(hit2, MISS_DEPTH, state == BOUNCED ? root : NONE)
                    blocked2 = hit2;
                }
                float L[3];
                bool lit = false;
                if (state == FREE) {
                    env_sample(E, d, L);
                    lit = true;
                } else if (state == BOUNCED && !blocked2) {
                    float Le[3];
                    env_sample(E, w2, Le);
                    bounce_radiance(rec, w2, pl2, Dd, Ds, Dl, geom, Le, E.clamp_max, L);
                    lit = true;
                }
                if (lit) {
                    float df[3] = {0.f, 0.f, 0.f}, sp[3];
                    if constexpr (MIS) mis_terms(q, d, pl, Dd, Ds, Dl, geom, L, df, sp);
                    else two_strategy_terms(q, d, j, Dd, Ds, geom, L, df, sp);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        if (state == FREE) { dir_d[c] = df[c]; dir_s[c] = sp[c]; }
                        else { ind_d[c] = df[c]; ind_s[c] = sp[c]; }
                    }
                }
            }
        }
    }
    if constexpr (!RAYS) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                dir_d[c] += __shfl_xor(dir_d[c], off);
                dir_s[c] += __shfl_xor(dir_s[c], off);
                if constexpr (BOUNCE) {
                    ind_d[c] += __shfl_xor(ind_d[c], off);
                    ind_s[c] += __shfl_xor(ind_s[c], off);
                }
            }
        }
        if (lane == 0) {
            float* out = partial + (size_t)wave * (BOUNCE ? PARTIAL_BOUNCE : PARTIAL_DIRECT);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                out[c] = dir_d[c]; out[3 + c] = dir_s[c];
                if constexpr (BOUNCE) { out[6 + c] = ind_d[c]; out[9 + c] = ind_s[c]; }
            }
        }
    }
}

// a point's partials added in index order, and the means: n_diff, n_spec = the samples the diffuse and the specular sums are over
// (two-strategy: the Dd cosine samples and all D; MIS: all D both).  The indirect terms are normalised like the direct ones.
template <bool BOUNCE>
__global__ __launch_bounds__(256) void finish_kernel(const float* __restrict__ partial, int P_, int wpp, float n_diff, float n_spec,
                                                     float* __restrict__ rgb_lin, float* __restrict__ diffuse_lin, float* __restrict__ spec_lin,
                                                     float* __restrict__ indirect_lin) {
#pragma clang fp contract(off)
    constexpr int PF = BOUNCE ? PARTIAL_BOUNCE : PARTIAL_DIRECT;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P_) return;
    float s[PF];
#pragma unroll
    for (int c = 0; c < PF; ++c) s[c] = 0.f;
    for (int k = 0; k < wpp; ++k) {
        const float* in = partial + ((size_t)p * wpp + k) * PF;
#pragma unroll
        for (int c = 0; c < PF; ++c) s[c] += in[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float df = s[c] / n_diff, sp = s[3 + c] / n_spec;
        float ind = 0.f;
        if constexpr (BOUNCE) ind = s[6 + c] / n_diff + s[9 + c] / n_spec;
        rgb_lin[(size_t)p * 3 + c] = BOUNCE ? (df + sp) + ind : df + sp;
        if (diffuse_lin) diffuse_lin[(size_t)p * 3 + c] = df;
        if (spec_lin) spec_lin[(size_t)p * 3 + c] = sp;
        if constexpr (BOUNCE) {
            if (indirect_lin) indirect_lin[(size_t)p * 3 + c] = ind;
        }
    }
}

// ---- argument checks, launch ------------------------------------------------------------------------------------------------------------
int check_mesh(const char* who, const Handle* h, const float* verts, int V, const int* tris, int T, const float* mat5) {
    char msg[200];
    if (!verts || !tris || !mat5) { snprintf(msg, sizeof(msg), "%s: null verts, tris or mat5", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (V < 1) { snprintf(msg, sizeof(msg), "%s: V must be >= 1", who); return nero_fail(NERO_ERR_ARG, msg); }
    if (T != h->b.n_tris) {
        snprintf(msg, sizeof(msg), "%s: T = %d, but the tree was built from %d triangles: tris must be the array it was built from", who, T,
                 h->b.n_tris);
        return nero_fail(NERO_ERR_ARG, msg);
    }
    return NERO_OK;
}

template <bool MIS, bool BOUNCE, bool RAYS>
int launch(const char* who, const Handle* h, const Samples& S, const If<BOUNCE, Mesh>& M, const EnvMap& E, float* partial,
           const If<BOUNCE, RayOut>& R, hipStream_t s) {
    const long long total = total_lanes(S.P, S.Dd, S.Ds, S.Dl);
    with_walk(h, [&](auto overlap, int threads) {
        hipLaunchKernelGGL((relight_kernel<MIS, BOUNCE, decltype(overlap)::value, RAYS>), dim3(grid_blocks(total, threads)), dim3(threads), 0, s,
                           h->b.d_nodes, h->b.d_tris, h->root, S, M, E, partial, R);
    });
    return nero_check_launch(who);
}

int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need, const char* sizer) {
    if (ws && ((uintptr_t)ws & 3u) == 0 && ws_bytes >= need) return NERO_OK;
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: workspace missing, misaligned or smaller than %s", who, sizer);
    return nero_fail(NERO_ERR_ARG, msg);
}

// what a fused entry point does once its arguments are checked and P > 0: the workspace (sized by the entry point `sizer` names), the
// estimator, the finishing pass
template <bool MIS, bool BOUNCE>
int estimate(const char* who, const char* sizer, const Handle* h, const Samples& S, const If<BOUNCE, Mesh>& M, const EnvMap& E, float* rgb_lin,
             float* diffuse_lin, float* spec_lin, float* indirect_lin, void* ws, size_t ws_bytes, hipStream_t s) {
    const size_t need = workspace_bytes(S.P, S.Dd, S.Ds, S.Dl, BOUNCE ? PARTIAL_BOUNCE : PARTIAL_DIRECT);
    if (check_workspace(who, ws, ws_bytes, need, sizer) != NERO_OK) return NERO_ERR_ARG;
    float* partial = (float*)ws;
    if (launch<MIS, BOUNCE, false>(who, h, S, M, E, partial, {}, s) != NERO_OK) return NERO_ERR_LAUNCH;
    const float n_spec = (float)(S.Dd + S.Ds + S.Dl), n_diff = MIS ? n_spec : (float)S.Dd;
    hipLaunchKernelGGL(finish_kernel<BOUNCE>, dim3(grid_blocks(S.P, 256)), dim3(256), 0, s, partial, S.P, S.wpp, n_diff, n_spec, rgb_lin,
                       diffuse_lin, spec_lin, indirect_lin);
    char what[64];
    snprintf(what, sizeof(what), "%s (finish)", who);
    return nero_check_launch(what);
}

}  // namespace

extern "C" {

size_t nero_relight_workspace_bytes(int P, int Dd, int Ds) {
    if (!samples_ok(Dd, Ds, 0) || !total_ok(P, Dd, Ds, 0)) return 0;
    return workspace_bytes(P, Dd, Ds, 0, PARTIAL_DIRECT);
}

size_t nero_relight_mis_workspace_bytes(int P, int Dd, int Ds, int Dl) {
    if (!mis_samples_ok(Dd, Ds, Dl) || !total_ok(P, Dd, Ds, Dl)) return 0;
    return workspace_bytes(P, Dd, Ds, Dl, PARTIAL_DIRECT);
}

size_t nero_relight_bounce_workspace_bytes(int P, int Dd, int Ds) {
    if (!samples_ok(Dd, Ds, 0) || !total_ok(P, Dd, Ds, 0)) return 0;
    return workspace_bytes(P, Dd, Ds, 0, PARTIAL_BOUNCE);
}

size_t nero_relight_mis_bounce_workspace_bytes(int P, int Dd, int Ds, int Dl) {
    if (!mis_samples_ok(Dd, Ds, Dl) || !total_ok(P, Dd, Ds, Dl)) return 0;
    return workspace_bytes(P, Dd, Ds, Dl, PARTIAL_BOUNCE);
}

int nero_bvh_relight(void* handle, const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                     const float* env, int eh, int ew, int convention, const float* rot, float clamp_max, float* rgb_lin, float* diffuse_lin,
                     float* spec_lin, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "nero_bvh_relight";
    if (!handle || !pt || !tab_d || !tab_s || !rgb_lin) return nero_fail(NERO_ERR_ARG, "nero_bvh_relight: null handle or pointer");
    if (check_samples(who, P, Dd, Ds, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env(who, env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const Samples S = {pt, tab_d, tab_s, nullptr, nullptr, nullptr, nullptr, nullptr, P, Dd, Ds, 0, waves_per_point(Dd, Ds, 0), geometry_type, 1, 1};
    return estimate<false, false>(who, "nero_relight_workspace_bytes", (const Handle*)handle, S, Absent{}, E, rgb_lin, diffuse_lin, spec_lin,
                                  nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int nero_bvh_relight_mis(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l, int P,
                         int Dd, int Ds, int Dl, int geometry_type, const float* env, int eh, int ew, int convention, const float* rot,
                         float clamp_max, const int64_t* cdf, const int64_t* info, float* rgb_lin, float* diffuse_lin, float* spec_lin, void* ws,
                         size_t ws_bytes, void* stream) {
    const char* who = "nero_bvh_relight_mis";
    if (!handle || !pt || !tab_d || !tab_s || !tab_l || !cdf || !info || !rgb_lin)
        return nero_fail(NERO_ERR_ARG, "nero_bvh_relight_mis: null handle or pointer");
    if (check_mis_samples(who, P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env(who, env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (check_table_size(who, eh, ew) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const Samples S = {pt, tab_d, tab_s, tab_l, rand_l, nullptr, cdf, info, P, Dd, Ds, Dl, waves_per_point(Dd, Ds, Dl), geometry_type, eh, ew};
    return estimate<true, false>(who, "nero_relight_mis_workspace_bytes", (const Handle*)handle, S, Absent{}, E, rgb_lin, diffuse_lin, spec_lin,
                                 nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int nero_bvh_relight_bounce(void* handle, const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, int geometry_type,
                            const float* env, int eh, int ew, int convention, const float* rot, float clamp_max, const float* verts, int V,
                            const int* tris, int T, const float* mat5, const float* normals, const unsigned* key, float* rgb_lin,
                            float* diffuse_lin, float* spec_lin, float* indirect_lin, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "nero_bvh_relight_bounce";
    if (!handle || !pt || !tab_d || !tab_s || !rgb_lin) return nero_fail(NERO_ERR_ARG, "nero_bvh_relight_bounce: null handle or pointer");
    if (check_samples(who, P, Dd, Ds, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env(who, env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    const Handle* h = (const Handle*)handle;
    if (check_mesh(who, h, verts, V, tris, T, mat5) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const Samples S = {pt, tab_d, tab_s, nullptr, nullptr, key, nullptr, nullptr, P, Dd, Ds, 0, waves_per_point(Dd, Ds, 0), geometry_type, 1, 1};
    const Mesh M = {verts, tris, mat5, normals, h->b.d_face, V, T};
    return estimate<false, true>(who, "nero_relight_bounce_workspace_bytes", h, S, M, E, rgb_lin, diffuse_lin, spec_lin, indirect_lin, ws, ws_bytes,
                                 (hipStream_t)stream);
}

int nero_bvh_relight_mis_bounce(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l,
                                int P, int Dd, int Ds, int Dl, int geometry_type, const float* env, int eh, int ew, int convention,
                                const float* rot, float clamp_max, const int64_t* cdf, const int64_t* info, const float* verts, int V,
                                const int* tris, int T, const float* mat5, const float* normals, const unsigned* key, float* rgb_lin,
                                float* diffuse_lin, float* spec_lin, float* indirect_lin, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "nero_bvh_relight_mis_bounce";
    if (!handle || !pt || !tab_d || !tab_s || !tab_l || !cdf || !info || !rgb_lin)
        return nero_fail(NERO_ERR_ARG, "nero_bvh_relight_mis_bounce: null handle or pointer");
    if (check_mis_samples(who, P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    EnvMap E;
    if (check_env(who, env, eh, ew, convention, rot, clamp_max, &E) != NERO_OK) return NERO_ERR_ARG;
    if (check_table_size(who, eh, ew) != NERO_OK) return NERO_ERR_ARG;
    const Handle* h = (const Handle*)handle;
    if (check_mesh(who, h, verts, V, tris, T, mat5) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const Samples S = {pt, tab_d, tab_s, tab_l, rand_l, key, cdf, info, P, Dd, Ds, Dl, waves_per_point(Dd, Ds, Dl), geometry_type, eh, ew};
    const Mesh M = {verts, tris, mat5, normals, h->b.d_face, V, T};
    return estimate<true, true>(who, "nero_relight_mis_bounce_workspace_bytes", h, S, M, E, rgb_lin, diffuse_lin, spec_lin, indirect_lin, ws,
                                ws_bytes, (hipStream_t)stream);
}

int nero_relight_bounce_rays(void* handle, const float* pt, const float* tab_d, const float* tab_s, const float* tab_l, const float* rand_l, int P,
                             int Dd, int Ds, int Dl, int geometry_type, const int64_t* cdf, const int64_t* info, int gh, int gw,
                             const float* verts, int V, const int* tris, int T, const float* mat5, const float* normals, const unsigned* key,
                             unsigned char* state, int* face, float* bary, float* sec_o, float* sec_d, int* strategy, float* pdf_l,
                             int* cell, void* stream) {
    const char* who = "nero_relight_bounce_rays";
    if (!handle || !pt || !tab_d || !tab_s) return nero_fail(NERO_ERR_ARG, "nero_relight_bounce_rays: null handle or pointer");
    const bool mis = tab_l != nullptr;
    if (mis) {
        if (!cdf || !info) return nero_fail(NERO_ERR_ARG, "nero_relight_bounce_rays: tab_l without cdf and info");
        if (check_mis_samples(who, P, Dd, Ds, Dl, geometry_type) != NERO_OK) return NERO_ERR_ARG;
        if (!map_ok(gh, gw)) return nero_fail(NERO_ERR_ARG, "nero_relight_bounce_rays: gh and gw must be in [1, 16384] and gh * gw at most 2^26");
    } else {
        if (Dl != 0) return nero_fail(NERO_ERR_ARG, "nero_relight_bounce_rays: Dl must be 0 without tab_l");
        if (check_samples(who, P, Dd, Ds, geometry_type) != NERO_OK) return NERO_ERR_ARG;
    }
    const Handle* h = (const Handle*)handle;
    if (check_mesh(who, h, verts, V, tris, T, mat5) != NERO_OK) return NERO_ERR_ARG;
    if (P == 0) return NERO_OK;
    const Samples S = {pt, tab_d, tab_s, tab_l, mis ? rand_l : nullptr, key, mis ? cdf : nullptr, mis ? info : nullptr, P, Dd, Ds, Dl,
                       waves_per_point(Dd, Ds, Dl), geometry_type, mis ? gh : 1, mis ? gw : 1};
    const Mesh M = {verts, tris, mat5, normals, h->b.d_face, V, T};
    const RayOut R = {state, face, bary, sec_o, sec_d, strategy, pdf_l, cell};
    EnvMap E = {};
    return mis ? launch<true, true, true>(who, h, S, M, E, nullptr, R, (hipStream_t)stream)
               : launch<false, true, true>(who, h, S, M, E, nullptr, R, (hipStream_t)stream);
}

}  // extern "C"
