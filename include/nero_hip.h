/* nero_hip.h -- C ABI of libnero_hip.so, the MI355X (gfx950) implementation of the NeRO Stage-I/II render-step hot path.
 *
 * The reference (liuyuan-pal/NeRO) is pure Python/PyTorch: it has no FFI for this path except two third-party CUDA
 * extensions (`_raytracing.create_raytracer/trace`, raytracing/raytracer.py:19,49, and `nvdiffrast.torch.texture`,
 * network/field.py:612).  The entry points below are therefore the boundary a maintainer binds with ctypes from the
 * reference's own modules (INTEGRATION.md shows the stubs); each one cites the reference code it replaces.
 *
 * Conventions: every pointer is a DEVICE pointer to fp32 (or int32 where stated) unless marked host; matrices are
 * row-major with an explicit leading dimension; every row count `n` may be any value >= 0 but all row buffers must be
 * allocated for NERO_ROW_PAD(n) rows; every call is asynchronous on `stream` (a hipStream_t passed as void*); every
 * function returns 0 on success or a negative error code, with a message available from nero_last_error().
 * Nothing here allocates device memory or synchronises, except nero_bvh_create / nero_bvh_create_device / nero_bvh_destroy (the
 * library owns BVH handles), nero_bvh_export (a synchronous copy to the host), the one-time upload of the IDE coefficient table, and
 * the calls that say they read a count back (one synchronisation each, on `stream`).
 */
#ifndef NERO_HIP_H
#define NERO_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERO_TILE_ROWS 64
#define NERO_ROW_PAD(n) (((n) + 63) / 64 * 64)
#define NERO_MAX_LAYERS 10
#define NERO_HID 256              /* leading dimension of every saved hidden activation matrix */

enum { NERO_ACT_NONE = 0, NERO_ACT_RELU = 1, NERO_ACT_SOFTPLUS100 = 2 };
/* arithmetic of the dense layers.  F32: v_mfma_f32_32x32x2_f32, an exact fp32 fmaf chain (157 TFLOP/s peak).
 * BF16X6: every fp32 operand is carried as three bf16 planes (exact 3-way split) and each product is the sum of the six
 * significant plane products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- dropped terms <= 3*2^-27 relative, i.e.
 * below fp32's own rounding; 417 TFLOP/s fp32-equivalent peak.  Packed operands are mode specific. */
/* F16X3: operands as two fp16 planes h = fp16(xs), l = fp16(xs - h) of their block-scaled value xs (per activation row / per weight
 * matrix, exact powers of two that put the block maximum into [2^14, 2^15), the top of fp16's range), three plane products
 * hw hx + hw lx + lw hx accumulated into ONE fp32 accumulator set -- half the MFMA count of BF16X6 at the same error class
 * (representation error <= 2^-24 of the block maximum, dropped term <= 2^-24 of the product; the format of rounds 1-4: docs/experiments.md). */
/* (value 3 was NERO_GEMM_F16X3P, the two-workgroups-per-CU forward engine of rounds 2-3, removed in round 4 for a wrong partial sum in one
 * launch of three at size.  Round 5 found the mechanism -- packed fp32 beside another wave's MFMAs, DESIGN.md 9.3 -- and the kernels are
 * back as an execution detail of F16X3, nero_f16_paired below: not a mode, the value 3 stays refused.) */
enum { NERO_GEMM_F32 = 0, NERO_GEMM_BF16X6 = 1, NERO_GEMM_F16X3 = 2 };
enum { NERO_OK = 0, NERO_ERR_ARG = -1, NERO_ERR_LAUNCH = -2, NERO_ERR_UNSUPPORTED = -3, NERO_ERR_NOMEM = -4 };

const char* nero_last_error(void);
int nero_version(void);
/* Would a caller-owned workspace of `need_bytes` fit the current device?  The step drivers below never allocate -- the caller hands over ONE
 * workspace sized by nero_stage1_workspace_bytes / nero_stage2_workspace_bytes (31 GiB typical, 52 GiB worst case at 4096 rays) -- so the place
 * to fail cleanly is in front of the caller's allocation: NERO_OK when need_bytes <= free device memory + reusable_bytes (memory the caller
 * will release or re-use for it: its previous workspace, its allocator's cached blocks), else NERO_ERR_NOMEM with the byte counts and `what`
 * in nero_last_error().  (The reference has no counterpart: torch raises an allocator OOM from wherever the step happens to be.) */
int nero_check_device_memory(size_t need_bytes, size_t reusable_bytes, const char* what);
/* per-launch HIP-event timing of the MFMA kernel classes {0 forward, 1 tangent, 2 reverse, 3 weight-gradient GEMM}:
 * report fills out[kind*3 + {0,1,2}] = {launches, total ms, total algorithmic flops} (host array of 12 doubles). */
int nero_prof_enable(int on);
int nero_prof_report(double* out);
/* the same per kernel, 24 doubles: classes 0-3 = the 512-thread chain kernels and the weight-gradient GEMM alone, 4 / 5 / 6 = the forward /
 * tangent / reverse launches that ran on the two-workgroups-per-CU kernels (nero_f16_paired), 7 unused */
int nero_prof_report_kernels(double* out);

/* ---- weight packing -------------------------------------------------------------------------------------------
 * Packs (a column window of) an effective weight matrix W[rows, ld] into the MFMA B-operand order used by the chain
 * kernels:  out[((c*NT + nt)*64 + lane)*4 + t] = B[8c + 4(lane>>5) + t][32nt + (lane&31)] * scale, zero outside.
 *   transpose == 0 ("forward" operand):  B[k][n] = W[n][col0 + k],  K = ncols,  N = nrows
 *   transpose == 1 ("backward" operand): B[k][n] = W[k][col0 + n],  K = nrows,  N = ncols
 * K is padded to a multiple of 8 (kpad), N to 32*nt_count.  Replaces the per-call cuBLAS operand handling inside
 * nn.Linear (network/field.py:142, 266, 325-331). */
int nero_pack_weight(const float* W, int nrows, int ld, int col0, int ncols, int transpose, float scale,
                     int kpad, int nt_count, float* out, void* stream);
/* NERO_GEMM_BF16X6 operand: same (W, window, transpose, scale) meaning; kpad is a multiple of 16 and the image holds three
 * bf16 planes in A-fragment order, nt_count * (kpad/16) * 3072 bytes:
 *   out[(((t*(kpad/16) + c)*3 + p)*64 + lane)*8 + j] = plane_p(A[32t + (lane&31)][16c + 8(lane>>5) + j]),
 *   transpose == 0: A[m][k] = W[m][col0 + k] (M = nrows, K = ncols);  transpose == 1: A[m][k] = W[k][col0 + m] */
int nero_pack_weight_split(const float* W, int nrows, int ld, int col0, int ncols, int transpose, float scale,
                           int kpad, int nt_count, void* out, void* stream);

/* Batched form: up to NERO_MAX_PACK_JOBS packing / copy jobs of one network in ONE launch (a training step repacks ~90
 * operand images and copies ~60 bias / head vectors; as separate launches they are pure launch latency).
 *   kind 0: nero_pack_weight_split(W, nrows, ld, col0, ncols, transpose, scale, kpad, nt_count, out)
 *   kind 1: nero_pack_weight(...) with the same fields
 *   kind 2: 2-D copy  out[r*kpad + c] = W[r*ld + c],  r < nrows, c < ncols   (bias: nrows = 1; head weights [n_head][k] -> [4][256])
 *   kind 3: NERO_GEMM_F16X3 operand: out = [256-byte header: float 2^ew][two fp16 planes of A * 2^-ew in A-fragment order,
 *           (((t*(kpad/16) + c)*2 + p)*64 + lane)*16 bytes], ew = exponent of max|A|; `out` must be zero-filled by the caller */
#define NERO_MAX_PACK_JOBS 64
typedef struct {
    const float* W; void* out;
    int kind, nrows, ld, col0, ncols, transpose, kpad, nt_count;
    float scale; int pad_;
} nero_pack_job;
int nero_pack_batch(const nero_pack_job* jobs /*host*/, int n_jobs, void* stream);

/* ---- fused MLP chain ------------------------------------------------------------------------------------------
 * One workgroup owns a tile of 64 rows and walks the whole layer list with the activations resident in LDS; every
 * dense layer is computed with v_mfma_f32_32x32x2_f32.  Replaces the nn.Linear/softplus/ReLU sequences of
 * SDFNetwork.forward (network/field.py:130-147), NeRFNetwork.forward (:258-283), make_predictor (:310-346). */
typedef struct {
    const float* w_main;   /* packed fwd operand [k_main/8][n_tiles][64][4]; input = current LDS activation tile      */
    const float* w_aux;    /* packed fwd operand [k_aux/8][n_tiles][64][4];  input = aux tile (skip connections)      */
    const float* bias;     /* [32*n_tiles] or NULL                                                                    */
    float* save;           /* [rows_pad, 256] post-activation output, or NULL (forward-only evaluation)               */
    const float* head_w;   /* optional VALU head evaluated on this layer's INPUT tile: [n_head][256] row-major        */
    const float* head_b;   /* [n_head]                                                                                */
    float* head_out;       /* [rows_pad, 4]                                                                           */
    int k_main, k_aux;     /* multiples of 8 (0 = unused)                                                             */
    int n_tiles;           /* output width / 32 (0 = head-only pseudo layer)                                          */
    int n_head;            /* 0..4                                                                                    */
    int act;               /* NERO_ACT_*                                                                              */
    int head_k;            /* columns of the input tile the head reads (multiple of 4, <= 256)                        */
    uint32_t* relu_mask;   /* optional [rows_pad, 8] (F16X3 engine, ReLU layers): bit 16h + v of word [row][tile] = output
                              feature 32 tile + 4h + (v&3) + 8(v>>2) is > 0.  The reverse pass then reads 32 B per row
                              instead of the 1 KiB saved activation row (which only the weight-gradient GEMM still needs) */
} nero_fwd_layer;

typedef struct {
    const float* init;     /* [rows_pad, ld_init]: first k_init columns are loaded into the activation tile           */
    const float* aux;      /* [rows_pad, ld_aux]: first k_aux columns are loaded into the aux tile                    */
    int ld_init, k_init, ld_aux, k_aux;
    int n_layers, aux_wide; /* aux_wide: 0 -> aux tile holds <= 40 columns (2 workgroups/CU), 1 -> <= 88              */
    int gemm_mode, pad_;    /* NERO_GEMM_*: the packed operands must have been built for the same mode; BF16X6 wants
                               k_main / k_aux padded to multiples of 16                                               */
    double macs_per_row;    /* logical multiply-adds per row (profiling only)                                         */
    nero_fwd_layer layer[NERO_MAX_LAYERS];
} nero_fwd_chain;

int nero_mlp_forward(const nero_fwd_chain* chain /*host*/, int n_rows, void* stream);

/* Tangent (forward-mode) pass of a softplus chain: same layer walk with  adot_l = sigma'(a_l) * (W_l adot_{l-1})  and
 * inj_l = gbar_l * beta (1 - sigma'(a_l)) * zdot_l.  It is the "second-order" half of the backward of
 * SDFNetwork.gradient (network/field.py:155-167, create_graph=True); SURVEY.md App. E. */
typedef struct {
    const float* w_main; const float* w_aux;
    const float* a_saved;  /* [rows_pad,256] activations saved by the forward pass (for sigma')                       */
    const float* gbar;     /* [rows_pad,256] first-order backward signal saved by the normal pass; may be NULL when   */
                           /* inj is NULL (round 4: the F16X3 reverse kernel forms the injection itself, see          */
                           /* nero_bwd_layer.inj_adot)                                                                 */
    float* adot;           /* out [rows_pad,256]                                                                      */
    float* inj;            /* out [rows_pad,256], or NULL = not written (saves 1 KB read + 1 KB written per row and layer) */
    int k_main, k_aux, n_tiles, pad_;
} nero_tan_layer;

typedef struct {
    const float* init; const float* aux;
    int ld_init, k_init, ld_aux, k_aux;
    int n_layers, aux_wide;
    int gemm_mode, pad_;
    double macs_per_row;
    nero_tan_layer layer[NERO_MAX_LAYERS];
} nero_tan_chain;

int nero_mlp_tangent(const nero_tan_chain* chain /*host*/, int n_rows, void* stream);

/* Reverse pass of a chain: delta_{l-1} = (delta_l W_l [+ dy_head W_head]) * act'(a_{l-1}) [+ inj_{l-1}], every delta_l
 * written out for the weight-gradient GEMMs.  Replaces autograd's AddmmBackward / SoftplusBackward / ReluBackward
 * chain for the same modules. */
typedef struct {
    const float* w_main_t; /* packed bwd operand [n_out/8][k_main/32][64][4]                                          */
    const float* w_aux_t;  /* packed bwd operand [n_out/8][k_aux_tiles][64][4] or NULL                                */
    const float* a_prev;   /* [rows_pad,256] saved activation of the layer's INPUT (NULL for the first layer)          */
    const float* inj;      /* optional additive term for delta_{l-1} [rows_pad,256]                                   */
    float* delta_prev;     /* out [rows_pad,256] (NULL for the first layer)                                           */
    const float* head_w;   /* head on this layer's input tile: [n_head][256]                                          */
    const float* head_dy;  /* [rows_pad,4]                                                                            */
    int n_out;             /* K of the reverse GEMM (multiple of 8; 0 = head-only pseudo layer)                       */
    int k_main_tiles, k_aux_tiles, n_head;
    int act_prev;          /* activation that produced a_prev                                                         */
    int pad_;
    const uint32_t* mask_prev; /* optional relu_mask of the layer that produced a_prev (F16X3 engine): replaces reading a_prev */
    const float* inj_adot; /* F16X3 engine, softplus a_prev only.  When set, `inj` holds the first-order signal gbar_{l-1} and this the
                              tangent adot_{l-1} (both [rows_pad,256]) and the kernel forms the injection itself,
                              gbar * beta (1 - s) * adot / s  with s = sigma'(a_prev) -- the tangent pass then neither reads gbar
                              nor writes inj.  NULL = `inj` is the finished additive term (every engine).                    */
} nero_bwd_layer;

typedef struct {
    const float* dy;       /* [rows_pad, ld_dy] gradient w.r.t. the LAST dense layer's pre-activation output, or NULL */
    int ld_dy, k_dy;
    float* d_init;         /* out [rows_pad, ld_dinit] gradient w.r.t. the init columns (NULL = not needed)           */
    float* d_aux;          /* out [rows_pad, ld_daux]  gradient w.r.t. the aux columns, summed over the layers using it */
    int ld_dinit, ld_daux, accumulate_dinit;
    int n_layers, aux_wide;
    int gemm_mode;
    double macs_per_row;
    nero_bwd_layer layer[NERO_MAX_LAYERS];   /* in FORWARD order; walked from n_layers-1 down to 0                    */
} nero_bwd_chain;

int nero_mlp_backward(const nero_bwd_chain* chain /*host*/, int n_rows, void* stream);
/* Workgroup organisation of the F16X3 chain passes: bit 0 / 1 / 2 of `mask` = the forward / tangent / reverse pass runs with TWO 256-thread
 * workgroups per CU (mlp_f16p.hip: one's epilogue, barriers and HBM waits under the other's MFMAs) instead of one 512-thread workgroup
 * (mlp_f16x3.hip) on launches of more than 4 tiles of 64 rows per CU; bit 3 = on launches of every size.  Same packed operands, same
 * descriptors, the same results bit for bit (tests/test_paired_engine.py).  mask < 0 only queries; returns the previous selection.
 * Initial value: NERO_F16_PAIRED in the environment, default 3.  Process-wide, not thread-safe against concurrent launches.
 * (No reference counterpart: an execution detail of network/field.py's nn.Linear stacks.) */
int nero_f16_paired(int mask);

/* ---- weight-gradient GEMM ------------------------------------------------------------------------------------
 * dW[n][k] (+)= sum_r D0[r][n] * B0[r][k] (+ sum_r D1[r][n] * B1[r][k]),  db[n] (+)= sum_r D0[r][n]
 * split over row slices; `partials` holds n_slices * (n_out_pad*k_pad + n_out_pad) floats of workspace and is reduced
 * by the same call.  Output dW is row-major [n_out, ldw] written at column offset col0 (so skip-layer parts land in
 * place), scaled by `scale`.  Replaces autograd's mm(grad.t(), input) per Linear. */
typedef struct {
    const float* d0; const float* b0;   /* [rows_pad, ldd0], [rows_pad, ldb0] */
    const float* d1; const float* b1;   /* optional second pair (NULL)        */
    int ldd0, ldb0, ldd1, ldb1;
    int n_out, k_cols;                  /* logical sizes (<= 256 each)        */
    float* dW; int ldw, col0;
    float* db;                          /* [n_out] or NULL                    */
    float scale;
    int accumulate;                     /* 0: overwrite, 1: add into dW/db    */
    int gemm_mode, pad_;                /* NERO_GEMM_* (operands are plain fp32 matrices in every mode).  F16X3: three fp16
                                           plane products, each 16-row chunk block-scaled to the top of fp16's range, one fp32
                                           accumulator with a running unit (mlp_f16dw.hip); BF16X6: six bf16 products */
} nero_dw_job;

int nero_dw_workspace_floats(int n_rows);
int nero_dw_gemm(const nero_dw_job* job /*host*/, int n_rows, float* partials, void* stream);
/* The weight gradients of SEVERAL jobs over the same n_rows rows (all layers of one MLP chain).  Same results as n_jobs calls of
 * nero_dw_gemm up to the order of the row-slice sums: below 131072 rows the fp16 engine runs the jobs as ONE launch per kernel kind
 * (grid.y = job, ~1024 row slices over all jobs instead of 256 per job) plus one batched reduction -- a chain of the reference's own
 * train_ray_num = 512 batch, or the 2 P rows of the Stage-II material MLPs, otherwise pays 2 launches and 256 partial matrices per
 * layer for ~40 k rows.  At or above that row count, and for the other engines, it IS the per-job loop.  partials: as nero_dw_gemm. */
int nero_dw_gemm_batch(const nero_dw_job* jobs /*host*/, int n_jobs, int n_rows, float* partials, void* stream);

/* Head weight gradient: dWh[j][k] = sum_r dy[r][j] a[r][k] (+ extra[r][k] for j == 0 if extra != NULL), dbh[j] = sum_r dy[r][j]. */
int nero_head_dw(const float* dy /*[rows,4]*/, const float* a /*[rows,256]*/, const float* extra, int n_head, int n_rows,
                 float* dWh /*[n_head,256]*/, float* dbh, float* partials, int accumulate, void* stream);
/* the same with an explicit destination shape: dWh [n_head rows of k_cols columns, row pitch ld_dwh] (nero_head_dw: 256 / 256) */
int nero_head_dw_ld(const float* dy, const float* a, const float* extra, int n_head, int n_rows, float* dWh, int ld_dwh, int k_cols, float* dbh,
                    float* partials, int accumulate, void* stream);

/* ---- trainer-loop fusion (replaces the per-Linear nn.utils.weight_norm reparametrisation, network/field.py:
 *      118-119, 323-331, and torch.optim.Adam over ~125 tensors, train/trainer.py:105-170, ~750 tiny kernels per step) -------------
 * One job per weight-normed matrix (dim = 0: one norm per output row).  forward: w_eff = g v / ||v||_row, inv_norm = 1 / ||v||_row.
 * adam: dg = <dW, v> inv_norm, dv = g inv_norm (dW - <dW, v> inv_norm^2 v), then Adam on g and v in place (m_*, v_* = first / second
 * moment buffers).  Plain jobs: Adam on p given grad.  Hyper-parameters and operation order of torch.optim.Adam (fused). */
#define NERO_MAX_WN_JOBS 40
#define NERO_MAX_ADAM_JOBS 96
typedef struct {
    const float* v; const float* g;      /* forward inputs: weight_v [rows, cols], weight_g [rows]                                */
    float* w_eff; float* inv_norm;       /* forward outputs / backward inputs                                                     */
    float* v_rw; float* g_rw;            /* the same parameters, writable (updated in place by the Adam step)                     */
    const float* dW;                     /* dL/dW_eff [rows, cols]                                                                */
    float* m_v; float* v_v; float* m_g; float* v_g;
    int rows, cols;
} nero_wn_job;
/* step: 0 = this job uses the call's `step` argument; > 0 = the job's own 1-based Adam step (bias correction); < 0 = the tensor has no
 * gradient this step: skipped entirely -- torch.optim.Adam skips parameters whose .grad is None, their step counter and moments do not
 * advance (deviation_network.variance while step < freeze_inv_s_step, network/renderer.py:494-495). */
typedef struct { float* p; const float* grad; float* m; float* v; int n; int step; } nero_adam_job;
int nero_wn_forward_batch(const nero_wn_job* jobs /*host*/, int n_jobs, void* stream);
/* The weight-norm backward ALONE, for hosts that keep their own optimiser (the drop-in renderers under torch.optim.Adam: round 6): given
 * dL/dW_eff of every weight-normed matrix, dg = <dW, v> inv_norm and dv = g inv_norm (dW - <dW, v> inv_norm^2 v) in ONE launch -- what
 * autograd does per Linear through torch._weight_norm_interface_backward (nn.utils.weight_norm, network/field.py:118-119, 323-331).
 * inv_norm: the row norms nero_wn_forward_batch left behind.
 * All three calls: n_jobs / n_wn in [0, NERO_MAX_WN_JOBS], n_plain >= 0 (any number: chunks of NERO_MAX_ADAM_JOBS), step >= 1, a job array
 * with a positive count and every pointer a call uses non-NULL, rows, cols and n > 0; anything else is NERO_ERR_ARG before the first launch,
 * nothing written (nero_wn_adam_batch checks the plain jobs before it launches the weight-norm ones). */
typedef struct {
    const float* v; const float* g; const float* inv_norm; const float* dW;
    float* dv; float* dg;                /* out: [rows, cols], [rows]                                                                 */
    int rows, cols;
} nero_wn_grad_job;
int nero_wn_backward_batch(const nero_wn_grad_job* jobs /*host*/, int n_jobs, void* stream);
int nero_wn_adam_batch(const nero_wn_job* wn /*host*/, int n_wn, const nero_adam_job* plain /*host*/, int n_plain, float lr, float beta1,
                       float beta2, float eps, int step /*1-based*/, void* stream);

/* ---- encodings --------------------------------------------------------------------------------------------------
 * Positional encoding rows [x, sin(2^k x), cos(2^k x)]_{k<n_freq}, zero padded to ldo, rows >= n zero
 * (Embedder, network/field.py:14-58). */
int nero_encode_pe(const float* x, int ldx, int dim, int n_freq, int n, float* out, int ldo, void* stream);
/* out[r,0:3] = J_e(x_r)^T (e0[r] + e1[r])  -- input gradient of the SDF network through its PE-6 (the NORMAL,
 * SDFNetwork.gradient, network/field.py:155-167).  e1 may be NULL. */
int nero_pe_vjp(const float* x, int ldx, const float* e0, int ld0, const float* e1, int ld1, int n_freq, int n,
                float* out, int ldo, void* stream);
/* out[r] = J_e(x_r) t_r  (tangent of the PE; seeds the second-order pass), zero padded like nero_encode_pe. */
int nero_pe_jvp(const float* x, int ldx, const float* t, int ldt, int n_freq, int n, float* out, int ldo, void* stream);

/* ---- hierarchical sampling (NeROShapeRenderer.sample_ray / upsample / cat_z_vals, network/renderer.py:355-443;
 *      sample_pdf, network/field.py:399-429).  Per-ray tables: z [R, ldz], sdf [R, lds].
 *      Argument ranges (anything else: NERO_ERR_ARG before a launch, nothing written; R == 0 returns NERO_OK):
 *        nero_coarse_z      1 <= n <= 160, ldz >= n;           nero_background_z  n_bg >= 0, col0 >= 0, ldz >= col0 + n_bg
 *        nero_upsample / nero_sample_pdf   2 <= n <= 160, 0 <= m <= 32  (n <= 128: one wavefront per ray, else one thread per ray)
 *        nero_merge_sorted  n >= 1, m >= 0, n + m <= 160          (n <= 128 and m <= 64: one wavefront per ray, else one thread per ray)
 *      Row pitches (ldz, lds, ldb, ldw) may exceed the row length; columns beyond it are neither read nor written.
 *      z_new / w_out / inds_out / index_out are dense: [R,m], [R,n-1], [R,m], [R,n+m]. ----------------------------------------- */
int nero_coarse_z(const float* near, const float* far, const float* rand1 /*[R] or NULL*/, int R, int n, float* z, int ldz, void* stream);
int nero_background_z(const float* far, const float* rand_bg /*[R,n_bg] or NULL*/, int R, int n_bg, float* z, int ldz, int col0, void* stream);
/* PE-6 rows (ld 40) of the points o + d*z[r, col0+j], row = r*ncols + j */
int nero_ray_points_pe(const float* o, const float* d, const float* z, int ldz, int col0, int ncols, int R, float* pe, void* stream);
/* one up-sampling round: m new z per ray from the NeuS section weights of (z, sdf)[0..n).  inv_s = min(exp(10*variance), cap),
 * or cap when variance == NULL.  w_out [R,n-1] / inds_out int32 [R,m] optional (tests). */
int nero_upsample(const float* o, const float* d, const float* z, int ldz, const float* sdf, int lds, int n,
                  const float* variance, float inv_s_cap, int m, int R, float* z_new, float* w_out, int* inds_out, void* stream);
/* deterministic inverse-CDF sampling from given bins/weights; inds = searchsorted(cdf, u, right=True) (bit-exact contract) */
int nero_sample_pdf(const float* bins, int ldb, const float* w, int ldw, int n, int m, int R, float* out, int* inds_out, void* stream);
/* stable in-place merge of sorted z[r,0..n) with sorted z_new[r,0..m), ties: z first; z[r,0..n+m) is written.  sdf[r,0..n+m) is permuted
 * alike when BOTH sdf and sdf_new are given (either NULL: the table is left alone); sdf_new is dense [R,m] read with element stride ldsn
 * (column 0 of a head output [rows,4] -> ldsn = 4); index_out int32 [R,n+m] optional = position in the concatenation [z, z_new] */
int nero_merge_sorted(float* z, int ldz, int n, float* sdf, int lds, const float* z_new, int m, const float* sdf_new, int ldsn,
                      int R, int* index_out, void* stream);
/* sdf[r, i] = src[(r*n + i) * ld_src], i < n  (column 0 of a head output [rows,4] -> ld_src = 4) */
int nero_scatter_sdf(const float* src, int ld_src, int R, int n, float* sdf, int lds, void* stream);

/* ---- occlusion-loss march along the reflected rays (compute_occ_loss, network/renderer.py:522-548; get_intersection /
 *      get_weights / get_sphere_intersection, network/field.py:390-396, 432-484) ----------------------------------------- */
int nero_occ_candidates(const float* x4, const float* sdf4, const float* grad, const int* idx, const float* d, int T, float thresh,
                        int n, unsigned char* flag, void* stream);
int nero_occ_z(const float* o, const float* d, int P, int n, float* z /*[P,n]*/, void* stream);
/* sdf is read as sdf[(p*n+i)*lds] (column 0 of a head output [rows,4] -> lds = 4); w_out [P,n-1] and/or wsum [P] (at least one);
 * z is dense [P,n], n >= 1.  All three calls: every pointer but w_out / wsum is required (NULL: NERO_ERR_ARG); n == 0 / P == 0: NERO_OK. */
int nero_section_weights(const float* z, const float* sdf, int lds, int n, const float* variance, int P, float* w_out, float* wsum,
                         void* stream);

/* ---- render preparation (render_core, network/renderer.py:550-565): mid points, section lengths, inner/outer split ---- */
/* pts4 [R*T,4] = (x,y,z,dist); ray_counts/ray_off int32 [R]; counts int32 [2] = (#inner, #outer).  T >= 1 (2 <= T <= 192: one
 * wavefront per ray, else one thread per ray); z is dense [R,T].  nero_compact: inner_idx [#inner] / outer_idx [#outer] = the flat sample
 * indices r*T + i in ascending order.  nero_gather_*: rows n .. NERO_ROW_PAD(n)-1 of every output are written as zeros; n == 0: NERO_OK. */
int nero_render_prep(const float* o, const float* d, const float* z, int R, int T, float* pts4, int* ray_counts, int* ray_off,
                     int* counts, void* stream);
int nero_compact(const float* pts4, const int* ray_off, int R, int T, int* inner_idx, int* outer_idx, void* stream);
int nero_gather_inner(const float* pts4, const int* idx, int n, float* x4 /*[rows,4]*/, float* pe /*[rows,40]*/, void* stream);
int nero_gather_outer(const float* pts4, const float* d, const int* idx, int T, int n, float* pe88, float* pev32, float* dist, void* stream);

/* ---- Stage-I shading and compositing (everything from here to the mesh ray tracer), and nero_pe_vjp / nero_pe_jvp above.
 *      Argument ranges (anything else: NERO_ERR_ARG before a launch, nothing written; n == 0 / R == 0 returns NERO_OK):
 *        n >= 0, R >= 0, T >= 1 (T divides the flat sample index: sample k belongs to ray idx[k] / T);
 *        nero_composite_*: T <= 192: one wavefront per ray, else one thread per ray;
 *        every pointer is required except:  d_gerr, d_geo (nero_sdf_alpha_bwd: a NULL one contributes nothing);  d_occ (nero_shade_combine_bwd);
 *        the d_geo argument of nero_shade_combine_bwd (unused);  extra (nero_shade_encode_bwd);  x4 of nero_shade_encode_bwd unless
 *        sphere_direction;  e1 (nero_pe_vjp);  Lh / hmask, given together or not at all, and dLh, given exactly when Lh is.
 *      Rows.  "rows" below is NERO_ROW_PAD(n); the MLP chains read whole 64-row blocks, so these outputs get their pad rows
 *      n .. NERO_ROW_PAD(n)-1 written as ZEROS, every column of the row:
 *        nero_sdf_alpha_bwd      d_sdf4 [rows,4], dinv [rows]                 (d_grad [n,3]: live rows only)
 *        nero_shade_encode       Xd, Xs [rows,72|144], Xi [rows,128], Xo [rows,96]      (mat [n,8]: live rows only)
 *        nero_human_encode       Xh [rows,24], hmask [rows]
 *        nero_shade_combine_bwd  dLd, dLs, dLi, dLo, dLh [rows,4]             (dmat [n,8]: live rows only)
 *        nero_shade_encode_bwd   d_geo [rows,8], dm_raw, dr_raw, da_raw [rows,4]
 *        nero_nerf_head_bwd      d_sig4, d_rgb4 [rows,4]
 *        nero_pe_jvp / nero_encode_pe   out [rows,ldo] (and columns beyond the encoding of the live rows)
 *      Every other output is written for the n live rows (R rays) only and nothing behind them is touched: alpha, geo, gerr, color,
 *      occ_prob, rec, extra, the nerf head's alpha / color, weights, rgb, d_alphaRT, d_colorRT, d_a, d_c; nero_pe_vjp writes out[r,0:3]
 *      and leaves the columns up to ldo alone; nero_scatter_samples writes exactly the slots idx names.  Gradient rows [.,4] carry their
 *      values in the leading columns (d_sdf4: 1, dm_raw / dr_raw: 1, da_raw: 3, dL*: 3, dLo: 1, dLh: 4) and zeros behind. ---- */
/* ---- inner samples: NeuS alpha + shading frame + eikonal term (compute_sdf_alpha, network/renderer.py:484-512, 574) ---- */
/* geo [rows,8] = { nhat(3), NoV, refl(3), |grad| };  variance: device pointer to deviation_network.variance.  nhat = grad / max(|grad|, 1e-12)
 * (F.normalize): on a row with grad == 0 d_grad still receives d_nhat / 1e-12, the norm itself carries no gradient there */
int nero_sdf_alpha_fwd(const float* sdf4, const float* grad, const float* x4, const int* idx, const float* d, int T,
                       const float* variance, float anneal, int n, float* alpha, float* geo, float* gerr, void* stream);
int nero_sdf_alpha_bwd(const float* sdf4, const float* grad, const float* x4, const int* idx, const float* d, int T,
                       const float* variance, float anneal, int n, const float* d_alpha, const float* d_gerr, const float* d_geo,
                       float* d_sdf4, float* d_grad, float* dinv /*[rows_pad] per-sample d inv_s*/, void* stream);

/* ---- split-sum shader algebra (AppShadingNetwork.forward, network/field.py:591-651; IDE utils/ref_utils.py:53-117;
 *      dr.texture field.py:612; linear_to_srgb utils/raw_utils.py:4-10) ------------------------------------------------ */
/* sphere_direction != 0 (shader_config.sphere_direction, field.py:558-562, 582-586): Xd / Xs rows are 144 wide,
 * [IDE(v, .) | IDE(normalised sphere exit point of the ray (offset_points_to_sphere(p), v), .)] for v = normal / reflection */
int nero_shade_encode(const float* x4, const float* geo, const float* m_raw, const float* r_raw, const float* a_raw, int n,
                      float* mat /*[rows,8]*/, float* Xd /*[rows,72|144]*/, float* Xs /*[rows,72|144]*/, float* Xi /*[rows,128]*/,
                      float* Xo /*[rows,96]*/, int sphere_direction, void* stream);
/* Lh [rows,4] raw human-light head + hmask [rows] (from nero_human_encode), or NULL/NULL when shader_config.human_light is off */
int nero_shade_combine_fwd(const float* geo, const float* mat, const float* Ld, const float* Ls, const float* Li, const float* Lo,
                           const float* lut /*[256,256,2]*/, float exp_max, int n, float* color /*[n,3]*/, float* occ_prob,
                           const float* Lh, const float* hmask, void* stream);
/* dmat[k] = { d_metallic, d_rough (LUT part), d_albedo(3), d_NoV (LUT part), 0, 0 }: whole rows.  d_geo is NOT written here (round 5: the
 * argument is kept for the ABI); nero_shade_encode_bwd writes every row of d_geo once: { d_nhat(3), d_NoV = dmat[k][5], d_refl(3), 0 } */
int nero_shade_combine_bwd(const float* geo, const float* mat, const float* Ld, const float* Ls, const float* Li, const float* Lo,
                           const float* lut, float exp_max, int n, const float* d_color, const float* d_occ /*or NULL*/, float* dLd,
                           float* dLs, float* dLi, float* dLo, float* dmat /*[rows,8]*/, float* d_geo /*[rows,8]*/,
                           const float* Lh, const float* hmask, float* dLh, void* stream);
/* validation-only shader intermediates (inter_results=True, network/field.py:630-649): rec [n,32], layout in shade.hip */
int nero_shade_inter_results(const float* geo, const float* mat, const float* Ld, const float* Ls, const float* Li, const float* Lo,
                             const float* lut, float exp_max, int n, const float* Lh, const float* hmask, float* rec, void* stream);
/* extra [rows,4] = { d_refl(3), d_rough } from nero_human_encode_bwd, or NULL */
int nero_shade_encode_bwd(const float* geo, const float* mat, const float* dXd, const float* dXs, const float* dXi, const float* dmat,
                          int n, float* d_geo, float* dm_raw, float* dr_raw, float* da_raw, const float* extra,
                          const float* x4 /*sample positions [rows,4]; needed when sphere_direction*/, int sphere_direction, void* stream);
/* human ("photo capturer") light input (predict_human_light, network/field.py:536-552; get_camera_plane_intersection :348-367;
 * IPE :369-378): Xh [rows,24], hmask [rows]; poses [R,3,4] human-frame poses per RAY, sample k belongs to ray idx[k]/T */
int nero_human_encode(const float* x4, const float* geo, const float* mat, const int* idx, int T, const float* poses, int n,
                      float* Xh, float* hmask, void* stream);
int nero_human_encode_bwd(const float* x4, const float* geo, const float* mat, const int* idx, int T, const float* poses, int n,
                          const float* dXh, float* extra, void* stream);

/* ---- NeRF++ head (compute_density_alpha, network/renderer.py:514-520) and compositing (renderer.py:578-579) ----------- */
int nero_nerf_head_fwd(const float* sig4, const float* rgb4, const float* dist, int n, float* alpha, float* color, void* stream);
int nero_nerf_head_bwd(const float* sig4, const float* rgb4, const float* dist, int n, const float* d_alpha, const float* d_color,
                       float* d_sig4, float* d_rgb4, void* stream);
int nero_scatter_samples(const float* a, const float* c, const int* idx, int n, float* alphaRT, float* colorRT, void* stream);
int nero_composite_fwd(const float* alphaRT, const float* colorRT, int R, int T, float* weights, float* rgb, void* stream);
int nero_composite_bwd(const float* alphaRT, const float* colorRT, const float* weights, const float* d_rgb, int R, int T,
                       float* d_alphaRT, float* d_colorRT, void* stream);
int nero_gather_sample_grads(const float* d_alphaRT, const float* d_colorRT, const int* idx, int n, float* d_a, float* d_c, void* stream);

/* ---- mesh ray tracer (Stage II).  Replaces the third-party CUDA extension `_raytracing` behind raytracing/raytracer.py:
 *      create_raytracer(vertices, triangles) (:19) and impl.trace(rays_o, rays_d, positions, face_normals, depth) (:49).
 *      verts [nV,3] float32 / tris [nT,3] int32 are HOST arrays; rays and outputs are device arrays.  Closest hit with t > 0;
 *      face normal = normalize(cross(v1-v0, v2-v0)); a miss reports depth = 10, position = o + 10 d, normal = 0
 *      (NeROMaterialRenderer.trace treats depth >= 10 as a miss, network/renderer.py:727). */
int nero_bvh_create(const float* verts, int nV, const int* tris, int nT, void** handle);
int nero_bvh_trace(void* handle, const float* rays_o, const float* rays_d, int n, float* positions, float* face_normals, float* depth,
                   void* stream);
/* nero_bvh_trace with a LAUNCH-ORDER hint (round 5): the rays come in groups of `group` (Stage II: the D = Dd + Ds secondary rays of a
 * surface point, field.py:856-880) whose entries [heavy_from, group) are the expensive ones (the GGX specular directions: the only rays
 * that can point below the surface and cross the inside of the mesh); their 64-ray chunks are started first, so that the launch ends
 * with short rays.  Outputs identical to nero_bvh_trace's.  group, heavy_from multiples of 64, 0 < heavy_from < group, n % group == 0;
 * otherwise the natural order. */
int nero_bvh_trace_grouped(void* handle, const float* rays_o, const float* rays_d, int n, float* positions, float* face_normals, float* depth,
                           int group, int heavy_from, void* stream);
/* nero_bvh_trace for a caller that knows some rays' results will not be used (round 6): skip [n] bytes, non-zero = do not traverse; such a
 * ray is reported as a miss (depth 10, zero normal).  Every other ray's outputs are nero_bvh_trace's bit for bit; skip = NULL: the same call.
 * Stage II passes the flags of nero_mc_dead_rays: GGX-sampled directions below the shading horizon, whose estimator weight is exactly zero
 * (field.py:892-903, 979-987 with geometry_type 'schlick') and which are the longest rays of the launch (they cross the inside of the mesh). */
int nero_bvh_trace_masked(void* handle, const float* rays_o, const float* rays_d, int n, const unsigned char* skip, float* positions,
                          float* face_normals, float* depth, void* stream);
/* nero_bvh_trace_masked (skip may be NULL) with an explicit LAUNCH ORDER: rays in groups of n_order * 64; phase p of the launch holds chunk
 * order[p] of every group (a permutation of 0 .. n_order-1, n_order <= 32, n % (64 n_order) == 0; anything else falls back to the natural order).
 * Outputs identical to nero_bvh_trace_masked's.  Stage II starts the chunks in DESCENDING order: the later entries of both direction tables
 * (field.py:741-749) are the grazing directions, the long traversals; with them first the launch no longer ends on a handful of waves. */
int nero_bvh_trace_ordered(void* handle, const float* rays_o, const float* rays_d, int n, const unsigned char* skip, const int* order, int n_order,
                           float* positions, float* face_normals, float* depth, void* stream);
int nero_bvh_destroy(void* handle);
/* which kernel nero_bvh_trace launches: 1 = memory requests of a traversal step overlapped, stack in LDS (default when the tree is no
 * deeper than the 24-entry LDS stack), 0 = private stack, one request after the other.  Same visit order and arithmetic per ray:
 * bit-identical outputs. */
int nero_bvh_set_traversal(void* handle, int mode);
/* ---- the same tree built ON THE DEVICE from a device-resident mesh (bvh_build.hip; DESIGN.md, "BVH build on the device").
 *      nero_bvh_create splits a range of n > 4 triangles at lo + n / 2, so node indices, ranges, leaf references and depth depend on nT alone;
 *      the device build sorts where the host partitions (stable, ascending, -0 == +0: equal centroids keep their order) and so produces the
 *      host tree -- the same node bytes and the same triangles per leaf wherever no two centroids tie at a median -- bit-reproducibly.
 * nero_bvh_build_workspace_bytes: host arithmetic, no device needed; 0 = unsupported (nV < 3, nT < 1 or nT >= 2^27).  About 84 nT bytes plus
 *   the radix sort's scratch.  Non-decreasing in nT.
 * nero_bvh_build_lds_capacity: S, the largest range the finishing kernel sorts in LDS; ranges above it are sorted globally, level by level.
 * nero_bvh_create_device: d_verts [nV,3] float32 / d_tris [nT,3] int32 are DEVICE arrays, read only; ws: nero_bvh_build_workspace_bytes(nV, nT)
 *   bytes of device memory, free for reuse once the work queued on `stream` has run.  All work runs on `stream`; the library allocates the
 *   node and triangle buffers (as nero_bvh_create).  ONE synchronisation: the count of bad triangles (a vertex index outside [0, nV) or a
 *   non-finite coordinate) is read back on `stream` before anything is allocated; a non-zero count returns NERO_ERR_ARG with the count in
 *   nero_last_error(), nothing stays allocated and *handle is untouched.  nT < 1, nV < 3, a null pointer or ws_bytes too small:
 *   NERO_ERR_ARG; nT >= 2^27: NERO_ERR_UNSUPPORTED (leaf references must stay above the no-node sentinel).  The handle has the traversal
 *   mode and depth nero_bvh_create would have set and serves every nero_bvh_trace*, nero_bvh_set_traversal and nero_bvh_destroy.
 * nero_bvh_info: any of the four outputs may be NULL.  max_depth = level of the deepest inner node, root = level 1 (0: the root reference is
 *   a leaf).  root = the root reference (0, or a leaf reference -(n) - 1 when nT <= 4).  Never synchronises.
 * nero_bvh_export: synchronous copy of the tree to HOST arrays -- n_nodes records of 64 bytes {lmin[3], lmax[3], rmin[3], rmax[3] float32,
 *   left, right, pad[2] int32} and n_tris records of 48 bytes {v0[3], e1[3], e2[3], pad[3] float32} in leaf order; waits for the device
 *   first.  Works for handles of either builder. */
size_t nero_bvh_build_workspace_bytes(int nV, int nT);
int nero_bvh_build_lds_capacity(void);
int nero_bvh_create_device(const float* d_verts, int nV, const int* d_tris, int nT, void* ws, size_t ws_bytes, void* stream, void** handle);
/* time of the calling process's LAST successful nero_bvh_create_device by phase, from HIP events the build records on its stream:
 * ms [4] (host) = prep, wide levels, finishing kernel, emit.  Waits for that build to finish.  For scripts/bench_bvh_build.py. */
int nero_bvh_build_last_phase_ms(float* ms);
int nero_bvh_info(void* handle, int* n_nodes, int* n_tris, int* max_depth, int* root);
int nero_bvh_export(void* handle, void* nodes_host, void* tris_host);

/* ---- Stage-II Monte-Carlo shading glue (MCShadingNetwork.shade_mixed and helpers, network/field.py:756-1012).
 *      Row r = p*D + j, D = Dd + Ds (j < Dd cosine-weighted diffuse samples, then GGX specular samples).
 *      pt [P,32] per-point record (layout in mc_shade.hip); mat5 [P,5] = metallic, roughness, albedo(3);
 *      tab_d [Dd,2] / tab_s [Ds,2] = fixed (azimuth, elevation) tables in [0,1] (field.py:741-749);
 *      slot[r] >= 0 -> miss row index, < 0 -> hit row index -(slot)-1. ---------------------------------------------------- */
int nero_mc_point_setup(const float* pts, const float* view, const float* normals, const float* mat5, const float* rand_d,
                        const float* rand_s, int P, float* pt, void* stream);
/* hit / miss split of the n = P*D secondary rays by `depth < 10` (NeROMaterialRenderer.trace, network/renderer.py:727; get_lights,
 * network/field.py:861-877): miss_idx / hit_idx = the ray ids in ascending order (what torch.nonzero yields), slot as above, counts int32 [2]
 * = (n_miss, n_hit) on the device; miss_idx / hit_idx need room for n entries each; tmp: nero_mc_split_tmp_ints(n) int32 of scratch. */
int nero_mc_split_tmp_ints(int n);
int nero_mc_split(const float* depth, int n, int* slot, int* miss_idx, int* hit_idx, int* counts, int* tmp, void* stream);
/* DEAD rays (round 6).  With geometry_type 'schlick' (the reference's default, field.py:702; the only one its configurations use) a direction
 * below the shading horizon has NoL = saturate(n.w) = 0, hence G = 0 and an estimator weight D G / (4 NoV p + 1e-5) of EXACTLY zero, with
 * zero derivatives (the clamp passes no gradient for n.w < 0): the ray contributes nothing to any output or gradient of shade_mixed
 * (field.py:950-1012), whatever it hits.  nero_mc_dead_rays: dead [P*D] bytes = 1 for the GGX-sampled rows with n.w < -1e-6 (0 everywhere for
 * geometry_type 1, whose weight at NoL = 0 is small but not zero).  nero_mc_split_dead: nero_mc_split with a third class -- flagged rays get
 * slot = INT_MIN and enter neither list (counts[0] + counts[1] = n - #dead); the estimator kernels read L = 0 for them; dead = NULL: nero_mc_split. */
int nero_mc_dead_rays(const float* pt, const float* dirs, int P, int Dd, int Ds, int geometry_type, unsigned char* dead, void* stream);
int nero_mc_split_dead(const float* depth, const unsigned char* dead, int n, int* slot, int* miss_idx, int* hit_idx, int* counts, int* tmp,
                       void* stream);

/* ---- Stage-II training glue (nero_amd/csrc/mat_loss.hip): what NeROMaterialRenderer.train_step does between the MLP / shading kernels,
 * as single launches.
 * nero_mat_reg_points: out [2P,3] = [pts ; pts + (cos(a) x + sin(a) y) eps], a = 2 pi ang01[p], (x, y) the tangent frame of
 *   get_orthogonal_directions (network/field.py:756-766, 1066-1076); eps [P] (change_type 'gaussian') or NULL -> eps_const.
 * nero_mat_head_fwd / _bwd: raw [n,5] -> (metallic, roughness in [0.04^2, 1], albedo[3]) = sigmoid heads of predict_materials
 *   (network/field.py:915-922) and their backward (d_raw from d_mat; raw is re-read, not the output).
 * nero_mat_loss_fwd: loss[0] = mean(loss_rgb) + mean(loss_mat_reg) + mean(loss_diffuse_light) (train/trainer.py:134-137 over
 *   network/renderer.py:837-844); loss[1..3] = the three means; rgb_pr [P,3] = linear_to_srgb(rgb_lin) (may be NULL).
 *   mat: [2P,5] when has_reg (rows P.. = the materials at the perturbed points), else [P,5]; partials: nero_mat_loss_partials(P) floats.
 *   hinge_weight: 0 = the reg_min_max hinge is off (step >= 2000), otherwise the weight of the hinge SUM (1 for one process; the
 *   data-parallel step passes world size).
 * nero_mat_loss_bwd: gradients of loss[0] * grad_out[0] (grad_out: device scalar, NULL = 1) -> d_mat (same shape as mat), d_rgb_lin, d_dl.
 * P == 0 (all five calls): NERO_OK, nothing launched, nothing written. */
typedef struct {
    int rgb_l1;                 /* 0: Charbonnier sqrt(sum d^2 + 1e-3) (default), 1: L1 */
    int reg_mat, reg_change;
    float reg_lambda1;
    float hinge_weight;
    int reg_diffuse;
    float reg_diffuse_lambda;
} nero_mat_loss_cfg;
int nero_mat_reg_points(int P, const float* pts, const float* normals, const float* ang01, const float* eps, float eps_const, float* out, void* stream);
int nero_mat_head_fwd(int n, const float* raw, float* mat, void* stream);
int nero_mat_head_bwd(int n, const float* raw, const float* d_mat, float* d_raw, void* stream);
int nero_mat_loss_partials(int P);
int nero_mat_loss_fwd(const nero_mat_loss_cfg* cfg, int P, int has_reg, const float* mat, const float* rgb_lin, const float* dl, const float* gt,
                      float* rgb_pr, float* partials, float* loss, void* stream);
int nero_mat_loss_bwd(const nero_mat_loss_cfg* cfg, int P, int has_reg, const float* mat, const float* rgb_lin, const float* dl, const float* gt,
                      const float* grad_out, float* d_mat, float* d_rgb_lin, float* d_dl, void* stream);
/* ---- Stage-I training glue (nero_amd/csrc/step_glue.hip): what NeROShapeRenderer.train_step / the trainer do BETWEEN the render calls,
 *      as a handful of launches and without a second host read-back.  Replaces, per step: near_far_from_sphere
 *      (network/renderer.py:231-238), the candidate subset of compute_occ_loss (network/renderer.py:528-541: mask -> nonzero ->
 *      random subset of occ_loss_max_pn), compute_rgb_loss + the means of loss_rgb / loss_eikonal / loss_occ and their sum
 *      (network/renderer.py:332-343, network/loss.py:8-55, train/trainer.py:127-137) and autograd's seeds for the render backward.
 * nero_occ_select: flag [n] (nero_occ_candidates) -> counts = (kept = min(total, cap), total); cand [cap] = the sample indices of the
 *   kept candidates in ascending order, -1 in unused slots.  Above the cap the kept ones are the `cap` smallest keys[ordinal]
 *   (ordinal = rank of the candidate among the candidates; ties to the lower ordinal): argsort(keys[:total], stable)[:cap], sorted.
 *   A candidate whose key is +inf ranks behind every finite key, by ordinal, and ahead of every sample that is no candidate.  A key
 *   that is a positive NaN ranks behind +inf and still ahead of the non-candidates, as in torch.argsort; -0.0 ties with +0.0.
 *   Nothing is read back: every launch covers the worst case n.  ws: nero_occ_select_workspace(n) bytes.
 * nero_occ_gather: pts / dirs [cap,3] = x4[cand, 0:3] / geo[cand, 4:7] (the reflected direction); unused slots: origin, +z.
 * nero_occ_l1: loss[0] = sum over the used slots k of |occ_prob[cand[k]] - gt[k]| / max(counts[0], 1) -- F.l1_loss(occ_prob[cand], gt) of
 *   network/renderer.py:546-547 on the fixed-capacity candidate list (one block, fixed summation tree); nero_occ_l1_backward: d_occ [n_in] =
 *   d_loss[0] * sign(occ_prob[cand[k]] - gt[k]) / max(counts[0], 1) at the kept candidates, zero elsewhere (sign(0) = 0 as in ATen).  For
 *   callers that assemble the loss themselves under autograd (the drop-in renderer); nero_shape_loss below holds the same term for the fused step.
 * nero_shape_loss: losses [4] = (total, mean loss_rgb, eik_weight * mean(gerr) * w[0], L1(occ_prob[cand], gt_occ) * w[1]);
 *   d_rgb [R,3], d_gerr [n_in], d_occ [n_in] (zero except at the kept candidates) = d total / d (ray_rgb, gradient_error, occ_prob).
 *   cand = NULL: no occlusion term (d_occ may be NULL).  weights: device [2] (data-parallel count weights) or NULL = (1, 1).
 *   partials: nero_shape_loss_partials(R, n_in) floats.
 * nero_var_grad: grad[0] = dsum[0] * 10 * inv_s * [1e-6 <= inv_s <= 1e6], inv_s = exp(10 variance[0])  (std_act 'exp'). */
enum { NERO_RGB_L2 = 0, NERO_RGB_L1 = 1, NERO_RGB_SMOOTH_L1 = 2, NERO_RGB_CHARBONIER = 3 };
int nero_near_far_sphere(const float* o, const float* d, int R, float* near, float* far, void* stream);
size_t nero_occ_select_workspace(int n);
int nero_occ_select(const unsigned char* flag, int n, const float* keys, int cap, int* cand, int* counts, void* ws, size_t ws_bytes,
                    void* stream);
int nero_occ_gather(const float* x4, const float* geo, const int* cand, int cap, float* pts, float* dirs, void* stream);
int nero_occ_l1(const float* occ_prob, const int* cand, const int* counts, const float* gt, int cap, float* loss, void* stream);
int nero_occ_l1_backward(const float* d_loss, const float* occ_prob, const int* cand, const int* counts, const float* gt, int cap, int n_in,
                         float* d_occ, void* stream);
int nero_shape_loss_partials(int R, int n_in);
int nero_shape_loss(int R, int rgb_kind, const float* rgb, const float* gt, int n_in, const float* gerr, float eik_weight,
                    const float* occ_prob, const int* cand, const int* counts, const float* gt_occ, const float* weights, float* losses,
                    float* d_rgb, float* d_gerr, float* d_occ, float* partials, void* stream);
int nero_var_grad(const float* dsum, const float* variance, float* grad, void* stream);
int nero_mc_dirs(const float* pt, const float* tab_d, const float* tab_s, int P, int Dd, int Ds, float* dirs, float* origins, void* stream);
/* sphere != 0 ('sphere_direction'): X [rows,144] = [IDE(w,0) | IDE(unit-sphere exit point,0)], else X [rows,72] */
int nero_mc_encode_miss(const float* dirs, const int* idx, const float* pt, int D, int sphere, int n, float* X, void* stream);
/* human-light input of the miss rows (get_human_light, network/field.py:820-834): Xh [rows,24], hmask [rows]; poses [P,3,4] */
int nero_mc_human_encode(const float* dirs, const int* idx, const float* pt, int D, const float* poses, int n, float* Xh, float* hmask,
                         void* stream);
int nero_mc_encode_hit(const float* dirs, const float* pos, const float* face_normals, const int* idx, int n, float* X /*[rows,128]*/,
                       void* stream);
/* human_raw [miss rows,4] / hmask [miss rows] may be NULL (shader_cfg.human_lights false).
 * geometry_type: 0 = 'schlick' (geometry_schlick, network/field.py:892-903), 1 = 'ggx_smith' (geometry_ggx_smith_correlated, :905-913) */
int nero_mc_combine_fwd(const float* pt, const float* dirs, const float* depth, const int* slot, const float* outer_raw,
                        const float* inner_raw, const float* human_raw, const float* hmask, float exp_max, float inner_exp_max, int P,
                        int Dd, int Ds, int geometry_type, float* rgb_lin, float* dl_mean, float* sl_mean, float* spec_lin /*or NULL*/,
                        void* stream);
int nero_mc_combine_bwd(const float* pt, const float* dirs, const float* depth, const int* slot, const float* outer_raw,
                        const float* inner_raw, const float* human_raw, const float* hmask, float exp_max, float inner_exp_max, int P,
                        int Dd, int Ds, int geometry_type, const float* d_rgb, const float* d_dl, float* d_outer_raw, float* d_inner_raw,
                        float* d_human_raw, float* d_mat5, float* d_wspec, void* stream);
int nero_mc_dir_bwd(const float* pt, const float* dirs, const float* face_normals, const int* slot, const float* tab_s,
                    const float* dX_miss, const float* dX_hit, const float* d_wspec, int P, int Dd, int Ds, float* d_mat5, int sphere,
                    const float* dXh /*or NULL*/, const float* poses /*[P,3,4] or NULL*/, void* stream);
/* Round 6: the photographer's light exists only where a ray reaches his region of the camera plane -- get_human_light multiplies the MLP's
 * output by that mask (field.py:819-829), so every other row of the human-light MLP is exactly dead.  nero_mc_human_flags: hum [P*D] bytes =
 * the mask per ray (hits & |0.3 inter_xy| < 1.5 & dist > 0).  nero_mc_split_classes: nero_mc_split_dead (dead may be NULL) with the miss
 * list PARTITIONED by `hum`: the misses with hum != 0 first (ray order), then the others (ray order); counts3 int32 [3] = (n_miss, n_hit, n_hum).
 * The human-light MLP then runs on the miss rows [0, n_hum); the _h entry points take n_hum and read human_raw / hmask / dXh / write d_human_raw
 * for those rows only (the plain entry points: for every miss row). */
int nero_mc_human_flags(const float* pt, const float* dirs, const float* poses, int P, int D, unsigned char* hum, void* stream);
int nero_mc_split_classes(const float* depth, const unsigned char* dead, const unsigned char* hum, int n, int* slot, int* miss_idx, int* hit_idx,
                          int* counts3, int* tmp, void* stream);
int nero_mc_combine_fwd_h(const float* pt, const float* dirs, const float* depth, const int* slot, const float* outer_raw,
                          const float* inner_raw, const float* human_raw, const float* hmask, int n_hum, float exp_max, float inner_exp_max, int P,
                          int Dd, int Ds, int geometry_type, float* rgb_lin, float* dl_mean, float* sl_mean, float* spec_lin /*or NULL*/,
                          void* stream);
int nero_mc_combine_bwd_h(const float* pt, const float* dirs, const float* depth, const int* slot, const float* outer_raw,
                          const float* inner_raw, const float* human_raw, const float* hmask, int n_hum, float exp_max, float inner_exp_max, int P,
                          int Dd, int Ds, int geometry_type, const float* d_rgb, const float* d_dl, float* d_outer_raw, float* d_inner_raw,
                          float* d_human_raw, float* d_mat5, float* d_wspec, void* stream);
int nero_mc_dir_bwd_h(const float* pt, const float* dirs, const float* face_normals, const int* slot, const float* tab_s,
                      const float* dX_miss, const float* dX_hit, const float* d_wspec, int P, int Dd, int Ds, float* d_mat5, int sphere,
                      const float* dXh /*or NULL*/, const float* poses /*[P,3,4] or NULL*/, int n_hum, void* stream);

/* ---- C-level driver of the Stage-I render step (nero_stage1_render_fwd / _bwd, nero_workspace_bytes) -------------------
 * One call each for sample_ray (network/renderer.py:403-443), render / render_core (:445-463, 550-606: the drop-in boundary) and
 * their backward incl. the second-order SDF term (autograd through SDFNetwork.gradient, network/field.py:155-167).  The calls
 * sequence the entry points above exactly as nero_amd/shape_step.py does (tests/test_stage1_driver.py: bit-for-bit equal), so a host in
 * any language runs the step without Python.  ALL memory is the caller's: one workspace (nero_stage1_workspace_bytes) from which every
 * intermediate is carved, one buffer for the packed operand images (nero_stage1_pack_bytes).  The only host synchronisation is the
 * read-back of the inner / outer sample counts inside nero_stage1_render_fwd (they size every later launch).
 * The fp16 two-plane engines only (gemm_* = NERO_GEMM_F16X3); NERO_ERR_UNSUPPORTED otherwise. */
#define NERO_S1_LINEARS 49
/* index of a Linear in nero_stage1_weights / _grads: sdf_network.lin0..8 = 0..8, outer_nerf.pts_linears.0..7 = 9..16, views_linears.0 = 17,
 * feature_linear = 18, alpha_linear = 19, rgb_linear = 20, then the predictors' four Linears each: metallic 21.., roughness 25.., albedo
 * 29.., outer_light 33.., inner_light 37.., inner_weight 41.., human_light_predictor 45.. (shader_config.human_light only). */
typedef struct { const float* W; const float* b; } nero_linear;        /* EFFECTIVE weight [n_out, k] row-major contiguous, bias [n_out] */
typedef struct { float* dW; float* db; } nero_linear_grad;              /* destinations shaped like W / b (overwritten)                   */
typedef struct { nero_linear lin[NERO_S1_LINEARS]; } nero_stage1_weights;
typedef struct { nero_linear_grad lin[NERO_S1_LINEARS]; } nero_stage1_grads;
typedef struct {
    int n_samples, n_importance, n_bg_samples, up_sample_steps, clip_sample_variance;   /* NeROShapeRenderer.default_cfg, renderer.py:84-95 */
    int human_light, sphere_direction;                                                  /* shader_config, network/field.py:487-495          */
    float light_exp_max;
    int gemm_fwd, gemm_tan, gemm_bwd, gemm_dw;                                           /* NERO_GEMM_*                                      */
} nero_stage1_cfg;
/* device pointers into the workspace, valid from nero_stage1_render_fwd until the next one (what the losses and the validation path read:
 * compute_occ_loss renderer.py:522-548 needs x4 / sdf4 / normal / geo / inner_idx, compute_validation_info :465-482 needs weights) */
typedef struct {
    int R, T, n_in, n_out;
    float* pts4;            /* [R*T,4] mid points + section lengths                       */
    int* ray_counts; int* ray_off; int* counts;
    int* inner_idx; int* outer_idx;
    float* x4;              /* [rows_pad(n_in),4] inner sample positions                  */
    float* sdf4;            /* [rows_pad(n_in),4] column 0 = sdf                          */
    float* feat;            /* [rows_pad(n_in),256]                                       */
    float* normal;          /* [n_in,3] SDF gradient                                      */
    float* geo;             /* [rows_pad(n_in),8] nhat, NoV, reflection, |grad|           */
    float* weights;         /* [R,T] compositing weights                                  */
} nero_stage1_state;
typedef struct nero_stage1 nero_stage1;

int nero_stage1_create(const nero_stage1_cfg* cfg, nero_stage1** out);
void nero_stage1_destroy(nero_stage1* h);
size_t nero_stage1_pack_bytes(nero_stage1* h);
/* (re)build the packed operand images of all ten networks from the effective weights: once per optimisation step */
int nero_stage1_pack(nero_stage1* h, const nero_stage1_weights* w, void* pack_buf, void* stream);
/* worst case over the data-dependent inner / outer split for R rays (sampler + forward + backward) */
size_t nero_stage1_workspace_bytes(nero_stage1* h, int R);
size_t nero_stage1_workspace_bytes_for(nero_stage1* h, int R, int n_in, int n_out, int with_sampler);
/* sampler + render forward only (inference chunks: no nero_stage1_render_bwd on this workspace), worst case over the split */
size_t nero_stage1_workspace_bytes_fwd(nero_stage1* h, int R);
/* z_vals [R, n_samples + n_importance + n_bg_samples]; rand1 [R] / rand_bg [R, n_bg] uniform draws or NULL (no perturbation) */
int nero_stage1_sample(nero_stage1* h, int R, const float* o, const float* d, const float* near, const float* far, const float* variance,
                       const float* rand1, const float* rand_bg, float* z_vals, void* ws, size_t ws_bytes, void* stream);
/* rgb [R,3]; gerr / occ_prob: capacity R*T floats, the first n_in entries are written (eikonal term, unclamped occ_prob);
 * n_in_out / n_out_out: host ints.  poses [R,3,4] human frames or NULL.  Keeps its state in `ws` for nero_stage1_render_bwd. */
int nero_stage1_render_fwd(nero_stage1* h, int R, const float* o, const float* d, const float* z_vals, const float* variance,
                           const float* lut, const float* poses, float anneal, float* rgb, float* gerr, float* occ_prob,
                           int* n_in_out, int* n_out_out, void* ws, size_t ws_bytes, void* stream);
/* d_rgb [R,3], d_gerr [n_in] or NULL, d_occ [n_in] or NULL -> every dW / db of `grads` (NULL entries are skipped);
 * d_inv_s_sum: device float receiving sum_k d L / d inv_s (the caller applies d inv_s / d variance), or NULL */
int nero_stage1_render_bwd(nero_stage1* h, const float* d_rgb, const float* d_gerr, const float* d_occ, const nero_stage1_grads* grads,
                           float* d_inv_s_sum, void* stream);
int nero_stage1_get_state(nero_stage1* h, nero_stage1_state* out);
/* no-grad SDF values of PE-6 rows [rows_pad(n),40] -> out4 [rows_pad(n),4], column 0 = sdf (sampler / occlusion march / mesh grid) */
int nero_stage1_sdf_from_pe(nero_stage1* h, const float* pe, int n, float* out4, void* ws, size_t ws_bytes, void* stream);
/* The occlusion-loss branch of a training step (compute_occ_loss, network/renderer.py:522-541 + get_intersection, network/field.py:454-484)
 * on the state of the last nero_stage1_render_fwd (n_in > 0), as one call: nero_occ_candidates, nero_occ_select, nero_occ_gather and the
 * march nero_occ_z -> PE -> SDF values of cap*sn0 rows -> nero_section_weights -> nero_sample_pdf -> PE -> SDF values of cap*sn1 rows ->
 * nero_section_weights, the launches nero_amd/shape_step.py::secondary_occlusion issues, in its order.
 *   d [R,3] and variance [1]: those of the forward.  keys [>= n_in] uniform draws (nero_occ_select).  thresh = occ_sdf_thresh.
 *   1 <= cap <= 4096, 2 <= sn0 <= 160, 1 <= sn1 <= 32.  cand int32 [cap], counts int32 [2] (nero_occ_select), occ [cap] = the marched
 *   occlusion probability of the kept candidates (unused slots: the march of the origin along +z).
 *   ws: nero_stage1_occlusion_workspace(h, n_in, cap, sn0, sn1) bytes of the caller's, NOT part of the step workspace.
 * Streams: the branch needs x4 / sdf4 / normal / geo / inner_idx only, which exist once nero_sdf_alpha_fwd of the forward has run, so it is
 * enqueued on `branch_stream` behind an event the forward records there, beside the shading networks, and `join_stream` (the stream of
 * nero_stage1_render_fwd and of whatever reads cand / counts / occ next) is made to wait for its end.  Work the caller queued on
 * branch_stream before the call (the key draw) stays in front of the branch.  branch_stream == join_stream, a one-stream handle
 * (NERO_STREAMS=1, no side stream) or nero_prof_enable: everything is enqueued on join_stream, behind branch_stream's earlier work. */
size_t nero_stage1_occlusion_workspace(nero_stage1* h, int n_in, int cap, int sn0, int sn1);
int nero_stage1_occlusion(nero_stage1* h, const float* d, const float* variance, const float* keys, float thresh, int cap, int sn0, int sn1,
                          int* cand, int* counts, float* occ, void* ws, size_t ws_bytes, void* branch_stream, void* join_stream);

/* ---- C-level driver of the Stage-II (material) shading step (nero_mc_shade_fwd / _bwd) -----------------------------------
 * predict_materials (network/field.py:915-922) and MCShadingNetwork.shade_mixed / get_lights (:856-880, 950-1012) with their backward, in
 * the call order of NeROMaterialRenderer.shade (network/renderer.py:810-813):
 *     nero_stage2_predict_fwd   raw material heads of the points (and of the regulariser's perturbed copies)
 *     nero_stage2_rays          tangent frames, cosine-weighted + GGX directions, secondary-ray origins p + 1e-5 w
 *     <the caller traces `origins, dirs` -- nero_bvh_trace, where the reference calls raytracing/raytracer.py:49 from field.py:860>
 *     nero_stage2_shade_fwd     hit / miss split, light MLPs on the compacted rows, microfacet estimator
 *     nero_stage2_shade_bwd, nero_stage2_predict_bwd   (autograd order: the shading first)
 * One caller-owned workspace for the whole step (opened by predict_fwd), one buffer for the packed operand images; the only host
 * synchronisation is the read-back of the (miss, hit) counts in shade_fwd.  fp16 two-plane engines only. */
#define NERO_S2_LINEARS 32
/* Linear index: feats_network.module0 / module1 Linears = 0..7, then the predictors' four each: metallic 8.., roughness 12.., albedo 16..,
 * outer_light 20.., inner_light 24.., human_light 28.. (shader_cfg.human_lights only) */
typedef struct { nero_linear lin[NERO_S2_LINEARS]; } nero_stage2_weights;
typedef struct { nero_linear_grad lin[NERO_S2_LINEARS]; } nero_stage2_grads;
typedef struct {
    int diffuse_sample_num, specular_sample_num, human_lights, sphere_direction;    /* MCShadingNetwork.default_cfg, network/field.py:695-712 */
    int geometry_type;                                                              /* 0 'schlick', 1 'ggx_smith'                             */
    float light_exp_max, inner_light_exp_max;
    int gemm_fwd, gemm_bwd, gemm_dw;
} nero_stage2_cfg;
typedef struct nero_stage2 nero_stage2;
int nero_stage2_create(const nero_stage2_cfg* cfg, nero_stage2** out);
void nero_stage2_destroy(nero_stage2* h);
size_t nero_stage2_pack_bytes(nero_stage2* h);
int nero_stage2_pack(nero_stage2* h, const nero_stage2_weights* w, void* pack_buf, void* stream);
/* n_pred rows through predict_materials (P points + their P perturbed copies when the smoothness regulariser is on), P shaded points:
 * worst case over the hit / miss split of the P * (Dd + Ds) light rays */
size_t nero_stage2_workspace_bytes(nero_stage2* h, int n_pred, int P);
/* x [n,3] -> raw5 [n,5] = pre-sigmoid (metallic, roughness, albedo rgb) */
int nero_stage2_predict_fwd(nero_stage2* h, const float* x, int n, float* raw5, void* ws, size_t ws_bytes, void* stream);
/* mat5 [P,5] = (metallic, roughness, albedo) after their activations; rand_d / rand_s [P] azimuth offsets or NULL; tab_d [Dd,2] / tab_s [Ds,2]
 * the fixed (azimuth, elevation) tables (field.py:741-749) -> origins, dirs [P*(Dd+Ds),3] (caller-owned, kept alive until shade_bwd) */
int nero_stage2_rays(nero_stage2* h, int P, const float* pts, const float* view, const float* normals, const float* mat5, const float* rand_d,
                     const float* rand_s, const float* tab_d, const float* tab_s, float* origins, float* dirs, void* stream);
/* the flags of the rays of the last nero_stage2_rays call whose estimator weight is exactly zero (nero_mc_dead_rays; device pointer, [P*D]
 * bytes, valid until the next nero_stage2_rays), for the caller's tracer (nero_bvh_trace_masked); NULL when nothing is skipped (geometry_type 1,
 * or NERO_MC_SKIP_DEAD=0 at nero_stage2_create).  nero_stage2_shade_fwd leaves the flagged rays out of both light MLPs whatever the tracer reported. */
const unsigned char* nero_stage2_dead_rays(nero_stage2* h);
/* rows of the last nero_stage2_shade_fwd: miss rows (outer light), hit rows (inner light), and how many of the miss rows own a row of the
 * human-light MLP (round 6: the rays that reach the photographer's region of the camera plane; 0 without human_lights).  Rays that are none of
 * these are the zero-weight rays nobody shades. */
int nero_stage2_counts(nero_stage2* h, int* n_miss, int* n_hit, int* n_hum);
/* pos / face_normals [P*D,3], depth [P*D] of the traced rays (depth >= 10 = miss; kept alive until shade_bwd); poses [P,3,4] or NULL
 * -> rgb (linear), mean diffuse light, mean weighted specular light, specular part: [P,3] each */
int nero_stage2_shade_fwd(nero_stage2* h, const float* pos, const float* face_normals, const float* depth, const float* poses, float* rgb,
                          float* dl, float* sl, float* sp, int* n_miss_out, int* n_hit_out, void* stream);
/* -> dW / db of the light MLPs (entries 20.. of `grads`), d_mat5 [P,5] */
int nero_stage2_shade_bwd(nero_stage2* h, const float* d_rgb, const float* d_dl, const nero_stage2_grads* grads, float* d_mat5, void* stream);
/* d_raw5 [n,5] -> dW / db of the feats network and the material predictors (entries 0..19) */
int nero_stage2_predict_bwd(nero_stage2* h, const float* d_raw5, const nero_stage2_grads* grads, void* stream);

/* ---- marching cubes: Stage-I SDF grid -> triangle mesh (nero_amd/csrc/mcubes.hip) -----------------------------------------------------
 * Replaces `vertices, triangles = mcubes.marching_cubes(u, threshold)` (PyMCubes, network/field.py:1110-1117, called from extract_mesh.py:24-31),
 * the step between Stage I and Stage II.
 *   u [nx][ny][nz] fp32, contiguous, z fastest (NeROShapeRenderer.extract_fields' layout); any nx, ny, nz >= 1 with nx*ny*nz < 2^32 (1024^3 is
 *   2^30).  A grid with fewer than 2 points on an axis has no cell: the empty mesh, NERO_OK.
 *   Inside: corner c is "below" when u < threshold (strict); cube index bit c = corner c below.  Corners (x,y,z index offsets) 0:(0,0,0)
 *   1:(1,0,0) 2:(1,1,0) 3:(0,1,0) 4:(0,0,1) 5:(1,0,1) 6:(1,1,1) 7:(0,1,1); edges 0:(0,1) 1:(1,2) 2:(2,3) 3:(3,0) 4:(4,5) 5:(5,6) 6:(6,7)
 *   7:(7,4) 8:(0,4) 9:(1,5) 10:(2,6) 11:(3,7); Paul Bourke's triangle table (nero_amd/csrc/mcubes_tables.h).
 *   Orientation: cross(v_b - v_a, v_c - v_a) of a triangle (a,b,c) points into u < threshold -- for an SDF, inward (the winding the reference's
 *   Stage II expects: NeROMaterialRenderer.trace flips the tracer's face normals, network/renderer.py:719-723).
 *   Vertices: one per grid edge whose endpoints straddle the threshold, float32 [V,3] in index space; the edge from point a to a + e_axis
 *   gives a + t e_axis, t = (threshold - u_a) / (u_b - u_a) in fp32, t in [0, 1].  Order: (linear index (i*ny + j)*nz + k of a, axis x<y<z).
 *   Triangles: int32 [T,3] vertex ids, ordered by (linear index of the cell's min corner, position in the table).  Fixed by prefix sums,
 *   not atomics: independent of the launch shape, bit-identical run to run.  NaN / inf in u: never a fault or a write out of range;
 *   such cells give some deterministic mesh.
 * nero_mcubes_workspace_bytes: the workspace both calls share: 5 bytes per grid point + 32 bytes per 2048 points + the scan's scratch
 *   (< 6 nx*ny*nz + 64 KiB; 256 bytes for a grid without cells; 0 for a grid the calls refuse).
 * nero_mcubes_count: -> totals [2] (device int64) = {V, T}, also kept in the workspace for nero_mcubes_emit.
 * nero_mcubes_emit: same u, sizes, threshold and workspace as the count before it -> verts [V,3], tris [T,3].  Before any launch it reads
 *   the 16-byte totals back from the workspace -- the one synchronisation of these calls, on `stream` -- and fails (nothing written) when
 *   V > v_cap or T > t_cap (NERO_ERR_ARG) or V or T >= 2^31 (NERO_ERR_UNSUPPORTED); every store is also bounded by v_cap / t_cap on the
 *   device. */
size_t nero_mcubes_workspace_bytes(int nx, int ny, int nz);
int nero_mcubes_count(const float* u, int nx, int ny, int nz, float threshold, void* ws, int64_t* totals /*device, {V, T}*/, void* stream);
int nero_mcubes_emit(const float* u, int nx, int ny, int nz, float threshold, void* ws, float* verts, int64_t v_cap, int* tris, int64_t t_cap,
                     void* stream);

/* ---- mesh clean-up: connected components of the extracted mesh and their removal (nero_amd/csrc/mesh_clean.hip) -------------------------
 * A marching-cubes surface of a learned SDF holds floaters, hidden inner shells and scraps of the support surface.  The reference has no
 * counterpart (its users delete them in a mesh editor); Stage II traces its secondary rays against whatever the mesh holds.  Host
 * counterpart: nero_amd/mesh.py.
 *   tris [T,3] int32 over V vertices, verts [V,3] fp32; 0 <= V, T < 2^31 (else NERO_ERR_UNSUPPORTED); V = 0 and T = 0 are valid and launch
 *   nothing over zero items.  Two vertices are connected when a triangle holds both.  Degenerate and duplicate triangles and non-manifold
 *   edges are ordinary input.  A triangle with an index outside [0, V) is skipped by every kernel and never dereferenced.
 *   No floating-point atomics, no atomics that decide a position or a label: every result is bit-identical run to run.
 * nero_mesh_cc_label -- label [V] = the smallest vertex index of the vertex's component (an unreferenced vertex is a component of its own).
 *   A concurrent union-find: label doubles as the parent array, every change of it is an agent-scope compare-and-swap or minimum, and a
 *   launch of its own flattens it; near-linear in V + T whatever the diameter of the mesh graph.  info [2] (device int64) = {K, the number
 *   of components; the number of skipped triangles}.  Never synchronises: the caller reads info.
 * nero_mesh_cc_stats -- label and K as nero_mesh_cc_label gave them -> comp [V] = the component of each vertex, numbered 0..K-1 in ascending
 *   order of the smallest vertex, and per component n_verts [K], n_faces [K] (a face belongs to the component of its first vertex), area [K]
 *   float64 (0.5 |(b - a) x (c - a)| in float64 from the fp32 vertices; the faces of a component, in ascending order, are cut into pieces of
 *   2048, a wave sums a piece and then the pieces: two fixed levels, the same bits every run), bbox_min / bbox_max [K,3] fp32 (exact; -0
 *   orders below +0).  Never synchronises.  ws: nero_mesh_cc_stats_workspace_bytes(V, T) (20 V + 16 T bytes + the sort's scratch).
 * nero_mesh_compact_count -- keep [K] bytes (non-zero = the component stays) -> totals [2] (device int64) = {V', T'}: the triangles of the
 *   kept components and the vertices they use (an unreferenced vertex is always dropped); also kept in the workspace.
 * nero_mesh_compact_emit -- same tris, sizes and workspace as the count before it -> verts_out [V',3], tris_out [T',3] in their original
 *   relative order with the indices remapped, vmap [V] (may be NULL) = the new index of each vertex or -1.  As nero_mcubes_emit it first
 *   reads the 16-byte totals back on `stream`, its one synchronisation, and fails with nothing written when V' > v_cap or T' > t_cap
 *   (NERO_ERR_ARG).  ws of both: nero_mesh_compact_workspace_bytes(V, T) (8 V + 8 T bytes + the scan's scratch). */
int nero_mesh_cc_label(const int* tris, int64_t T, int64_t V, int* label, int64_t* info /*device, {K, skipped}*/, void* stream);
size_t nero_mesh_cc_stats_workspace_bytes(int64_t V, int64_t T);
int nero_mesh_cc_stats(const float* verts, const int* tris, int64_t T, int64_t V, const int* label, int64_t K, void* ws, int* comp,
                       int* n_verts, int* n_faces, double* area, float* bbox_min, float* bbox_max, void* stream);
size_t nero_mesh_compact_workspace_bytes(int64_t V, int64_t T);
int nero_mesh_compact_count(const int* tris, int64_t T, int64_t V, const int* comp, const unsigned char* keep, int64_t K, void* ws,
                            int64_t* totals /*device, {V', T'}*/, void* stream);
int nero_mesh_compact_emit(const float* verts, const int* tris, int64_t T, int64_t V, void* ws, float* verts_out, int64_t v_cap, int* tris_out,
                           int64_t t_cap, int* vmap /*or NULL*/, void* stream);

/* ---- mesh simplification: vertex clustering with quadric-error placement (nero_amd/csrc/mesh_simplify.hip) ------------------------------
 * The mesh as dense as the extraction grid (a 512^3 grid: one to three million triangles) reduced to one vertex per occupied cell of a
 * uniform grid, directly behind the clean-up.  The definition is DESIGN.md's ("Mesh simplification"); tests/mesh_simplify_ref.py restates
 * it in numpy.  Host counterpart: nero_amd/mesh.py.
 *   verts [V,3] fp32, tris [T,3] int32; 0 <= V < 2^31 and 0 <= 3 T < 2^31 (else NERO_ERR_UNSUPPORTED); V = 0 and T = 0 are valid.
 *   cell > 0 and finite, origin [3] finite: HOST doubles (else NERO_ERR_ARG; NULL pointers likewise).  Cell of a vertex: i_a = floor((double(x_a)
 *   - origin_a) / cell) in IEEE float64, a true division; key = i_x << 42 | i_y << 21 | i_z.  A vertex that is non-finite or has an i_a outside
 *   [0, 2^21), and a triangle with an index outside [0, V), are counted and never followed.  A triangle survives when its three keys are
 *   pairwise different; the cells that hold a corner of a survivor are the output vertices, in ascending key order.
 *   No floating-point atomics and no atomics that decide a position: every output is bit-identical run to run.
 * nero_mesh_simplify_count -- totals [4] (device int32, 16 bytes) = {V', survivors (before de-duplication), refused vertices, refused
 *   triangles}, also kept in the workspace.  faces_only != 0: only the survivors are counted (no sort; V' = -1), for the search of a cell
 *   that meets a face budget; the workspace then does not serve nero_mesh_simplify_emit.  Never synchronises.
 * nero_mesh_simplify_emit -- same mesh, cell, origin and workspace as the complete count before it.  placement: NERO_SIMPLIFY_MEAN (the mean
 *   of the cell's vertices, referenced or not) or NERO_SIMPLIFY_QUADRIC (mean + (A + 1e-3 tr(A)/3 I)^-1 r over the 3T corner contributions
 *   with unnormalised normals, pivot-free LDL^T, clamped to the cell's closed box; the mean where tr(A) = 0).  Sums in float64, in a fixed
 *   order: vertices by ascending id, contributions by ascending 3 t + corner, cut into pieces of 2048 that a wave sums (lane-strided, then a
 *   butterfly) and adds in ascending order.  -> positions [V',3] float64, verts_out [V',3] = their fp32 rounding, cell_key [V'] int64;
 *   tris_out [T',3]: the survivors renumbered, winding and relative order kept; dedup != 0: of several survivors with the same unordered
 *   vertex set only the first stays.  n_tris (device int64, may be NULL) = T' <= survivors.  vmap [V] (may be NULL) = the output vertex of
 *   each vertex's cell or -1; fmap [T] (may be NULL) = the output index of each triangle or -1.  As nero_mesh_compact_emit it first reads
 *   the totals back on `stream`, its one synchronisation, and fails with nothing written when V' > v_cap or survivors > t_cap, or when the
 *   count refused a vertex or a triangle (NERO_ERR_ARG).
 * ws: nero_mesh_simplify_workspace_bytes(V, T): non-decreasing in V and in T (about 72 V + 136 T bytes + 4 MiB); 0 for sizes the calls
 *   refuse. */
enum { NERO_SIMPLIFY_MEAN = 0, NERO_SIMPLIFY_QUADRIC = 1 };
size_t nero_mesh_simplify_workspace_bytes(int64_t V, int64_t T);
int nero_mesh_simplify_count(const float* verts, const int* tris, int64_t T, int64_t V, double cell, const double* origin /*host [3]*/,
                             int faces_only, void* ws, int* totals /*device [4]*/, void* stream);
int nero_mesh_simplify_emit(const float* verts, const int* tris, int64_t T, int64_t V, double cell, const double* origin /*host [3]*/,
                            int placement, int dedup, void* ws, double* positions, float* verts_out, int64_t* cell_key, int64_t v_cap,
                            int* tris_out, int64_t t_cap, int* vmap /*or NULL*/, int* fmap /*or NULL*/, int64_t* n_tris /*device, or NULL*/,
                            void* stream);

/* ---- chart atlas: the UV unwrap of the Stage-II asset export (nero_amd/csrc/mesh_atlas.hip) ------------------------------------------------
 * The reference unwraps with xatlas (extract_materials_texture_map.py:83-85).  This is a PROJECTION atlas: charts are edge-connected sets of
 * faces whose normals share a dominant signed axis, each projected along that axis at one common world-to-texel scale, the chart rectangles
 * shelf-packed into the square map on the host.  The definition is DESIGN.md 9.7.1; tests/mesh_atlas_ref.py restates it in numpy.  Host
 * counterparts: nero_amd/mesh.py (face_adjacency_device, face_charts_device), nero_amd/texture.py (chart_atlas).
 *   verts [V,3] fp32, tris [T,3] int32; 0 <= V < 2^31 and 0 <= 3 T < 2^31 (else NERO_ERR_UNSUPPORTED); T = 0 and V = 0 are valid and launch
 *   nothing.  NULL pointers are NERO_ERR_ARG.  A face is VALID when its three indices lie in [0, V) and are pairwise different; any other
 *   face is chartless: counted, never dereferenced.  No floating-point atomics and no atomic that decides a position or a label: every
 *   output is bit-identical run to run.
 * nero_mesh_face_adjacency -- every valid face contributes the edges e = (v_e, v_(e+1)%3) with the key min << 32 | max; a stable radix sort of
 *   the (key, 3 t + e) pairs groups them.  A key held by exactly two entries, of two different faces, makes the two faces neighbours across
 *   that edge; a key held once is a boundary edge, three times or more a non-manifold edge: no neighbour.  -> nbr [T,3] int32 (-1 = none),
 *   counts [2] (device int64) = {boundary edges, non-manifold edges}.  Never synchronises.  ws: nero_mesh_face_adjacency_workspace_bytes(T)
 *   (72 T bytes + the sort's scratch).
 * nero_mesh_chart_label -- face_class [T] int32: n = (b - a) x (c - a) in float64 from the fp32 vertices (every product and difference rounded
 *   on its own), k = argmax |n_k| with ties to the lowest axis, class 2 k + (n_k < 0); 6 = chartless: a face that is not valid, or whose n
 *   is not finite or is zero.  Two faces belong to one chart when they are neighbours in nbr and have the same class below 6.  A concurrent
 *   union-find over the faces (chart doubles as the parent array; every change of it is an agent-scope compare-and-swap or minimum, the
 *   larger root goes under the smaller, a launch of its own flattens it).  -> chart [T] int32: charts numbered 0..K-1 in ascending order of
 *   their smallest face, -1 for a chartless face; info [2] (device int64) = {K, chartless faces}.  Never synchronises: the caller reads info.
 *   ws: nero_mesh_chart_label_workspace_bytes(T) (8 T bytes + the scan's scratch).
 * nero_mesh_chart_stats -- chart, face_class and K as nero_mesh_chart_label gave them -> per chart chart_class [K], n_faces [K] and box [K,4]
 *   fp32 = {min_p, min_q, max_p, max_q} of the projected coordinates of the chart's vertices, where class 2 k + s projects onto the axes
 *   p = (k + 1) % 3, q = (k + 2) % 3.  Exact: integer atomics on order-preserving bit images (-0 orders below +0).  Never synchronises.
 * nero_mesh_chart_corners_count / _emit -- the UV vertices: one per distinct (chart, mesh vertex) pair among the corners of charted faces, in
 *   ascending (chart, vertex) order (a stable sort of the 3T corner keys chart << 32 | vertex, head flags, a scan).  When a face is chartless
 *   one more UV vertex comes last and all three corners of every chartless face point at it.  count: totals [2] (device int64) = {n_vt,
 *   corners of chartless faces}, also kept in the workspace; never synchronises.  emit: same T and workspace as the count before it -> ft
 *   [T,3] int32, vt_vertex [n_vt] (the mesh vertex, -1 for the last one of a mesh with chartless faces: xatlas's vmapping), vt_chart [n_vt]
 *   (-1 likewise).  As nero_mesh_compact_emit it first reads the totals back on `stream`, its one synchronisation, and fails with nothing
 *   written when n_vt > vt_cap (NERO_ERR_ARG).  ws of both: nero_mesh_chart_corners_workspace_bytes(T) (96 T bytes + scratch).
 * nero_mesh_chart_uv -- origin [K,2] int32: the texel (ox, oy) of each chart's rectangle; scale: texels per world unit, a HOST double, finite
 *   and >= 0; size in [1, 16384] (else NERO_ERR_ARG).  For a UV vertex of chart c (class 2 k + s) at mesh vertex x:
 *   U = ox + 0.5 + (s ? max_p - x_p : x_p - min_p) * scale, V = oy + 0.5 + (x_q - min_q) * scale, vt = (U / size, V / size): float64, the
 *   difference, one product, the two sums left to right, one true division, each rounded on its own (no fused multiply-add), the result
 *   rounded once to fp32.  The mirror of the odd classes gives every UV triangle a positive area.  The vertex without a chart is (0, 0).  A
 *   call of its own, so that a search of the scale repeats no sort.  Never synchronises. */
size_t nero_mesh_face_adjacency_workspace_bytes(int64_t T);
int nero_mesh_face_adjacency(const int* tris, int64_t T, int64_t V, void* ws, int* nbr, int64_t* counts /*device, {boundary, non-manifold}*/,
                             void* stream);
size_t nero_mesh_chart_label_workspace_bytes(int64_t T);
int nero_mesh_chart_label(const float* verts, const int* tris, int64_t T, int64_t V, const int* nbr, void* ws, int* face_class, int* chart,
                          int64_t* info /*device, {K, chartless}*/, void* stream);
int nero_mesh_chart_stats(const float* verts, const int* tris, int64_t T, int64_t V, const int* chart, const int* face_class, int64_t K,
                          int* chart_class, int* n_faces, float* box, void* stream);
size_t nero_mesh_chart_corners_workspace_bytes(int64_t T);
int nero_mesh_chart_corners_count(const int* tris, int64_t T, int64_t V, const int* chart, int64_t K, void* ws,
                                  int64_t* totals /*device, {n_vt, chartless corners}*/, void* stream);
int nero_mesh_chart_corners_emit(int64_t T, void* ws, int* ft, int* vt_vertex, int* vt_chart, int64_t vt_cap, void* stream);
int nero_mesh_chart_uv(const float* verts, int64_t V, const int* vt_vertex, const int* vt_chart, int64_t n_vt, const int* chart_class,
                       const float* box, const int* origin, int64_t K, double scale /*host*/, int size, float* vt, void* stream);

/* ---- geometry evaluation: Chamfer distance of the extracted mesh (nero_amd/csrc/geom_eval.hip) --------------------------------------------
 * The reference's only geometry metric (eval_synthetic_shape.py, eval_real_shape.py, eval.md) without nvdiffrast / open3d / trimesh.  No
 * atomics decide a value or a position: every result is bit-identical run to run.  Host counterpart: nero_amd/eval_shape.py.
 *
 * nero_nn_dist -- `nearest_dist` (eval_synthetic_shape.py:16-25): exact brute-force nearest neighbour.  q [nq,3], r [nr,3] fp32;
 *   dist [nq] = sqrt(min_j d2(i,j)), d2 = fma(dz,dz, fma(dy,dy, dx*dx)) with dx = q_x - r_x ... formed first, all fp32 (within 4 * 2^-24 relative of
 *   the float64 distance of the same inputs); idx [nq] int32 or NULL = the j of the minimum, the lowest j among equal fp32 d2.  nq = 0: no-op;
 *   nr = 0: NERO_ERR_ARG; nr >= 2^31 with idx: NERO_ERR_UNSUPPORTED.  `splits`: over how many workgroups the reference set is divided (a second
 *   pass takes the minimum); 0 = chosen from the sizes (nero_nn_dist_splits) so that a 50 k x 50 k call fills 256 CUs; at most 4096.  The result
 *   does not depend on it.  ws: nero_nn_dist_workspace_bytes(nq, nr, splits) bytes (8 bytes per query and split; 0 = refused arguments).
 *
 * nero_voxel_downsample -- open3d `voxel_down_sample` (eval_synthetic_shape.py:79-82, dataset/database.py:451-456), whose output order is
 *   unspecified, made deterministic.  pts [n,3] fp32; origin o = min(pts) - voxel / 2 per axis; voxel index floor((p - o) / voxel) per axis in
 *   float64; the points are ordered by a stable radix sort of the key ix << 42 | iy << 21 | iz; out [n_out,3] = for each occupied voxel in
 *   ascending key order the float64 sum of its points in ascending input index, divided by their count, stored as fp32.  n_out: device int64 (may
 *   be NULL).  The call reads the count back on `stream` (its one synchronisation, as nero_mcubes_emit) before it writes: more voxels than
 *   out_cap is NERO_ERR_ARG with nothing written; a cloud spanning more than 2^21 voxels on an axis, or holding a non-finite coordinate, is
 *   NERO_ERR_UNSUPPORTED; n >= 2^31 - 1 likewise.  n = 0: n_out = 0.  ws: nero_voxel_downsample_workspace_bytes(n) (about 24 bytes per point +
 *   the sort's scratch).
 *
 * nero_view_rays -- primary rays of one view through the pixel centres (x + 0.5, y + 0.5): rays_o [h*w,3] = the camera centre -R^T t, rays_d
 *   [h*w,3] = normalised R^T inv(K) (x + 0.5, y + 0.5, 1), row-major pixels.  K [9], pose [12] = [R|t] world -> camera: HOST doubles, row-major.
 * nero_view_points -- t [h*w] = the hit distances nero_bvh_trace returns for those rays (`depth` output; a miss is 10) -> depth [h*w] fp32
 *   camera-space z = t * d_z / |d| for the pixel's inv(K) direction d (0 where missed), mask [h*w] bytes = t < 10, and pts = the masked pixels
 *   back-projected to the world exactly as mask_depth_to_pts + pose_inverse + pose_apply do (utils/base_utils.py:44-52, 562-565, 583-584): pixel
 *   coordinates and depth float32, (x + off) * z and (y + off) * z float32 products, then float64: (xz, yz, z) inv(K)^T R + c, stored fp32 in row-major
 *   pixel order at positions fixed by a prefix sum.  unproject_offset = 0 is the reference (integer pixel coordinates: a half-pixel quirk its
 *   ground-truth points share); 0.5 puts the points on the rays they were traced along.  n_pts: device int64, the number of masked pixels;
 *   no store past pts_cap points.  Together these stand in for rasterize_depth_map (eval_synthetic_shape.py:39-60).  DEVIATION: the depth is ray
 *   cast through pixel centres; nvdiffrast rasterises (screen-affine z, top-left fill rule), so boundary pixels and the depth inside a triangle
 *   can differ.  That difference is not measured: nvdiffrast is not available to this project.
 * nero_depth_points -- the same back-projection of a given depth map + mask (ground truth: database.get_depth, dataset/database.py:443-449).
 *   ws of both: nero_view_points_workspace_bytes(h, w). */
int nero_nn_dist_splits(int64_t nq, int64_t nr);
size_t nero_nn_dist_workspace_bytes(int64_t nq, int64_t nr, int splits);
int nero_nn_dist(const float* q, int64_t nq, const float* r, int64_t nr, void* ws, int splits, float* dist, int* idx /*or NULL*/, void* stream);
size_t nero_voxel_downsample_workspace_bytes(int64_t n);
int nero_voxel_downsample(const float* pts, int64_t n, double voxel, void* ws, float* out, int64_t out_cap, int64_t* n_out /*device*/,
                          void* stream);
int nero_view_rays(const double* K /*host [9]*/, const double* pose /*host [12]*/, int h, int w, float* rays_o, float* rays_d, void* stream);
size_t nero_view_points_workspace_bytes(int h, int w);
int nero_view_points(const float* t, const double* K /*host*/, const double* pose /*host*/, int h, int w, float unproject_offset, void* ws,
                     float* depth, unsigned char* mask, float* pts, int64_t pts_cap, int64_t* n_pts /*device*/, void* stream);
int nero_depth_points(const float* depth, const unsigned char* mask, const double* K /*host*/, const double* pose /*host*/, int h, int w,
                      float unproject_offset, void* ws, float* pts, int64_t pts_cap, int64_t* n_pts /*device*/, void* stream);

/* ---- texture baking: the Stage-II materials as UV maps (nero_amd/csrc/texture.hip) --------------------------------------------------------
 * The device steps of extract_materials_texture_map.py without nvdiffrast / scipy / sklearn / cv2 (the unwrapping: the chart atlas above, or any vt / ft of
 * the caller's, xatlas's for one).  Maps are row-major [h][w], texel (row y, column x) has index y w + x and its centre at u = (x + 0.5) / w,
 * v = (y + 0.5) / h; h and w in [1, 16384], anything else is NERO_ERR_ARG.  Host counterpart: nero_amd/texture.py.  No floating-point
 * atomics, no atomics that decide a position: every result is bit-identical run to run.
 *
 * nero_uv_raster -- `dr.rasterize(glctx, uv, ft, (h, w))` (extract_materials_texture_map.py:89-99) with a coverage rule of this project's own,
 *   exact integer arithmetic.  vt [nvt,2] fp32, ft [nt,3] int32 -> tri_id [h w] int32, -1 where uncovered.  A vertex snaps to
 *   X = rint(double(u) w 256), Y = rint(double(v) h 256) (int64); a texel centre is (256 x + 128, 256 y + 128).  A = (x1-x0)(y2-y0) -
 *   (x2-x0)(y1-y0); A == 0 covers nothing; A < 0 swaps vertices 1 and 2 (both windings are accepted).  For each directed edge a -> b,
 *   e = (bx-ax)(py-ay) - (by-ay)(px-ax); the texel is inside when for all three edges e > 0, or e == 0 and the edge owns its boundary: dy < 0,
 *   or dy == 0 and dx > 0.  Every centre of a triangulated region is covered exactly once.  Where triangles overlap the lowest index wins
 *   (an integer atomic minimum: independent of arrival order).  Vertices outside [0, 1] are legal and clipped by the texel loop bounds; a
 *   triangle with a vertex that is not finite or snaps beyond 2^30 in magnitude covers nothing.  An index of ft outside [0, nvt) is
 *   NERO_ERR_ARG with nothing written: one validation kernel whose flag is read back on `stream`, the call's one synchronisation.
 *   Work is binned by bounding-box size: boxes of at most 16 texel centres are finished by the lane that set the triangle up, the others are
 *   cut into blocks of 8 x 8 texels that a fixed grid of waves shares.  ws: nero_uv_raster_workspace_bytes(nt) (16 bytes per triangle + the
 *   scan's scratch; 0 = a refused count).
 * nero_uv_overlap_count -- count (device int64) = the texel centres that more than one triangle covers, by the same rule and the same walk as
 *   nero_uv_raster (an integer count per texel instead of the minimum), so an edge two triangles share never counts twice.  For any vt / ft,
 *   an external unwrapper's too; a triangle with an index outside [0, nvt) covers nothing.  Never synchronises.
 *   ws: nero_uv_overlap_count_workspace_bytes(nt, h, w) (the raster's workspace + 4 bytes per texel).
 * nero_uv_interp -- `dr.interpolate(v, rast, f)`, the mask and `xyzs[mask]` (:100-113).  attr [nv,C] fp32 with its own face array fa [nt,3]
 *   (the reference rasterises with the UV faces and interpolates with the position faces) -> the covered texels compacted in ascending
 *   row-major order: texel [n] int32, out [n,C] = (e0 a0 + e1 a1 + e2 a2) / A with e_k the edge function opposite vertex k at the centre,
 *   formed in float64 (products, then the two sums left to right, then the quotient) and rounded once to fp32; mask [h w] bytes (may be NULL)
 *   = covered; n_out: device int64 (may be NULL).  Positions come from a prefix sum.  The call reads the count back on `stream` before it
 *   writes: more covered texels than `cap`, or an index of ft / fa out of range, is NERO_ERR_ARG with nothing written.
 *   ws: nero_uv_interp_workspace_bytes(h, w) (8 bytes per texel + the scan's scratch).
 * nero_tex_quantize -- `feats[mask] = ...; linear_to_srgb; (feats * 255).astype(np.uint8)` (:127-133; utils/raw_utils.py:4-15).  feat [n,C]
 *   fp32 at the texels texel [n] (distinct) -> tex [h w, C] uint8, zero elsewhere: x clamped to [0, 1] (NaN -> 0), srgb in float64 (as the reference's
 *   numpy branch), times 255, truncated toward zero.  1 <= C <= 64.
 * nero_tex_regions -- `binary_dilation(mask, iterations=32)` minus the mask and the mask minus `binary_erosion(mask, iterations=3)` (:136-141;
 *   cross structuring element, border_value 0).  mask [h w] bytes (non-zero = covered) -> region [h w] bytes: 3 (to be filled) = uncovered
 *   and within city-block distance `pad` of a covered texel; 2 (search band) = covered and within city-block distance `border` of an
 *   uncovered texel, everything outside the image counting as uncovered; 1 = covered interior; 0 = nothing.  A row pass and a column pass
 *   over clamped byte distances.  pad in [0, 64], border in [1, 16], else NERO_ERR_ARG.  ws: nero_tex_regions_workspace_bytes(h, w) (one byte
 *   per texel).
 * nero_tex_fill -- the kd-tree query and the copy (:143-149), in place on tex [h w, C]: every region-3 texel takes the C bytes of the nearest
 *   region-2 texel among those within `pad` rows and `pad` columns of it: smallest integer squared Euclidean distance, ties to the lowest
 *   row-major index (sklearn leaves ties unspecified).  For regions made by nero_tex_regions with the same pad that window always holds the
 *   global nearest (the city-block-nearest covered texel is a chart-border texel at Euclidean distance <= pad).  A fill texel without a search
 *   texel in its window is left as it is.  src [h w] int32 (may be NULL) = the source index, -1 where nothing was filled.  Sources are never
 *   written and destinations never read, so in place is safe.  pad in [0, 64], 1 <= C <= 64.
 * nero_tex_downsample2 -- `cv2.resize(..., (w, h), INTER_LINEAR)` of a [2h, 2w, C] map (:157-160): out [h,w,C] = (a + b + c + d + 2) >> 2 over each
 *   2 x 2 block (cv2's rounding of ties is not verified: cv2 is not available to this project).  2h, 2w <= 16384. */
size_t nero_uv_raster_workspace_bytes(int64_t nt);
int nero_uv_raster(const float* vt, int64_t nvt, const int* ft, int64_t nt, int h, int w, void* ws, int* tri_id, void* stream);
size_t nero_uv_overlap_count_workspace_bytes(int64_t nt, int h, int w);
int nero_uv_overlap_count(const float* vt, int64_t nvt, const int* ft, int64_t nt, int h, int w, void* ws, int64_t* count /*device*/, void* stream);
size_t nero_uv_interp_workspace_bytes(int h, int w);
int nero_uv_interp(const int* tri_id, const float* vt, int64_t nvt, const int* ft, int64_t nt, const float* attr, int64_t nv, int C, const int* fa,
                   int h, int w, void* ws, int* texel, float* out, int64_t cap, unsigned char* mask /*or NULL*/, int64_t* n_out /*device, or NULL*/,
                   void* stream);
int nero_tex_quantize(const float* feat, const int* texel, int64_t n, int C, int h, int w, unsigned char* tex, void* stream);
size_t nero_tex_regions_workspace_bytes(int h, int w);
int nero_tex_regions(const unsigned char* mask, int h, int w, int pad, int border, void* ws, unsigned char* region, void* stream);
int nero_tex_fill(unsigned char* tex, const unsigned char* region, int h, int w, int C, int pad, int* src /*or NULL*/, void* stream);
int nero_tex_downsample2(const unsigned char* in, int h, int w, int C, unsigned char* out, void* stream);

/* ---- validation metrics: PSNR and SSIM of 8-bit images (nero_amd/csrc/image_metrics.hip) --------------------------------------------------
 * What ShapeRenderMetrics / MaterialRenderMetrics (network/metrics.py:39-102) compute per validation view, on images that stay on the device.
 * Host counterpart: nero_amd/metrics.py.  The calls never allocate and never synchronise; no atomics; every result is bit-identical run to
 * run and independent of what the workspace held before.
 *
 * nero_img_quantize -- color_map_backward, `np.clip(rgb * 255, 0, 255).astype(np.uint8)` (utils/base_utils.py:453-456).  in [n] fp32 -> out [n]
 *   uint8: one fp32 multiply by 255 (never contracted with anything), clamped to [0, 255], truncated towards zero.  +inf -> 255, -inf -> 0,
 *   NaN -> 0: numpy leaves the cast of NaN to uint8 undefined, so the value 0 is THIS PROJECT'S definition, not the reference's.  n = 0 is a
 *   no-op; n < 0 is NERO_ERR_ARG.
 * nero_img_metrics -- compute_psnr (network/metrics.py:11-17) and `structural_similarity(gt, pr, win_size=11, channel_axis=2, data_range=255)`
 *   (network/metrics.py:50, 85; skimage's defaults otherwise) of B image pairs.  gt, pr [B, h, w, C] uint8, row-major, channels interleaved ->
 *     sse [B] uint64 (may be NULL): the exact sum of squared differences over the h w C bytes of image b;
 *     ssim_c [B, C] fp64 (may be NULL): the SSIM of each channel;
 *     out [B, 2] fp64: {psnr, ssim}.  psnr = 10 log10(65025 / (sse / (h w C))), +inf when sse = 0 -- the exact value; the reference averages
 *       in float32 and is up to 2e-3 dB off it at 800 x 800.  ssim = the mean of ssim_c over the channels.
 *   SSIM per channel: uniform 11 x 11 window; with sx, sy, sxx, syy, sxy the window's sums of x, y, x^2, y^2, x y (exact integers),
 *     ux = sx / 121, uy = sy / 121, vx = (121 sxx - sx^2) / (121 * 120) (the sample covariance: skimage's 121 / 120 normalisation), vy and vxy
 *     likewise, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) in fp64;
 *     ssim_c = the mean of S over the (h - 10)(w - 10) window positions that lie wholly inside the image (skimage crops 5 pixels per side, so
 *     its filter's border mode never reaches the result).  This is this project's statement of skimage's algorithm: skimage itself is not
 *     available to it.
 *   The sums of S are added in a fixed order: per 32 x 32 tile of window positions (within a thread by rising row, a shuffle tree across the
 *     wave, the four waves in order), then the tiles of an image (thread t takes tiles t, t + 256, ... by rising index, then the same tree).
 *   Limits: B in [1, 65535], h and w in [11, 16384] (skimage raises for a window larger than the image), C in [1, 4]; anything else is
 *   NERO_ERR_ARG before any launch.  ws: nero_img_metrics_workspace_bytes(B, h, w, C) bytes, 8-byte aligned (40 bytes per tile and image;
 *   0 = a refused shape). */
int nero_img_quantize(const float* in, int64_t n, unsigned char* out, void* stream);
size_t nero_img_metrics_workspace_bytes(int64_t B, int h, int w, int C);
int nero_img_metrics(const unsigned char* gt, const unsigned char* pr, int64_t B, int h, int w, int C, void* ws, unsigned long long* sse /*or NULL*/,
                     double* ssim_c /*or NULL*/, double* out, void* stream);

/* ---- the learned environment light as a lat-long panorama (nero_amd/csrc/envlight.hip) ------------------------------------------------------
 * What MCShadingNetwork.env_light / get_env_light (network/field.py:1020-1059) compute, around the outer_light chain of the MLP engine.
 * Host counterpart: nero_amd/envlight.py.  The calls never allocate and never synchronise; every output is a function of the pixel (or row)
 * alone, so results are bit-identical run to run and for every split of a panorama into windows.
 *
 * nero_env_encode -- the direction grid (:1021-1034) and sph_enc(pts, 0) of predict_outer_lights_pts (:1049-1055) for the pixels
 *   first .. first + n - 1 (row-major) of an h x w panorama.  Pixel (row r, column c): az = linspace(1, 0, w)[c] 2 pi - pi / 2,
 *   el = linspace(1, -1, h)[r] pi / 2 (a one-element linspace is its start value), formed in fp64 on the device from the pixel index;
 *   d = (cos el cos az, cos el sin az, sin el) when is_real, else (cos el sin az, sin el, cos el cos az), rounded once to fp32.
 *   X [NERO_ROW_PAD(n), 72] = IDE(d, roughness) (generate_ide_fn(5), utils/ref_utils.py:85-117; roughness = kappa_inv, 0 in Stage II);
 *   sphere != 0: X [NERO_ROW_PAD(n), 144] = the same 72 columns twice ('sphere_direction').  Rows n .. NERO_ROW_PAD(n) - 1 are written as
 *   zero rows: the layout nero_mc_encode_miss gives the chain engine.  dirs [n, 3] (may be NULL) receives d.  X may be NULL when dirs is
 *   not (directions only).  On the z axis the reference's IDE is NaN (its complex power of 0); here it is the finite limit.
 *   h, w in [1, 16384], the window inside the panorama, roughness >= 0, else NERO_ERR_ARG.
 * nero_env_encode_dirs -- the same rows for n given directions src [n, 3] (get_env_light's light_pts, :1058-1059).
 * nero_env_finish -- raw [rows, 4] (the chain's head output, columns 0-2) -> rgb [n, 3] = exp(min(raw, exp_max)) (ExpActivation,
 *   network/field.py:301-307), then linear_to_srgb (utils/raw_utils.py:4-10) when gamma != 0.  No clamp to 1, as in the reference.
 * nero_env_rgbe -- Radiance RGBE of rgb [n, 3] fp32 -> out [n, 4] bytes: v = max(r, g, b) with negative channels counted as 0; v < 1e-32
 *   gives (0, 0, 0, 0); otherwise v = m 2^e with m in [0.5, 1), the colour bytes are trunc(c 2^(8 - e)) (an exact product: the scale is a power
 *   of two, nothing is divided) and the fourth byte is e + 128.  Decoding is byte 2^(E - 136).  v >= 2^127 (or not finite) saturates at
 *   e = 127 with bytes capped at 255; the host writer refuses such images.  n in [0, 2^30] for both. */
int nero_env_encode(int h, int w, int64_t first, int n, int is_real, int sphere, float roughness, float* X /*or NULL*/, float* dirs /*or NULL*/,
                    void* stream);
int nero_env_encode_dirs(const float* src, int n, int sphere, float roughness, float* X, void* stream);
int nero_env_finish(const float* raw, int64_t n, float exp_max, int gamma, float* rgb, void* stream);
int nero_env_rgbe(const float* rgb, int64_t n, unsigned char* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
