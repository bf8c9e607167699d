// mlp_f16_util.h -- device helpers of the fp16 two-plane chain kernels (mlp_f16x3.hip: one 512-thread workgroup per CU): block scaling, fp32 <-> fp16 plane pairs, the softplus (beta = 100) family,
// the three-product GEMM core.  Include inside an anonymous namespace.
#pragma once

// ---- phase timing (scripts/f16_variants.sh, -DF16_PHASE_TIMING): shader-clock cycles of wave 0 of every workgroup per phase ----
#ifdef F16_PHASE_TIMING
__device__ unsigned long long g_phase[16];
#define PH_DECL long long ph_t = clock64(), ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define PH(k) do { __builtin_amdgcn_sched_barrier(0); const long long t_ = clock64(); ph_acc[k] += t_ - ph_t; ph_t = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define PH_PARAM , long long& ph_t, long long (&ph_acc)[8]
#define PH_ARG , ph_t, ph_acc
#define PH_END do { if (threadIdx.x == 0) for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&g_phase[k_], (unsigned long long)ph_acc[k_]); } while (0)
#else
#define PH_PARAM
#define PH_ARG
#define PH_DECL
#define PH(k)
#define PH_END
#endif

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float BETA = 100.0f;
constexpr int SA = 528;                 // bytes per row of a main plane: 256 fp16 + 16 B pad
constexpr int PLANE_A = 64 * SA;
constexpr int SX_N = 112, SX_W = 208;   // aux plane row strides (48 / 96 columns + 16 B)
// ONE accumulator set (round 5; rounds 1-4 kept an H / L pair: docs/experiments.md, "Retired compile-time switches").  The block scale puts
// an operand's
// largest magnitude into [2^14, 2^15), the TOP of fp16's range, instead of [0.5, 1): the remainder l = fp16(xs - h) is then an ordinary
// fp16 number at its TRUE scale (|l| <= 2^3 for the largest elements, normal down to 2^-14, i.e. for every element within 2^-17 of the
// row maximum; below that its absolute error 2^-25 is 2^-40 of the maximum) -- no 2^11 pre-scale -- and the three plane products
// hw hx + hw lx + lw hx accumulate into the SAME fp32 accumulator inside the matrix pipe (what the weight-gradient GEMM has done since
// round 2, mlp_f16dw.hip).  Same three MFMAs per k-step; what goes away is the second accumulator set (32 VGPRs per wave), the
// H + 2^-11 L combine (32 VALU per lane and layer), the 2^11 multiply of every split (32 more) and half of the skip-layer rescale.
// Products reach 2^30, a 256-term sum 2^38: far inside fp32.  Error against fp64: tests/test_mlp_engine.py (unchanged tolerances).
constexpr int F16_TOP = 15;
constexpr int HDR_BYTES = 256;          // packed-image header: float[0] = 2^ew (the factor results are multiplied by), uint[1] = max bits
constexpr int SCR_LD = 36, SCR_BYTES = 32 * SCR_LD * 4;

// row-major workspace stores (saved activations, deltas, tangents: 1 KB per row and layer, written once, read by a LATER kernel)
// carry the non-temporal policy so that they do not displace the weight images -- re-read by every tile -- from the XCD's L2:
// -3.3 % on the whole training step (forward -2 %, reverse -4 %, tangent -4 %; docs/experiments.md).
// The mirror image on the read side (nt loads / nt LDS-DMA of those workspaces in the consumer kernels) LOSES 0.5-0.9 ms per step:
// much of what a pass wrote is still in the MALL when the next pass asks for it.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_ws4(float* dst, float4 v) {
    f32x4_t t = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(dst));
}

constexpr int SCRP_ROWS = 16;
constexpr int SCRP_BYTES = SCRP_ROWS * SCR_LD * 4;     // 2304 B per wave: store-transposition scratch, 16 rows at a time

// accumulator-layout 32x32 block -> row-major global store, 16 rows at a time through the wave-private scratch
__device__ __forceinline__ void acc_to_global16(float* scr, const float4 (&q)[4], float* __restrict__ gblock, int lane) {
    constexpr int ROWS = SCRP_ROWS;
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int p = 0; p < 32 / ROWS; ++p) {
        if (i / ROWS == p) {
#pragma unroll
            for (int g = 0; g < 4; ++g) *reinterpret_cast<float4*>(scr + (i % ROWS) * SCR_LD + 8 * g + 4 * h) = q[g];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int k = 0; k < ROWS / 8; ++k) {
            const int idx = lane + 64 * k, row = idx >> 3, c4 = 4 * (idx & 7);
            store_ws4(gblock + (size_t)(ROWS * p + row) * NERO_HID + c4, *reinterpret_cast<const float4*>(scr + row * SCR_LD + c4));
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- LDS-DMA ----------------------------------------------------------------------------------------------------------------
// global_load_lds_dwordx4: lane l's 16 bytes at `gptr` land at LDS byte address `lds_addr` + 16 l, no VGPRs in between.  Issued
// through inline asm on purpose: the compiler's wait-count pass otherwise puts a vmcnt(0) in front of EVERY later LDS access
// (it cannot prove the rest of the dynamic LDS array disjoint from the DMA target), which turns the prefetch into a stall.  Its
// vmcnt bookkeeping stays conservative (an untracked older load only makes counted waits longer); the reader must issue its own
// s_waitcnt vmcnt(0) before touching the target.
__device__ __forceinline__ void lds_dma16(const void* gptr, unsigned lds_addr) {
    // M0 = LDS base of the transfer.  It is handed over as a "{m0}"-constrained INPUT, so the compiler materialises the s_mov_b32 m0
    // itself and knows the register is live here (a clobber of m0 is ignored by hipcc: "reserved register").  The s_nop covers the
    // S_MOV-to-M0 -> LDS-DMA wait state, which hipcc's hazard recogniser cannot insert for an instruction inside an asm block.
    asm volatile("s_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(gptr), "{m0}"(lds_addr) : "memory");
}
__device__ __forceinline__ unsigned lds_offset_of(const void* p) { return (unsigned)(size_t)p; }      // generic -> LDS byte offset

// ---- scaling -----------------------------------------------------------------------------------------------------------
// exponent e with m * 2^-e in [0.5, 1) * 2^F16_TOP for normal m > 0 (-F16_TOP for m == 0 / denormal).  The exponent of m is taken from
// [2^-40, 2^100]: below, the block is scaled as if its maximum were 2^-40 (everything in it is then tiny but finite in the planes); the
// upper end keeps 2^e and 2^-e normal floats with room to spare (|e - F16_TOP| <= 115 < 126).  Rounds 1-5 clamped the exponent to +-40 BEFORE the shift by F16_TOP: with the
// one-accumulator format a block maximum beyond 2^40 would then have been scaled above 65504 and become fp16 infinity (the
// two-accumulator format stayed finite to 2^56).  No value of the training step comes near either end.
__device__ __forceinline__ int scale_exp(float m) {
    const int eb = (__float_as_uint(m) >> 23) & 0xff;
    int e = eb ? eb - 126 : 0;
    e = e < -40 ? -40 : (e > 100 ? 100 : e);
    return e - F16_TOP;                                  // (one accumulator: m * 2^-e in [2^14, 2^15), the top of fp16's range)
}
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }

// ---- fp32 <-> fp16 plane pairs -----------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pk_f16(float a, float b) {       // v_cvt_pk_f16_f32 (RN): a -> low half
    f32x2 v = {a, b};
    f16x2 c = __builtin_convertvector(v, f16x2);
    return __builtin_bit_cast(unsigned, c);
}
__device__ __forceinline__ void split2h(float a, float b, unsigned& h, unsigned& l) {     // a, b already block-scaled
    h = pk_f16(a, b);
    const f16x2 hh = __builtin_bit_cast(f16x2, h);
    l = pk_f16(a - (float)hh[0], b - (float)hh[1]);
}
__device__ __forceinline__ void store_planes4h(char* dst, int plane_bytes, float4 v) {
    unsigned h0, l0, h1, l1;
    split2h(v.x, v.y, h0, l0);
    split2h(v.z, v.w, h1, l1);
    *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(dst + plane_bytes) = make_uint2(l0, l1);
}
__device__ __forceinline__ float4 load_planes4h(const char* src, int plane_bytes) {       // -> block-scaled values
    const uint2 a = *reinterpret_cast<const uint2*>(src);
    const uint2 b = *reinterpret_cast<const uint2*>(src + plane_bytes);
    const f16x2 a0 = __builtin_bit_cast(f16x2, a.x), a1 = __builtin_bit_cast(f16x2, a.y);
    const f16x2 b0 = __builtin_bit_cast(f16x2, b.x), b1 = __builtin_bit_cast(f16x2, b.y);
    float4 v;
    v.x = (float)a0[0] + (float)b0[0];
    v.y = (float)a0[1] + (float)b0[1];
    v.z = (float)a1[0] + (float)b1[0];
    v.w = (float)a1[1] + (float)b1[1];
    return v;
}

// ---- activations ---------------------------------------------------------------------------------------------------------
// (NOT the code of mlp_split.hip / mlp_engine.hip: their softplus takes __expf / __logf with a log1p series for small arguments;
//  softplus100_grad_from_out is the same formula as theirs, on exp2)
// softplus(beta = 100) on the hardware exp2 / log2 units (v_exp_f32 / v_log_f32, ~1 ulp each, no range fix-ups needed here:
// the exp2 argument is <= 0 and the log2 argument lies in [1, 2]):   max(x, 0) + ln(1 + exp(-|100 x|)) / 100.
// Absolute error <= 1e-9 (the rounding of 1 + t), i.e. far below one fp32 ulp of the row maximum every value is block-scaled
// against.  Beyond 100 x > 20 the correction term is < 2e-11 and the sum rounds to x itself: torch's threshold rule
// (nn.Softplus(beta=100), network/field.py:124) without a branch.  8 VALU ops instead of ~30 (the epilogue is issue-bound).
__device__ __forceinline__ float softplus100(float x) {
    const float t = __builtin_amdgcn_exp2f(-fabsf(x) * 144.26950408889634f);
    const float l = __builtin_amdgcn_logf(1.0f + t);
    return fmaf(l, 0.0069314718055994531f, fmaxf(x, 0.f));
}
template <int ACT>
__device__ __forceinline__ float act_fwd(float x) {
    if (ACT == NERO_ACT_RELU) return fmaxf(x, 0.f);
    if (ACT == NERO_ACT_SOFTPLUS100) return softplus100(x);
    return x;
}

// sigma'(z) of softplus(beta = 100) from the SAVED OUTPUT a = softplus(z):  1 - exp(-100 a)  (= sigmoid(100 z)); a short series
// below 100 a = 1/32 keeps the relative accuracy where the subtraction would cancel; 1 beyond torch's threshold.
__device__ __forceinline__ float softplus100_grad_from_out(float a) {
    const float ba = BETA * a;
    const float ps = ba * (1.f + ba * (-0.5f + ba * (0.16666667f + ba * (-0.041666668f))));
    const float pe = 1.f - __builtin_amdgcn_exp2f(ba * -1.4426950408889634f);
    const float r = ba < 0.03125f ? ps : pe;
    return ba > 20.f ? 1.f : r;
}
template <int ACT>
__device__ __forceinline__ float act_grad(float a, float g) {
    if (ACT == NERO_ACT_RELU) return a > 0.f ? g : 0.f;
    if (ACT == NERO_ACT_SOFTPLUS100) return g * softplus100_grad_from_out(a);
    return g;
}
__device__ __forceinline__ void tan_elem(float a, float zd, float gb, bool live, float& ad, float& ij) {
    const float s = softplus100_grad_from_out(a);
    ad = s * zd;
    const float r2 = (BETA * a > 20.f) ? 0.f : BETA * (1.f - s);
    ij = live ? gb * r2 * zd : 0.f;
}
// the same injection from the tangent's OUTPUT: adot = s zdot  =>  inj = gbar * beta (1 - s) * adot / s   (s == 0: a == 0 exactly, then
// gbar = upstream * s is 0 too and the term vanishes; beyond torch's threshold sigma'' is 0)
__device__ __forceinline__ float inj_elem(float a, float gb, float ad) {
    const float s = softplus100_grad_from_out(a);
    const float r2 = (BETA * a > 20.f) ? 0.f : BETA * (1.f - s);
    return s > 0.f ? gb * r2 * (ad / s) : 0.f;
}
__device__ __forceinline__ float amax4(float4 v) { return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))); }
__device__ __forceinline__ float4 scale4(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }


// ---- chain descriptors and operand scales without dependent round trips (round 6) ------------------------------------------------------
// The layer descriptors live in the kernel-argument segment.  Read through a reference (`const nero_fwd_layer& L = ch.layer[l]`) every
// field became its own s_load + s_waitcnt lgkmcnt(0) at its point of use -- about ten scalar-cache round trips per layer, serial, on the
// critical path between two barriers -- and the block scale of a packed image (`*L.w_main`, a device-side value in the image header) a
// scalar load FOLLOWED BY a global load and a vmcnt(0) in front of the GEMM, which also drained the weight prefetch.  Now: the
// descriptor of a layer is copied by value in one batch of scalar loads (PIN_LAYER keeps hipcc from sinking the loads back to the uses),
// the NEXT layer's while the matrix pipe drains the current GEMM, and the scales of every image of the chain sit in a 20-entry LDS table
// filled once per workgroup (wsc[2 l] = main, wsc[2 l + 1] = aux image of layer l).
constexpr int WSC_N = 2 * NERO_MAX_LAYERS;
constexpr int LDS_SMALL_BYTES = (64 + 64 + 512 + 32) * 4;      // rs_main[64] rs_aux[64] rmax[64][8] wsc[<= 32]
#define PIN_S(x) asm volatile("" : "+s"(x))
// (pointers are pinned as INPUTS only: a pointer redefined by an asm statement loses its provenance and hipcc addresses through it with
//  flat_load / flat_store, which count on vmcnt AND lgkmcnt -- every LDS wait of the k-loop then waits for the weight stream as well)
#define PIN_P(x) asm volatile("" : : "s"(x))
__device__ __forceinline__ nero_fwd_layer load_layer(const nero_fwd_chain& ch, int l) {
    nero_fwd_layer L = ch.layer[l];
    PIN_P(L.w_main); PIN_P(L.w_aux); PIN_P(L.bias); PIN_P(L.save); PIN_P(L.head_w); PIN_P(L.head_b); PIN_P(L.head_out);
    PIN_S(L.k_main); PIN_S(L.k_aux); PIN_S(L.n_tiles); PIN_S(L.n_head); PIN_S(L.act); PIN_S(L.head_k); PIN_P(L.relu_mask);
    return L;
}
__device__ __forceinline__ nero_tan_layer load_layer(const nero_tan_chain& ch, int l) {
    nero_tan_layer L = ch.layer[l];
    PIN_P(L.w_main); PIN_P(L.w_aux); PIN_P(L.a_saved); PIN_P(L.gbar); PIN_P(L.adot); PIN_P(L.inj);
    PIN_S(L.k_main); PIN_S(L.k_aux); PIN_S(L.n_tiles);
    return L;
}
__device__ __forceinline__ nero_bwd_layer load_layer(const nero_bwd_chain& ch, int l) {
    nero_bwd_layer L = ch.layer[l];
    PIN_P(L.w_main_t); PIN_P(L.w_aux_t); PIN_P(L.a_prev); PIN_P(L.inj); PIN_P(L.delta_prev); PIN_P(L.head_w); PIN_P(L.head_dy);
    PIN_S(L.n_out); PIN_S(L.k_main_tiles); PIN_S(L.k_aux_tiles); PIN_S(L.n_head); PIN_S(L.act_prev); PIN_P(L.mask_prev); PIN_P(L.inj_adot);
    return L;
}
// request the scale of every packed image of the chain (uniform addresses; branch-free: a missing image reads the chain's first one) ...
struct WscRegs { float v[WSC_N]; };
template <class CH, class F> __device__ __forceinline__ void wsc_request(WscRegs& r, const CH& ch, F&& images) {
    const float* fb = nullptr;
#pragma unroll
    for (int l = NERO_MAX_LAYERS - 1; l >= 0; --l) {
        const float *pm, *pa;
        images(ch.layer[l], pm, pa);
        if (l < ch.n_layers) { fb = pa ? pa : fb; fb = pm ? pm : fb; }
    }
#pragma unroll
    for (int k = 0; k < WSC_N; ++k) r.v[k] = 1.f;
    if (fb == nullptr) return;
#pragma unroll
    for (int l = 0; l < NERO_MAX_LAYERS; ++l) {
        const float *pm, *pa;
        images(ch.layer[l], pm, pa);
        const bool in = l < ch.n_layers;
        pm = (in && pm) ? pm : fb;
        pa = (in && pa) ? pa : fb;
        r.v[2 * l] = *pm;
        r.v[2 * l + 1] = *pa;
    }
}
// ... and put them into the table (one lane; the caller's next barrier publishes it)
__device__ __forceinline__ void wsc_commit(float* wsc, const WscRegs& r, int tid) {
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < WSC_N; k += 4) *reinterpret_cast<float4*>(wsc + k) = make_float4(r.v[k], r.v[k + 1], r.v[k + 2], r.v[k + 3]);
    }
}

// ---- GEMM core ------------------------------------------------------------------------------------------------------------
// aH[r] += wl xh + wh xl + wh xh  over `n` k-steps of 16 (r = 32-row half).  Weight planes three steps ahead in a
// ring of four register sets (L2 stream), activation planes one step ahead in a double buffer (LDS).
struct WF { uint4 wh, wl; };
struct XF { uint4 xh0, xl0, xh1, xl1; };

__device__ __forceinline__ void load_w(WF& o, const uint4* wp, int c) {
    const uint4* w = wp + (size_t)c * 128;
    o.wh = w[0];
    o.wl = w[64];
}
__device__ __forceinline__ void load_x(XF& o, const char* xp, int half_bytes, int plane_bytes, int c) {
    const char* x = xp + c * 32;
    o.xh0 = *reinterpret_cast<const uint4*>(x);
    o.xl0 = *reinterpret_cast<const uint4*>(x + plane_bytes);
    x += half_bytes;
    o.xh1 = *reinterpret_cast<const uint4*>(x);
    o.xl1 = *reinterpret_cast<const uint4*>(x + plane_bytes);
}
#define NERO_MFH(ACC, A, B) \
    ACC = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), ACC, 0, 0, 0)
__device__ __forceinline__ void ops_compute(f32x16 (&aH)[2], const WF& w, const XF& x) {
    // (the two small products first: they enter an accumulator that still holds little; dependent MFMAs on one accumulator issue back
    //  to back at full rate -- accumulation forwarding, measured for the weight-gradient kernel in round 2)
    NERO_MFH(aH[0], w.wl, x.xh0); NERO_MFH(aH[1], w.wl, x.xh1);
    NERO_MFH(aH[0], w.wh, x.xl0); NERO_MFH(aH[1], w.wh, x.xl1);
    NERO_MFH(aH[0], w.wh, x.xh0); NERO_MFH(aH[1], w.wh, x.xh1);
}
#define NERO_FENCE() __builtin_amdgcn_sched_barrier(0)      // (without the fences hipcc sinks the prefetches: the kernels run 40 % slower)
// One k-step = 2 weight loads (VMEM) + 4 activation-fragment reads (DS) for a LATER step + 6 MFMAs of this step.  Issued as
// [6 loads][6 MFMAs] the wave spends the load-issue time with an idle matrix pipe and the MFMA time with idle issue slots (an in-order
// wave: a lone wave reaches 46 % of the pipe rate in the loop, two per SIMD 70 %, profiles/r03_phase_probes.txt).  The loads are NOT
// interleaved with the MFMAs (MFMA, DS, MFMA, DS, ..., MFMA, VMEM): measured slower in round 3 -- the GEMM phase of a layer-tile went from
// 8.6 k to 9.4 k cycles (forward), 4.7 k to 6.0 k (reverse), 17.6 k to 19.4 k (two workgroups per CU): a load between two MFMAs costs the
// pipe more than its issue slot (same file; docs/experiments.md).  Hence the fence between the requests and the MFMAs of every k-step.

// The first three weight fragments of a GEMM can be requested by the CALLER ahead of time (`pre`: wa, wb, wc already hold -- or are about
// to receive -- steps 0, 1, 2; see prefetch_w): a layer's first MFMA then waits for an LDS read instead of an L2 round trip behind
// the barrier that ends the previous layer (~900 cycles per layer-tile).
constexpr int F16_PW_N = 3;                          // fragments requested ahead by the caller (the rest at the start of the GEMM)
__device__ __forceinline__ void prefetch_w(WF& wa, WF& wb, WF& wc, const uint4* wp, int n, int from = 0) {
    const int last = n - 1;
    if (from <= 0) load_w(wa, wp, 0);
    if (from <= 1) load_w(wb, wp, 1 < last ? 1 : last);
    if (from <= 2) load_w(wc, wp, 2 < last ? 2 : last);
}
__device__ __forceinline__ void gemm_f16x3_loop(f32x16 (&aH)[2], const uint4* wp, const char* xp, int half_bytes,
                                           int plane_bytes, int n, bool pre, WF& wa, WF& wb, WF& wc) {
    if (n <= 0) return;
    WF wd;
    XF xa, xb;
    const int last = n - 1;
#define NERO_CL(c) ((c) < last ? (c) : last)
    prefetch_w(wa, wb, wc, wp, n, pre ? F16_PW_N : 0);
    load_x(xa, xp, half_bytes, plane_bytes, 0);
    NERO_FENCE();
    for (int c = 0; c < n; c += 4) {
        load_w(wd, wp, NERO_CL(c + 3)); load_x(xb, xp, half_bytes, plane_bytes, NERO_CL(c + 1)); NERO_FENCE();
        ops_compute(aH, wa, xa); NERO_FENCE();
        if (c + 1 < n) {
            load_w(wa, wp, NERO_CL(c + 4)); load_x(xa, xp, half_bytes, plane_bytes, NERO_CL(c + 2)); NERO_FENCE();
            ops_compute(aH, wb, xb); NERO_FENCE();
        }
        if (c + 2 < n) {
            load_w(wb, wp, NERO_CL(c + 5)); load_x(xb, xp, half_bytes, plane_bytes, NERO_CL(c + 3)); NERO_FENCE();
            ops_compute(aH, wc, xa); NERO_FENCE();
        }
        if (c + 3 < n) {
            load_w(wc, wp, NERO_CL(c + 6)); load_x(xa, xp, half_bytes, plane_bytes, NERO_CL(c + 4)); NERO_FENCE();
            ops_compute(aH, wd, xb); NERO_FENCE();
        }
    }
#undef NERO_CL
}
// the same without fragments requested ahead by the caller
__device__ __forceinline__ void gemm_f16x3(f32x16 (&aH)[2], const uint4* wp, const char* xp, int half_bytes, int plane_bytes, int n) {
    WF wa, wb, wc;
    gemm_f16x3_loop(aH, wp, xp, half_bytes, plane_bytes, n, false, wa, wb, wc);
}

// dual-tile k-loop of the paired kernels (mlp_f16p.hip): a wave that owns TWO feature tiles (weights wp0 / wp1) walks the k-steps
// once.  One k-step = four activation-fragment reads (shared by both tiles: the second tile's fragments are byte for byte the first's),
// four weight loads, twelve MFMAs -- half the LDS operand reads, trip count, wait counts and fences of two gemm_f16x3_loop passes, the
// same weight stream and MFMA count.  Every accumulator sees the products of ops_compute in the same order over ascending k, so the
// results are those of the single-tile loop bit for bit.  A k-step lasts twice as long, so the weight PAIRS are requested two steps ahead
// in a ring of three (48 registers; the single-tile loop: three steps ahead in a ring of four), the fragments one step ahead.
struct WF2 { WF a, b; };
__device__ __forceinline__ void load_w2(WF2& o, const uint4* wp0, const uint4* wp1, int c) {
    load_w(o.a, wp0, c);
    load_w(o.b, wp1, c);
}
__device__ __forceinline__ void ops_compute2(f32x16 (&aH0)[2], f32x16 (&aH1)[2], const WF2& w, const XF& x) {
    ops_compute(aH0, w.a, x);
    ops_compute(aH1, w.b, x);
}
__device__ __forceinline__ void gemm_f16x3_dual(f32x16 (&aH0)[2], f32x16 (&aH1)[2], const uint4* wp0,
                                                const uint4* wp1, const char* xp, int half_bytes, int plane_bytes, int n) {
    if (n <= 0) return;
    WF2 w0, w1, w2;
    XF xa, xb;
    const int last = n - 1;
#define NERO_CL(c) ((c) < last ? (c) : last)
#define NERO_K2(W, X) NERO_FENCE(); ops_compute2(aH0, aH1, W, X); NERO_FENCE()
    load_w2(w0, wp0, wp1, 0);
    load_w2(w1, wp0, wp1, NERO_CL(1));
    load_x(xa, xp, half_bytes, plane_bytes, 0);
    NERO_FENCE();
    for (int c = 0; c < n; c += 6) {
        load_w2(w2, wp0, wp1, NERO_CL(c + 2)); load_x(xb, xp, half_bytes, plane_bytes, NERO_CL(c + 1)); NERO_K2(w0, xa);
        if (c + 1 < n) { load_w2(w0, wp0, wp1, NERO_CL(c + 3)); load_x(xa, xp, half_bytes, plane_bytes, NERO_CL(c + 2)); NERO_K2(w1, xb); }
        if (c + 2 < n) { load_w2(w1, wp0, wp1, NERO_CL(c + 4)); load_x(xb, xp, half_bytes, plane_bytes, NERO_CL(c + 3)); NERO_K2(w2, xa); }
        if (c + 3 < n) { load_w2(w2, wp0, wp1, NERO_CL(c + 5)); load_x(xa, xp, half_bytes, plane_bytes, NERO_CL(c + 4)); NERO_K2(w0, xb); }
        if (c + 4 < n) { load_w2(w0, wp0, wp1, NERO_CL(c + 6)); load_x(xb, xp, half_bytes, plane_bytes, NERO_CL(c + 5)); NERO_K2(w1, xa); }
        if (c + 5 < n) { load_w2(w1, wp0, wp1, NERO_CL(c + 7)); load_x(xa, xp, half_bytes, plane_bytes, NERO_CL(c + 6)); NERO_K2(w2, xb); }
    }
#undef NERO_K2
#undef NERO_CL
}

// compile-time step count (the 256-wide layers: 16 steps), fully unrolled: no clamps, no branches, every ring slot a fixed register
// set.  XD = how many steps ahead the activation fragments are requested (ring of XD + 1 sets), weights three steps ahead.
template <int V> struct IC { static constexpr int value = V; };
template <int I, int N, class F> __device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(IC<I>{}); static_for<I + 1, N>(f); }
}
// `hook(IC<c>)` runs in every step behind that step's operand requests: the caller issues its own global loads at the step after
// which the GEMM requests no more weights (c = N - WD: vmcnt retires in order, a load issued earlier would hold the weight stream back,
// one issued later has less of the GEMM left to hide behind).
template <int N, class F>
__device__ __forceinline__ void gemm_f16x3_fixed_hook(f32x16 (&aH)[2], const uint4* wp, const char* xp, int half_bytes,
                                                      int plane_bytes, F&& hook) {
    constexpr int XD = 1, XN = XD + 1, WD = 3, WN = WD + 1;
    WF w[WN];
    XF x[XN];
    static_for<0, WD>([&](auto c) { if (c.value < N) load_w(w[c.value], wp, c.value); });
    static_for<0, XD>([&](auto c) { if (c.value < N) load_x(x[c.value], xp, half_bytes, plane_bytes, c.value); });
    NERO_FENCE();
    static_for<0, N>([&](auto cc) {
        constexpr int c = cc.value;
        if (c + WD < N) load_w(w[(c + WD) % WN], wp, c + WD);
        if (c + XD < N) load_x(x[(c + XD) % XN], xp, half_bytes, plane_bytes, c + XD);
        hook(cc);
        NERO_FENCE();
        ops_compute(aH, w[c % WN], x[c % XN]);
        NERO_FENCE();
    });
}
template <int N>
__device__ __forceinline__ void gemm_f16x3_fixed(f32x16 (&aH)[2], const uint4* wp, const char* xp, int half_bytes,
                                                 int plane_bytes) {
    gemm_f16x3_fixed_hook<N>(aH, wp, xp, half_bytes, plane_bytes, [](auto) {});
}

// ---- dual-tile k-loop with a compile-time step count and a weight ring the CALLER can prefill (paired kernels, 256-wide layers) ----
// What gemm_f16x3_dual loses: (1) hipcc forms the address of a ring slot's next request in the registers of that slot's pending
// request, so three of its six k-steps open with s_waitcnt vmcnt(0) -- the ring is drained before it is refilled and a weight pair is
// in flight for less than one k-step instead of two; (2) a layer's first requests are issued behind the row stores of the previous
// layer's epilogue, and vmcnt retires in order: the first k-steps wait until 16 HBM-bound stores are acknowledged.
// Here the weight requests are inline asm -- the compiler neither counts nor waits for them -- with a uniform base in scalar registers
// (no per-lane address arithmetic), and every wait is a counted s_waitcnt vmcnt(N) placed by hand:
//   N = the vector-memory requests issued AFTER the awaited slot's = 4 per later ring request (+ the epilogue's row stores where the
//   slot was requested ahead of them).  A larger true count only makes the wait conservative; a smaller one would be a race, so every
//   request of the ring is an asm volatile statement (program order among them is fixed) and the count is written next to each wait.
// Every destination register stays live from its request to the statement behind its wait that names it (landed_w2q): no request is
// issued whose result is not consumed (no clamped tail requests), so the compiler can never reuse a register a request is still going
// to write.  What it MAY do is copy such a register early -- check the ISA after a change here: between a request and its wait no
// instruction may name the slot's registers (done for this version: none does, in the loop or across the layer boundary).
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
struct WQ2 { u32x4 ah, al, bh, bl; };                 // one k-step's weight planes (h, l) of the wave's tiles a = t and b = t + NW
constexpr int WQ_STEP_BYTES = 2048, WQ_PLANE_BYTES = 1024;      // load_w: step c at wp + 128 c (uint4), wl 64 uint4 behind wh
// k-step C of both tiles -> slot o.  voff = 16 * lane, s0 / s1 = the tiles' first fragment (wave-uniform).  (s_nop 4: an SGPR the
// compiler has just formed -> VMEM address operand inside an asm block, which its hazard recogniser does not see into)
template <int C, bool ORDER_MEM>
__device__ __forceinline__ void load_w2q(WQ2& o, unsigned voff, const char* s0, const char* s1) {
    const char* p0 = s0 + C * WQ_STEP_BYTES;
    const char* p1 = s1 + C * WQ_STEP_BYTES;
#define NERO_W2Q_ASM "s_nop 4\n\tglobal_load_dwordx4 %0, %4, %5\n\tglobal_load_dwordx4 %1, %4, %5 offset:1024\n\t" \
                     "global_load_dwordx4 %2, %4, %6\n\tglobal_load_dwordx4 %3, %4, %6 offset:1024"
    // ORDER_MEM (the prefill): no store of the epilogue may be moved in front of the requests -- the prefilled waits count them
    if (ORDER_MEM) asm volatile(NERO_W2Q_ASM : "=&v"(o.ah), "=&v"(o.al), "=&v"(o.bh), "=&v"(o.bl) : "v"(voff), "s"(p0), "s"(p1) : "memory");
    else asm volatile(NERO_W2Q_ASM : "=&v"(o.ah), "=&v"(o.al), "=&v"(o.bh), "=&v"(o.bl) : "v"(voff), "s"(p0), "s"(p1));
#undef NERO_W2Q_ASM
}
static_assert(WQ_PLANE_BYTES == 1024, "offset:1024 in load_w2q");
// the wait and, behind it, the point from which the slot may be read.  Two statements on purpose: with the registers named on the wait
// itself hipcc may copy them IN FRONT of it (seen with one such wait in each arm of a branch) -- a copy of registers whose data has not
// landed.  The scheduling fence keeps every such copy behind the wait; nothing below `landed_w2q` reads the slot above it.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" : : "n"(N)); }
__device__ __forceinline__ void landed_w2q(WQ2& w) {
    NERO_FENCE();
    asm volatile("" : "+v"(w.ah), "+v"(w.al), "+v"(w.bh), "+v"(w.bl));
}
__device__ __forceinline__ void ops_compute2q(f32x16 (&aH0)[2], f32x16 (&aH1)[2], const WQ2& w, const XF& x) {   // = ops_compute2
    NERO_MFH(aH0[0], w.al, x.xh0); NERO_MFH(aH0[1], w.al, x.xh1);
    NERO_MFH(aH0[0], w.ah, x.xl0); NERO_MFH(aH0[1], w.ah, x.xl1);
    NERO_MFH(aH0[0], w.ah, x.xh0); NERO_MFH(aH0[1], w.ah, x.xh1);
    NERO_MFH(aH1[0], w.bl, x.xh0); NERO_MFH(aH1[1], w.bl, x.xh1);
    NERO_MFH(aH1[0], w.bh, x.xl0); NERO_MFH(aH1[1], w.bh, x.xl1);
    NERO_MFH(aH1[0], w.bh, x.xh0); NERO_MFH(aH1[1], w.bh, x.xh1);
}
// the caller's prefill: k-steps 0 and 1 of a LATER GEMM into r0 / r1, issued in front of the epilogue's row stores
__device__ __forceinline__ void prefill_w2q(WQ2& r0, WQ2& r1, unsigned voff, const char* s0, const char* s1) {
    load_w2q<0, true>(r0, voff, s0, s1);
    load_w2q<1, true>(r1, voff, s0, s1);
    NERO_FENCE();
}
// r0 / r1 were requested by prefill_w2q; `stores_behind`: at least PRE_STORES vector-memory requests (the row stores of the epilogue
// in between) were issued behind them.  Same products in the same order as gemm_f16x3_dual: bit-identical.
constexpr int PRE_STORES = 2 * 2 * (32 / SCRP_ROWS) * (SCRP_ROWS / 8);    // 2 tiles x 2 row halves x acc_to_global16's store_ws4 calls = 16
template <int N>
__device__ __forceinline__ void gemm_f16x3_dual_fixed(f32x16 (&aH0)[2], f32x16 (&aH1)[2], unsigned voff, const char* s0, const char* s1,
                                                      const char* xp, int half_bytes, int plane_bytes, WQ2& r0, WQ2& r1, bool stores_behind) {
    static_assert(N >= 3, "ring of three");
    WQ2 r2;
    XF x[2];
    load_x(x[0], xp, half_bytes, plane_bytes, 0);
    NERO_FENCE();
    static_for<0, N>([&](auto cc) {
        constexpr int c = cc.value;
        auto slot = [&](auto k) -> WQ2& { if constexpr (k.value % 3 == 0) return r0; else if constexpr (k.value % 3 == 1) return r1; else return r2; };
        if constexpr (c + 2 < N) load_w2q<c + 2, false>(slot(IC<c + 2>{}), voff, s0, s1);
        if constexpr (c + 1 < N) load_x(x[(c + 1) & 1], xp, half_bytes, plane_bytes, c + 1);
        NERO_FENCE();
        // requests issued behind slot c's: k-step c + 1's (by the prefill for c = 0, by step c - 1 otherwise) and k-step c + 2's (just
        // now), four each, where those steps exist; slots 0 and 1 also have the epilogue's PRE_STORES row stores behind them, which
        // therefore stay in flight under these MFMAs
        constexpr int later = 4 * ((c + 1 < N ? 1 : 0) + (c + 2 < N ? 1 : 0));
        if (c < 2 && stores_behind) wait_vm<later + PRE_STORES>();
        else wait_vm<later>();
        landed_w2q(slot(cc));
        ops_compute2q(aH0, aH1, slot(cc), x[c & 1]);
        NERO_FENCE();
    });
}

// the single-tile k-loop on the same terms (the reverse walk of the paired kernels: one feature tile at a time): weights three steps
// ahead in a ring of four asm-requested slots, two requests per k-step, counted waits.  gemm_f16x3's compiler-managed ring is drained
// by a vmcnt(0) at the head of every fourth k-step (the same address-in-destination pattern as the dual loop).  Same products in the
// same order as gemm_f16x3 / ops_compute: bit-identical.
struct WQ1 { u32x4 h, l; };
template <int C> __device__ __forceinline__ void load_w1q(WQ1& o, unsigned voff, const char* s) {
    const char* p = s + C * WQ_STEP_BYTES;
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %2, %3\n\tglobal_load_dwordx4 %1, %2, %3 offset:1024"
                 : "=&v"(o.h), "=&v"(o.l) : "v"(voff), "s"(p));
}
__device__ __forceinline__ void landed_w1q(WQ1& w) {
    NERO_FENCE();
    asm volatile("" : "+v"(w.h), "+v"(w.l));
}
template <int N>
__device__ __forceinline__ void gemm_f16x3_single_fixed(f32x16 (&aH)[2], unsigned voff, const char* s, const char* xp, int half_bytes,
                                                        int plane_bytes) {
    constexpr int WD = 3, WN = WD + 1;
    static_assert(N > WD, "ring of four");
    WQ1 w[WN];
    XF x[2];
    static_for<0, WD>([&](auto cc) { load_w1q<cc.value>(w[cc.value], voff, s); });
    load_x(x[0], xp, half_bytes, plane_bytes, 0);
    NERO_FENCE();
    static_for<0, N>([&](auto cc) {
        constexpr int c = cc.value;
        if constexpr (c + WD < N) load_w1q<c + WD>(w[(c + WD) % WN], voff, s);
        if constexpr (c + 1 < N) load_x(x[(c + 1) & 1], xp, half_bytes, plane_bytes, c + 1);
        NERO_FENCE();
        // requests issued behind k-step c's: those of k-steps c + 1, c + 2, c + 3 where they exist, two each
        constexpr int later = 2 * ((c + 1 < N ? 1 : 0) + (c + 2 < N ? 1 : 0) + (c + 3 < N ? 1 : 0));
        wait_vm<later>();
        landed_w1q(w[c % WN]);
        NERO_MFH(aH[0], w[c % WN].l, x[c & 1].xh0); NERO_MFH(aH[1], w[c % WN].l, x[c & 1].xh1);
        NERO_MFH(aH[0], w[c % WN].h, x[c & 1].xl0); NERO_MFH(aH[1], w[c % WN].h, x[c & 1].xl1);
        NERO_MFH(aH[0], w[c % WN].h, x[c & 1].xh0); NERO_MFH(aH[1], w[c % WN].h, x[c & 1].xh1);
        NERO_FENCE();
    });
}

__device__ __forceinline__ void zero2(f32x16 (&acc)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[r][v] = 0.f;
}

// bias + activation of one accumulator set in the unit U -> val, and the row maxima of the result (forward epilogue of both organisations)
template <int ACT>
__device__ __forceinline__ void fwd_values(const f32x16 (&aH)[2], const float4 (&bq)[4], const float (&U)[2], float4 (&val)[2][4],
                                           float (&m)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        m[r] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v;
            v.x = act_fwd<ACT>(fmaf(aH[r][4 * g], U[r], bq[g].x));
            v.y = act_fwd<ACT>(fmaf(aH[r][4 * g + 1], U[r], bq[g].y));
            v.z = act_fwd<ACT>(fmaf(aH[r][4 * g + 2], U[r], bq[g].z));
            v.w = act_fwd<ACT>(fmaf(aH[r][4 * g + 3], U[r], bq[g].w));
            val[r][g] = v;
            m[r] = fmaxf(m[r], amax4(v));
        }
    }
}

// ---- lane exchanges without the LDS (round 6) ---------------------------------------------------------------------------------
// __shfl_xor compiles to ds_bpermute_b32 + a bounds select + s_waitcnt lgkmcnt: an LDS round trip (~100+ cycles, and lgkmcnt is shared
// with the scalar loads) per exchange, several of them on the critical path of every layer epilogue.  gfx950 has the exchange of the two
// 32-lane halves as ONE VALU instruction (v_permlane32_swap) and the exchanges inside a row of 16 as DPP modifiers.
// v_permlane32_swap vdst, src0: vdst[32..63] <-> src0[0..31].  With both operands = v: r[0] = v's lower half in both halves, r[1] = its
// upper half in both halves.
__device__ __forceinline__ float max_xor32(float m) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ unsigned other_half(unsigned v, int h) {          // the value lane ^ 32 holds
    const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return h ? r[0] : r[1];
}
// DPP: quad_perm [1,0,3,2] = 0xB1 (lane ^ 1), quad_perm [2,3,0,1] = 0x4E (lane ^ 2), row_half_mirror = 0x141 (lane j <-> 7 - j of each
// group of 8: the OTHER quad, which is all a reduction over 8 lanes needs once every lane holds its quad's result)
template <int CTRL> __device__ __forceinline__ float dpp_f32(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float max_4lanes(float m) { m = fmaxf(m, dpp_f32<0xB1>(m)); return fmaxf(m, dpp_f32<0x4E>(m)); }
__device__ __forceinline__ float max_8lanes(float m) { m = max_4lanes(m); return fmaxf(m, dpp_f32<0x141>(m)); }
// (same bits as the shuffle butterfly: every step adds the partner's partial sum to the lane's own, and fp32 addition commutes)
__device__ __forceinline__ float sum_8lanes(float s) { s += dpp_f32<0xB1>(s); s += dpp_f32<0x4E>(s); return s + dpp_f32<0x141>(s); }

// row maxima of this wave's 64x32 block (two rows per lane) -> rmax[row][wave]
__device__ __forceinline__ void publish_rowmax(float* rmax, float m0, float m1, int wave, int i, int h) {
    m0 = max_xor32(m0);
    m1 = max_xor32(m1);
    if (h == 0) { rmax[i * 8 + wave] = m0; rmax[(32 + i) * 8 + wave] = m1; }
}
__device__ __forceinline__ float row_max8(const float* rmax, int row) {
    const float4 a = *reinterpret_cast<const float4*>(rmax + row * 8);
    const float4 b = *reinterpret_cast<const float4*>(rmax + row * 8 + 4);
    return fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
}

// ---- epilogue of a reverse layer (shared by mlp_f16x3.hip and mlp_f16p.hip) ---------------------------------------------------------
// PRE: the injections were requested inside the GEMM (ijp, bwd_f16_kernel<true>); otherwise they are read here
template <int ACT, bool HEAD, bool PRE>
__device__ __forceinline__ void bwd_values(const float4 (&gq)[2][4], const float4 (&pa)[2][4], size_t goff, bool has_inj,
                                           const nero_bwd_layer& L, int row0, int i, int fbase, int n_rows, float4 (&val)[2][4],
                                           float (&m)[2], const float4 (&ijp)[2][4]) {
    // the global operands of the epilogue are requested in branch-free batches ahead of their use: with the loads inside
    // `if (has_inj)` / `if (j < nh)` hipcc waited for each of them separately (147 of the reverse kernel's 240 loads were followed by
    // s_waitcnt vmcnt(0)) -- eight serial HBM round trips per layer-tile for the injections of the second-order pass, up to 32 serial
    // L2 round trips for the head weights of a chain's first step.  Now: four head-weight rows per request group, and the four
    // injection vectors of a row half together (both halves at once costs 32 more registers: 255 + spills).
    const int nh = L.n_head;
    float4 gs[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int g = 0; g < 4; ++g) gs[r][g] = gq[r][g];
    if (HEAD) {
        float dj[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const float4 dyh = *reinterpret_cast<const float4*>(L.head_dy + (size_t)(row0 + 32 * r + i) * 4);
            dj[r][0] = dyh.x; dj[r][1] = dyh.y; dj[r][2] = dyh.z; dj[r][3] = dyh.w;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 hw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) hw[j] = *reinterpret_cast<const float4*>(L.head_w + (j < nh ? j : 0) * NERO_HID + fbase + 8 * g);
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nh) {
                        gs[r][g].x = fmaf(dj[r][j], hw[j].x, gs[r][g].x); gs[r][g].y = fmaf(dj[r][j], hw[j].y, gs[r][g].y);
                        gs[r][g].z = fmaf(dj[r][j], hw[j].z, gs[r][g].z); gs[r][g].w = fmaf(dj[r][j], hw[j].w, gs[r][g].w);
                    }
            __builtin_amdgcn_sched_barrier(0);         // (one request group at a time: all sixteen hoisted cost 40 registers and spills)
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const bool live = (row0 + 32 * r + i) < n_rows;
        float4 ij[4];
        if (PRE) {
#pragma unroll
            for (int g = 0; g < 4; ++g) ij[g] = ijp[r][g];
        } else if (has_inj) {
#pragma unroll
            for (int g = 0; g < 4; ++g) ij[g] = *reinterpret_cast<const float4*>(L.inj + goff + (size_t)r * 32 * NERO_HID + 8 * g);
            if (ACT == NERO_ACT_SOFTPLUS100 && L.inj_adot) {
                // `inj` is gbar and inj_adot the tangent: the sigma'' injection gbar beta (1 - s) zdot with zdot = adot / s is formed here
                // (s = sigma'(a_prev) is in hand anyway), so the tangent pass neither reads gbar nor writes a finished term
                float4 ad[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) ad[g] = *reinterpret_cast<const float4*>(L.inj_adot + goff + (size_t)r * 32 * NERO_HID + 8 * g);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 a = pa[r][g];
                    ij[g].x = inj_elem(a.x, ij[g].x, ad[g].x); ij[g].y = inj_elem(a.y, ij[g].y, ad[g].y);
                    ij[g].z = inj_elem(a.z, ij[g].z, ad[g].z); ij[g].w = inj_elem(a.w, ij[g].w, ad[g].w);
                }
            }
        }
        m[r] = 0.f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 a = pa[r][g];
            float4 d;
            d.x = act_grad<ACT>(a.x, gs[r][g].x); d.y = act_grad<ACT>(a.y, gs[r][g].y);
            d.z = act_grad<ACT>(a.z, gs[r][g].z); d.w = act_grad<ACT>(a.w, gs[r][g].w);
            if (has_inj) { d.x += ij[g].x; d.y += ij[g].y; d.z += ij[g].z; d.w += ij[g].w; }
            if (!live) d = make_float4(0.f, 0.f, 0.f, 0.f);
            val[r][g] = d;
            m[r] = fmaxf(m[r], amax4(d));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int ACT, bool PRE>
__device__ __forceinline__ void bwd_values_h(const float4 (&gq)[2][4], const float4 (&pa)[2][4], size_t goff, bool has_inj,
                                             const nero_bwd_layer& L, int row0, int i, int fbase, int n_rows, float4 (&val)[2][4],
                                             float (&m)[2], const float4 (&ijp)[2][4]) {
    if (L.n_head > 0) bwd_values<ACT, true, PRE>(gq, pa, goff, has_inj, L, row0, i, fbase, n_rows, val, m, ijp);
    else bwd_values<ACT, false, PRE>(gq, pa, goff, has_inj, L, row0, i, fbase, n_rows, val, m, ijp);
}

