// device_prims.h -- wave and workgroup reductions, the order-preserving float image and the concurrent union-find shared by the mesh
// kernels (mesh_clean, mesh_simplify, mesh_atlas, bvh_build, geom_eval, mcubes, texture), and the fixed-order float tree sum of the loss
// kernels (mat_loss, step_glue).  Wavefronts are 64 lanes (gfx950).
#pragma once
#include <hip/hip_runtime.h>

namespace nero_prims {

__device__ __forceinline__ bool in_range(int a, int n) { return (unsigned)a < (unsigned)n; }

// the counter hash of include/nero_hip_visibility.h (the AO rotations, the surface sampler's variates): a bijection of the 32-bit integers
__device__ __forceinline__ unsigned lowbias32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// order-preserving image of a float in the unsigned integers (-0 orders below +0)
__device__ __forceinline__ unsigned f2o(float f) {
    const unsigned b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float o2f(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// ---- butterflies over the 64 lanes: every lane ends with the result -----------------------------------------------------------------------
__device__ __forceinline__ unsigned wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = (unsigned)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
// (64 bits: the bit pattern of a non-negative double orders as the double does)
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
// the float pair is fminf / fmaxf, not a comparison: a NaN lane does not spread
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// (a float64 sum in this fixed order is the same bits every run)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum of v over the THREADS lanes of the workgroup, in every lane; part: THREADS / 64 shared words.  Ends with a barrier, so `part` may be
// reused by the next call.
template <int THREADS>
__device__ __forceinline__ int block_sum(int v, int* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    int tot = 0;
#pragma unroll
    for (int q = 0; q < THREADS / 64; ++q) tot += part[q];
    __syncthreads();
    return tot;
}

// float sum of v over the THREADS threads of the workgroup as a binary tree in LDS, in every thread; sh: THREADS shared floats.  Not an
// overload of block_sum: it pairs thread t with t + THREADS / 2, t + THREADS / 4, ..., an order of its own that the loss values are pinned
// to (the same bits every run, whatever the scheduling).  Ends with a barrier, so `sh` may be reused by the next call.
template <int THREADS>
__device__ __forceinline__ float block_tree_sum(float v, float* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// One atomic per wave and group, not per lane: a surface with floaters is one component that holds nearly every vertex, and per-lane
// atomics would queue on its few words.  Of the lanes in `todo` (wave-uniform), those that hold the group `c` of the first one (*leader,
// its group *cl); every lane of the wave must call this.
__device__ __forceinline__ unsigned long long next_group(int c, unsigned long long todo, int* cl, int* leader) {
    *leader = __ffsll((long long)todo) - 1;
    *cl = __shfl(c, *leader, 64);
    return __ballot(c == *cl) & todo;
}

// ---- concurrent union-find ----------------------------------------------------------------------------------------------------------------
// parent[v] = v at the start; uf_unite hooks the roots of its two elements, the larger root under the smaller, so parent[v] <= v always
// holds, a tree's root is its smallest element, and the forest cannot hold a cycle.  The XCDs' L2 caches are not coherent inside a launch,
// so every change of parent[] is an agent-scope atomic: the hook is a compare-and-swap parent[hi]: hi -> lo (it succeeds only while hi is
// still a root; when it fails it returned hi's parent, and the search goes on from there), the path compression an atomic minimum with an
// ancestor.  Plain loads of parent[] may be stale: a stale value is an OLDER ancestor pointer (entries only ever decrease, and an ancestor
// stays an ancestor), so it costs steps and decides nothing.  The roots are the smallest element of each set whatever order the atomics
// landed in; a caller flattens the trees in a second launch, behind the kernel boundary.

// some ancestor r of v with (a possibly stale) parent[r] == r; every element passed on the way is pointed at its grandparent
__device__ __forceinline__ int uf_find(int* parent, int v) {
    int p = parent[v];
    while (p != v) {
        const int g = parent[p];
        if (g != p) __hip_atomic_fetch_min(parent + v, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = p;
        p = g;
    }
    return v;
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;                                          // one element reached from both: one tree
        int hi = a > b ? a : b;
        const int lo = a > b ? b : a;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        a = seen;                                                    // hi had been hooked already: go on from its parent
        b = lo;
    }
}

}  // namespace nero_prims
