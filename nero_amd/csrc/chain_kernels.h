// chain_kernels.h -- the four small kernels the step drivers launch themselves, beside the host-side planner of chain_host.h (which
// holds no device code and comes along with this header).  Include once per translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include "chain_host.h"
#include "common.h"

namespace {

// x8[r] = (x4[r][0..2], 0, 0, 0, 0, 0) over all n_pad rows of the padded buffer (as x8[:, :3] = x4[:, :3])
__global__ void x8_from_x4_kernel(const float* __restrict__ x4, float* __restrict__ x8, int /*n*/, int n_pad) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pad) return;
    const float4 v = reinterpret_cast<const float4*>(x4)[r];
    reinterpret_cast<float4*>(x8)[2 * r] = make_float4(v.x, v.y, v.z, 0.f);
    reinterpret_cast<float4*>(x8)[2 * r + 1] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__global__ void ones_col0_kernel(float* __restrict__ b, int n_pad) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_pad) reinterpret_cast<float4*>(b)[r] = make_float4(1.f, 0.f, 0.f, 0.f);
}
// dst[r*ldd + c] = src[r*lds + c]
__global__ void copy2d_kernel(const float* __restrict__ src, int lds, float* __restrict__ dst, int ldd, int rows, int cols) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cols) return;
    const int r = idx / cols, c = idx - r * cols;
    dst[(size_t)r * ldd + c] = src[(size_t)r * lds + c];
}
// out[b] = sum of block b's grid-stride share of v[0..n) (deterministic two-stage reduction: 128 partials, then one block over them)
__global__ __launch_bounds__(256) void sum_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
    __shared__ float part[256];
    float s = 0.f;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) s += v[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

}  // namespace
