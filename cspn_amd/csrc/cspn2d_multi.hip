// cspn2d_multi.hip -- the two small kernels of the multi-channel 2D entry points (cspn2d_*_multi, include/cspn_amd.h): C channels of
// blur_depth on shared guidance (reference cspn_pytorch/models/cspn.py:58-81 broadcasts the affinities over the channels).
#include "cspn_common.h"

namespace cspn {
namespace {

// a mask shared by the C channels, [B][HW] -> [B][C][HW] (the ring reads the mask of image-channel b*C + c like its blur plane)
__global__ __launch_bounds__(256) void widen_channels_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, size_t HW, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // element of dst
    if (i >= n) return;
    const size_t r = i % HW, bc = i / HW;
    dst[i] = src[(bc / (size_t)C) * HW + r];
}

__global__ __launch_bounds__(256) void add_inplace_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

}  // namespace

int widen_channels(const float* src, float* dst, int B, int C, size_t HW, hipStream_t st) {
    const size_t n = (size_t)B * C * HW;
    hipLaunchKernelGGL(widen_channels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, dst, C, HW, n);
    return check_launch("widen_channels_kernel");
}

int add_inplace(float* dst, const float* src, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(add_inplace_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, src, n);
    return check_launch("add_inplace_kernel");
}

}  // namespace cspn
