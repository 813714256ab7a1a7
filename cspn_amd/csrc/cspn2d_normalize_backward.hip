// cspn2d_normalize_backward.hip -- the adjoint of normalize2d_kernel (cspn2d_stepwise.hip): what torch autograd computes through the
// reference's affinity_normalization (cspn_pytorch/models/cspn.py:85-144), cropped to the image, for a given dL/dgate_wb.  It chains the
// gradient CSPN_NORM_PRENORM's backward returns into the raw guidance, the same chain bwd_final_kernel
// (cspn2d_backward.hip) evaluates inside the raw route.  Notation of that file's header, g~ = g or |g| ('8sum_abs'):
//   G_k(p) = g~_k(p + off_k) (0 outside the image),  S(p) = sum_j |G_j(p)|,  T(p) = sum_j R_j(p) G_j(p),  R = dL/dgate_wb (consumer-sited)
//   dL/dg_k(p + off_k) = ( R_k(p) / S(p) - sign(G_k(p)) T(p) / S(p)^2 )  [ * sign(g_k(p + off_k)) for '8sum_abs' ]
// Elements no pixel reads get 0.  One thread per pixel p: it gathers the eight G_k(p) and reads R(p) (16 loads, L2 serves the shifted
// re-reads), writes its eight gradients to the neighbour-sited elements and zeroes those of its own elements no pixel reads -- every output
// element is written exactly once (no atomics, no workspace: deterministic).  96 B/pixel of algorithmic traffic.  IEEE division
// throughout: S = 0 gives NaN at the pixels that read it, as torch does.
#include "cspn_common.h"

namespace cspn {

namespace {

__global__ __launch_bounds__(256) void normalize2d_backward_kernel(const float* __restrict__ g, const float* __restrict__ gwb,
                                                                    float* __restrict__ gg, int B, int H, int W, int norm) {
    const size_t HW = (size_t)H * W, total = (size_t)B * HW;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int b = (int)(idx / HW);
    const int r = (int)(idx - (size_t)b * HW);
    const int y = r / W, x = r - y * W;
    const float* gb = g + (size_t)b * 8 * HW;
    const float* rb = gwb + (size_t)b * 8 * HW;
    float* ob = gg + (size_t)b * 8 * HW;
    float G[8], raw[8], R[8], S = 0.f;
    bool ok[8];
    size_t noff[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int yy = y + dy2(k), xx = x + dx2(k);
        ok[k] = yy >= 0 && yy < H && xx >= 0 && xx < W;
        noff[k] = ok[k] ? (size_t)yy * W + xx : 0;
        const float v = ok[k] ? gb[k * HW + noff[k]] : 0.f;
        raw[k] = v;
        G[k] = norm == CSPN_NORM_8SUM_ABS ? fabsf(v) : v;
        S += fabsf(G[k]);
    }
    float T = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        R[k] = rb[k * HW + r];
        T = fmaf(R[k], G[k], T);
    }
    // g_k(q) with q - off_k outside the image is read by no pixel (the gather sees the zero padding instead): gradient 0
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int ys = y - dy2(k), xs = x - dx2(k);
        if (ys < 0 || ys >= H || xs < 0 || xs >= W) ob[k * HW + r] = 0.f;
    }
    const float t2 = T / (S * S);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!ok[k]) continue;  // the zero padding is a constant
        const float sg = G[k] > 0.f ? 1.f : (G[k] < 0.f ? -1.f : 0.f);
        float d = R[k] / S - sg * t2;
        if (norm == CSPN_NORM_8SUM_ABS) d *= raw[k] > 0.f ? 1.f : (raw[k] < 0.f ? -1.f : 0.f);
        ob[k * HW + noff[k]] = d;  // g_k(p + off_k) is read by pixel p only
    }
}

}  // namespace

int normalize2d_backward(const float* g, const float* gwb, float* gg, int B, int H, int W, int norm, hipStream_t st) {
    const size_t total = (size_t)B * H * W;
    hipLaunchKernelGGL(normalize2d_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, gwb, gg, B, H, W, norm);
    return check_launch("normalize2d_backward_kernel");
}

}  // namespace cspn
