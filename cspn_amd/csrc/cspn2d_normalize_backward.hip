// cspn2d_normalize_backward.hip -- the adjoint of normalize2d_kernel (cspn2d_stepwise.hip): what torch autograd computes through the
// reference's affinity_normalization (cspn_pytorch/models/cspn.py:85-144), cropped to the image, for a given dL/dgate_wb.  It chains the
// gradient CSPN_NORM_PRENORM's backward returns into the raw guidance; bwd_final_kernel (cspn2d_backward.hip) ends the raw
// route with the same helper (norm_adjoint2, cspn2d_pixel.h).  Notation of that file's header, g~ = g or |g| ('8sum_abs'):
//   G_k(p) = g~_k(p + off_k) (0 outside the image),  S(p) = sum_j |G_j(p)|,  T(p) = sum_j R_j(p) G_j(p),  R = dL/dgate_wb (consumer-sited)
//   dL/dg_k(p + off_k) = ( R_k(p) / S(p) - sign(G_k(p)) T(p) / S(p)^2 )  [ * sign(g_k(p + off_k)) for '8sum_abs' ]
// Elements no pixel reads get 0.  One thread per pixel p: it gathers the eight G_k(p) and reads R(p) (16 loads, L2 serves the shifted
// re-reads), writes its eight gradients to the neighbour-sited elements and zeroes those of its own elements no pixel reads -- every output
// element is written exactly once (no atomics, no workspace: deterministic).  96 B/pixel of algorithmic traffic.  IEEE division
// throughout: S = 0 gives NaN at the pixels that read it, as torch does.
#include "cspn2d_pixel.h"

namespace cspn {

namespace {

__global__ __launch_bounds__(256) void normalize2d_backward_kernel(const float* __restrict__ g, const float* __restrict__ gwb,
                                                                    float* __restrict__ gg, int B, int H, int W, int norm) {
    const size_t HW = (size_t)H * W;
    const Pixel p(B, H, W);
    if (!p.ok) return;
    const float* rb = gwb + (size_t)p.b * 8 * HW;
    const Nbrs n(p.y, p.x, p.r, H, W);
    float G[8], raw[8], R[8];
    const float S = gather_gates2(g + (size_t)p.b * 8 * HW, HW, n, norm, G, raw);
#pragma unroll
    for (int k = 0; k < 8; ++k) R[k] = rb[k * HW + p.r];
    norm_adjoint2(R, G, raw, S, n, p.y, p.x, p.r, gg + (size_t)p.b * 8 * HW, HW, H, W, norm);
}

}  // namespace

int normalize2d_backward(const float* g, const float* gwb, float* gg, int B, int H, int W, int norm, hipStream_t st) {
    const size_t total = (size_t)B * H * W;
    hipLaunchKernelGGL(normalize2d_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g, gwb, gg, B, H, W, norm);
    return check_launch("normalize2d_backward_kernel");
}

}  // namespace cspn
