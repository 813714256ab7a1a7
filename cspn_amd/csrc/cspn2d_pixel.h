// cspn2d_pixel.h -- the 3 x 3 neighbourhood of the one-thread-per-pixel 2D kernels (cspn2d_stepwise.hip, cspn2d_backward.hip,
// cspn2d_normalize_backward.hip, head_norm_sited_kernel of cspn_head.hip), written once: a thread's pixel, the bounds test, a plane read at a
// tap, the eight neighbours, the neighbour-sited gather of the gates with their abs-sum, and the adjoint of the normalisation.  The 2D sibling
// of cspn3d_voxel.h; the channel offsets dy2 / dx2 are cspn_common.h's.  The four-column kernels (bwd_final_mx_kernel and its epilogue, the
// rings) keep their own arithmetic: other vector width, other rounding contract.
#pragma once
#include "cspn_common.h"

namespace cspn {

// element index -> (b, y, x) of a thread's pixel in B images of H rows at a pitch of Wp columns
struct Pixel {
    size_t idx;   // element of a [B][H][Wp] plane
    int b, r, y, x;   // r: offset inside the image
    bool ok;
    __device__ __forceinline__ Pixel(int B, int H, int Wp) {
        const size_t HW = (size_t)H * Wp;
        idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        ok = idx < (size_t)B * HW;
        b = (int)(idx / HW);
        r = (int)(idx - (size_t)b * HW);
        y = r / Wp;
        x = r - y * Wp;
    }
};

__device__ __forceinline__ bool in_image(int y, int x, int H, int W) { return y >= 0 && y < H && x >= 0 && x < W; }

// torch.sign without the NaN: d|v|/dv as autograd has it, 0 at 0
__device__ __forceinline__ float sign0f(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// f(k, dy, dx) for the eight channels in order
template <class F>
__device__ __forceinline__ void for_taps2(F f) {
#pragma unroll
    for (int k = 0; k < 8; ++k) f(k, dy2(k), dx2(k));
}

// img(y + dy, x + dx) of one H x W image, zero outside it (ZeroPad2d, cspn.py:149-167)
__device__ __forceinline__ float load_tap2(const float* img, int y, int x, int dy, int dx, int H, int W) {
    const int yy = y + dy, xx = x + dx;
    float v = 0.f;
    if (in_image(yy, xx, H, W)) v = img[(size_t)yy * W + xx];
    return v;
}

// the eight neighbours p + off_k of pixel (y, x): inside the image?  Where the gate G_k(p) lies inside a plane: at the neighbour (where that is
// outside: 0, always valid and uniform -- a fallback to the pixel's own offset cost normalize2d_backward_kernel a wave per SIMD).
// consumer: the planes hold g_k(p + off_k) at p = offset r already (head_raw_kernel<true>)
struct Nbrs {
    bool ok[8];
    int off[8];
    __device__ __forceinline__ Nbrs(int y, int x, int r, int H, int W, bool consumer = false) {
        for_taps2([&](int k, int dy, int dx) {
            const int yy = y + dy, xx = x + dx;
            ok[k] = in_image(yy, xx, H, W);
            off[k] = consumer ? r : (ok[k] ? yy * W + xx : 0);
        });
    }
};

// G_k(p) = g~_k(p + off_k), zero outside the image, g~ = |g| for '8sum_abs' (cspn.py:105-132); raw_k = the stored value; returns S = sum_k |G_k|.
// gb: the image's eight planes
__device__ __forceinline__ float gather_gates2(const float* gb, size_t HW, const Nbrs& n, int norm, float (&G)[8], float (&raw)[8]) {
    float S = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = n.ok[k] ? gb[k * HW + n.off[k]] : 0.f;
        raw[k] = v;
        G[k] = norm == CSPN_NORM_8SUM_ABS ? fabsf(v) : v;
        S += fabsf(G[k]);
    }
    return S;
}
__device__ __forceinline__ float gather_gates2(const float* gb, size_t HW, const Nbrs& n, int norm, float (&G)[8]) {
    float raw[8];
    return gather_gates2(gb, HW, n, norm, G, raw);
}

// the adjoint of w_k = G_k / S at pixel (y, x), R_k = dL/dw_k(p):  dL/dg_k(p + off_k) = (R_k / S - sign(G_k) T / S^2) [* sign(g_k) for '8sum_abs'],
// T = sum_j R_j G_j (torch: d|x|/dx = sign(x), 0 at 0; IEEE division: S = 0 gives NaN as torch does).  ob: the image's eight gradient planes.
// g_k(p + off_k) is read by pixel p only, and g_k(q) with q - off_k outside the image by no pixel (the gather sees the zero padding instead):
// the thread zeroes those of its own elements, so every element is written exactly once
__device__ __forceinline__ void norm_adjoint2(const float (&R)[8], const float (&G)[8], const float (&raw)[8], float S, const Nbrs& n, int y, int x,
                                              int r, float* ob, size_t HW, int H, int W, int norm) {
    float T = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) T = fmaf(R[k], G[k], T);
    for_taps2([&](int k, int dy, int dx) {
        if (!in_image(y - dy, x - dx, H, W)) ob[k * HW + r] = 0.f;
    });
    const float t2 = T / (S * S);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (!n.ok[k]) continue;  // the zero padding is a constant
        float d = R[k] / S - sign0f(G[k]) * t2;
        if (norm == CSPN_NORM_8SUM_ABS) d *= sign0f(raw[k]);
        ob[k * HW + n.off[k]] = d;
    }
}

}  // namespace cspn
