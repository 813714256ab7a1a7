// cspn2d_nl_taps.h -- what the non-local kernels share (cspn2d_nl.hip, cspn2d_nl_det.hip): the neighbour bases, the sample of one pixel and
// neighbour (tap_of), the one-pixel-per-lane tiling, and the storage types of aff / offset.  The contract is stated in cspn2d_nl.hip.
#pragma once
#include "cspn_common.h"
#include "cspn_gate16.h"

namespace cspn {
namespace nl {

constexpr int NT = 256;
constexpr int PW = 64, PH = NT / PW;                // per-pixel kernels: a 64 x 4 pixel tile, a wave is 64 adjacent pixels of a row
constexpr float FLOOR_LIM = 536870912.f;            // 2^29: p + base + floor(d) stays an int, and is outside every image (H W <= 2^27)

template <int K>
__host__ __device__ constexpr int base_y(int k) { return (k + (k >= (K / 2) * (K + 1) ? 1 : 0)) / K - K / 2; }
template <int K>
__host__ __device__ constexpr int base_x(int k) { return (k + (k >= (K / 2) * (K + 1) ? 1 : 0)) % K - K / 2; }

// the sample p + base + d of one pixel and neighbour: i00 the in-plane index of corner (y0, x0) with both coordinates clamped into the
// image, sx / sy the steps to the corners at x0 + 1 / y0 + 1 after their clamp (0 or 1, 0 or W): all four addresses are inside the plane.
// ok: bit i set where corner i (00, 01, 10, 11) is inside the image; w: the corner weights, zero where it is not
struct Tap {
    int i00, sx, sy;
    int cy0, cx0;   // corner (y0, x0), clamped: i00 = cy0 W + cx0
    unsigned ok;
    float fy, fx;
    float w[4];
};

__device__ __forceinline__ Tap tap_of(float dy, float dx, int y, int x, int by, int bx, int H, int W) {
    Tap t;
    const float gy = floorf(dy), gx = floorf(dx);
    t.fy = dy - gy;
    t.fx = dx - gx;
    const int y0 = y + by + (int)fminf(fmaxf(gy, -FLOOR_LIM), FLOOR_LIM), x0 = x + bx + (int)fminf(fmaxf(gx, -FLOOR_LIM), FLOOR_LIM);
    const int y1 = y0 + 1, x1 = x0 + 1;
    const bool oy0 = !(y0 >= 0 && y0 < H), oy1 = !(y1 >= 0 && y1 < H), ox0 = !(x0 >= 0 && x0 < W), ox1 = !(x1 >= 0 && x1 < W);
    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1), cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
    t.i00 = cy0 * W + cx0;
    t.cy0 = cy0;
    t.cx0 = cx0;
    t.sx = cx1 - cx0;
    t.sy = (cy1 - cy0) * W;
    t.ok = ((oy0 || ox0) ? 0u : 1u) | ((oy0 || ox1) ? 0u : 2u) | ((oy1 || ox0) ? 0u : 4u) | ((oy1 || ox1) ? 0u : 8u);
    const float gy1 = 1.f - t.fy, gx1 = 1.f - t.fx;
    t.w[0] = (t.ok & 1u) ? gy1 * gx1 : 0.f;
    t.w[1] = (t.ok & 2u) ? gy1 * t.fx : 0.f;
    t.w[2] = (t.ok & 4u) ? t.fy * gx1 : 0.f;
    t.w[3] = (t.ok & 8u) ? t.fy * t.fx : 0.f;
    return t;
}

struct Pixel {
    int n, y, x;
    bool in;
};

__device__ __forceinline__ Pixel pixel_of(int tiles_x, int tiles_y, int H, int W) {
    int b = blockIdx.x;
    Pixel p;
    const int tx = b % tiles_x;
    b /= tiles_x;
    p.y = (b % tiles_y) * PH + threadIdx.x / PW;
    p.n = b / tiles_y;
    p.x = tx * PW + threadIdx.x % PW;
    p.in = p.y < H && p.x < W;
    return p;
}

struct Grid {
    int tx, ty;
    unsigned blocks;
};

inline Grid pixel_grid(int N, int H, int W) {
    Grid g;
    g.tx = (W + PW - 1) / PW;
    g.ty = (H + PH - 1) / PH;
    g.blocks = (unsigned)((size_t)N * g.tx * g.ty);
    return g;
}

// the one rounding of a float32 gradient at its store (cspn_gate16.h: narrow).  The value is first taken out of the compiler's reach: folded into
// the conversion, a product a * b becomes fma(a, b, +0) (v_fma_mixlo_f16), whose zero results are all +0, where the float32 kernel stores a * b
// with its sign.  The float32 instance has no such fold and stays the code it was
template <class GT>
__device__ __forceinline__ store_t<GT> narrow_value(float v) {
    if constexpr (!std::is_same<GT, float>::value) asm volatile("" : "+v"(v));
    return narrow<GT>(v);
}

// host side: f(Tag<AT>{}, Tag<OT>{}) for the storage types of aff and offset.  The pairs the entry points let through (cspn_abi.cpp:
// nl_dtype_check): (0, 0), (0, T) and (T, T), T = CSPN_DTYPE_F16 or CSPN_DTYPE_BF16; no other pair has an instance
template <class F>
auto with_nl_types(int adt, int odt, F f) {
    if (odt == 0) return f(Tag<float>{}, Tag<float>{});
    if (odt == CSPN_DTYPE_F16) return adt == 0 ? f(Tag<float>{}, Tag<__half>{}) : f(Tag<__half>{}, Tag<__half>{});
    return adt == 0 ? f(Tag<float>{}, Tag<__hip_bfloat16>{}) : f(Tag<__hip_bfloat16>{}, Tag<__hip_bfloat16>{});
}

}  // namespace nl
}  // namespace cspn
