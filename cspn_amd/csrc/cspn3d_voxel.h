// cspn3d_voxel.h -- the 3 x 3 x 3 neighbourhood of the one-launch-per-step 3D kernels (cspn3d_stepwise.hip, cspn3d_backward.hip,
// cspn3d_norm_backward.hip), written once: the channel order, a thread's voxel position, its vector loads and stores, the neighbour-row
// loader, the tap enumerator, and on the host the VEC dispatch (the vector kernels' condition, quads_ok, is cspn_gate16.h's).  cspn3d_persistent.hip keeps its own
// tap loop (its rows live in registers across the steps).
#pragma once
#include "cspn_common.h"
#include "cspn_gate16.h"

namespace cspn {

// Channel order: raster over (f,t,l) in {0,1,2}^3 without (1,1,1); channel k couples voxel p with p + (dz3, dy3, dx3)(k) = (1-f, 1-t, 1-l)
__host__ __device__ constexpr int ch3(int k) { return k < 13 ? k : k + 1; }  // skip the centre (index 13)
__host__ __device__ constexpr int dz3(int k) { return 1 - ch3(k) / 9; }
__host__ __device__ constexpr int dy3(int k) { return 1 - (ch3(k) / 3) % 3; }
__host__ __device__ constexpr int dx3(int k) { return 1 - ch3(k) % 3; }
// raster index c27 != 13 -> channel: the inverse of ch3 (the kernels walk the raster row by row: c27 = 3 n + t)
__host__ __device__ constexpr int tap3(int c27) { return c27 < 13 ? c27 : c27 - 1; }

static_assert(ch3(12) == 12 && ch3(13) == 14, "the centre is raster index 13");
static_assert(tap3(ch3(0)) == 0 && tap3(ch3(12)) == 12 && tap3(ch3(13)) == 13 && tap3(ch3(25)) == 25 && ch3(tap3(26)) == 26, "k <-> c27");
static_assert(dz3(0) == 1 && dy3(0) == 1 && dx3(0) == 1, "the first offset is (1,1,1)");
static_assert(dz3(25) == -1 && dy3(25) == -1 && dx3(25) == -1, "the last offset is (-1,-1,-1)");
static_assert(dz3(12) == 0 && dy3(12) == 0 && dx3(12) == 1 && dz3(13) == 0 && dy3(13) == 0 && dx3(13) == -1, "the centre's x-neighbours");

// voxel index -> (b, z, y, x) of a thread's VEC consecutive voxels (VEC = 4: W % 4 == 0, so they share a row)
template <int VEC>
struct Pos {
    int b, z, y, x;
    size_t r;   // offset inside the volume
    bool ok;
    __device__ Pos(int B, int D, int H, int W) {
        const size_t HW = (size_t)H * W, V = (size_t)D * HW, n = (size_t)B * V / VEC;
        const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
        ok = i < n;
        const size_t idx = (ok ? i : 0) * VEC;
        b = (int)(idx / V);
        r = idx - (size_t)b * V;
        z = (int)(r / HW);
        const int r2 = (int)(r - (size_t)z * HW);
        y = r2 / W;
        x = r2 - y * W;
    }
};

template <int VEC>
__device__ __forceinline__ void load_vec(const float* p, float* v) {
    if (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[0];
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float* p, const float* v) {
    if (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

// the thread's VEC consecutive elements of a gate-typed plane, widened / narrowed: one 16-byte (float) or 8-byte (16-bit) access
template <int VEC, class GT>
__device__ __forceinline__ void load_gvec(const store_t<GT>* p, float* v) {
    if (VEC == 4) {
        const float4 q = ld4g<GT>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = widen<GT>(p[0]);
    }
}

// narrow<GT>() of a value that a float multiply has just produced.  Left to itself the compiler folds that multiply into the float16
// conversion behind it (v_fma_mixlo_f16 a, b, +0), and (-0) + (+0) = +0: a product of -0 -- a negative dW' of a pinned voxel, a dG of zero
// times sign(g) = -1 -- would lose the sign the float32 engine stores.  The conversion as an instruction of its own keeps it; bfloat16 is
// rounded with integer operations, which nothing folds
template <class GT>
__device__ __forceinline__ store_t<GT> narrow_product(float v) {
    if constexpr (std::is_same<GT, __half>::value) {
        uint32_t h;
        asm("v_cvt_f16_f32 %0, %1" : "=v"(h) : "v"(v));
        return (unsigned short)h;
    } else {
        return narrow<GT>(v);
    }
}

template <int VEC, class GT>
__device__ __forceinline__ void store_gvec(store_t<GT>* p, const float* v) {
    if constexpr (std::is_same<GT, float>::value) {
        if (VEC == 4) st4g<GT>(p, v[0], v[1], v[2], v[3]);
        else p[0] = v[0];
    } else if (VEC == 4) {
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)narrow_product<GT>(v[0]) | ((uint32_t)narrow_product<GT>(v[1]) << 16),
                                                  (uint32_t)narrow_product<GT>(v[2]) | ((uint32_t)narrow_product<GT>(v[3]) << 16));
    } else {
        p[0] = narrow_product<GT>(v[0]);
    }
}

// v[i] = plane(z + dz, y + dy, x + i + dx) of one volume, zero outside it: a 16-byte load at 4-byte alignment (16-bit planes: an 8-byte
// load at 2-byte alignment) where the quad lies inside the row
template <int VEC, class GT>
__device__ __forceinline__ void load_shifted(const store_t<GT>* plane, const Pos<VEC>& p, int dz, int dy, int dx, int D, int H, int W, float* v) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[i] = 0.f;
    const int zz = p.z + dz, yy = p.y + dy, xs = p.x + dx;
    if (zz < 0 || zz >= D || yy < 0 || yy >= H) return;
    const store_t<GT>* row = plane + ((size_t)zz * H + yy) * W;
    if (VEC == 4 && xs >= 0 && xs + 3 < W) {
        const float4 q = ld4gu<GT>(row + xs);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (xs + i >= 0 && xs + i < W) v[i] = widen<GT>(row[xs + i]);
    }
}

// neighbour row n = 0 .. 8 of the raster: (dz, dy) = (1 - n / 3, 1 - n % 3), with the three x-taps t = 0 .. 2 (dx = 1 - t) of raster index
// 3 n + t.  for_taps3 calls f(k, dx) for the row's taps in raster order and skips the centre, which has no gate
__host__ __device__ constexpr int row_dz3(int n) { return 1 - n / 3; }
__host__ __device__ constexpr int row_dy3(int n) { return 1 - n % 3; }

template <class F>
__device__ __forceinline__ void for_taps3(int n, F f) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int c27 = n * 3 + t;
        if (c27 == 13) continue;
        f(tap3(c27), 1 - t);
    }
}

// h[0 .. VEC + 1] = the volume at row (z + dz, y + dy), columns x - 1 .. x + VEC, zero outside the volume.  Returns whether the row lies
// inside it: (dz, dy) = (row_dz3, row_dy3)(n) for the forward's neighbour rows, their negatives for the adjoint's source rows
template <int VEC>
__device__ __forceinline__ bool load_row3(const float* vol, const Pos<VEC>& p, int dz, int dy, int D, int H, int W, float* h) {
#pragma unroll
    for (int i = 0; i < VEC + 2; ++i) h[i] = 0.f;
    const int zz = p.z + dz, yy = p.y + dy;
    const bool inside = zz >= 0 && zz < D && yy >= 0 && yy < H;
    if (inside) {
        const float* row = vol + ((size_t)zz * H + yy) * W;
        load_vec<VEC>(row + p.x, h + 1);
        if (p.x > 0) h[0] = row[p.x - 1];
        if (p.x + VEC < W) h[VEC + 1] = row[p.x + VEC];
    }
    return inside;
}

// acc[k][i] += a[i] ht(p + off_k) over the 26 taps of the thread's voxels: one level's share of the gate gradient
// dL/dw_k(p) = sum_t A_{t+1}(p) H_t(p + off_k) (a = A_{t+1} at the voxels, ht = the volume H_t)
template <int VEC>
__device__ __forceinline__ void gate_grad_level3(float (&acc)[26][VEC], const float* a, const float* ht, const Pos<VEC>& p, int D, int H, int W) {
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        float h[VEC + 2];
        load_row3<VEC>(ht, p, row_dz3(n), row_dy3(n), D, H, W, h);
        for_taps3(n, [&](int k, int dx) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[k][i] = fmaf(a[i], h[1 + i + dx], acc[k][i]);
        });
    }
}

// G_k at the thread's voxels: the raw gate of plane k where the norm uses it (at the neighbour; NONE: at the voxel itself)
template <int VEC, class GT>
__device__ __forceinline__ void load_G(const store_t<GT>* gb, size_t V, int k, const Pos<VEC>& p, int D, int H, int W, int norm, float* G) {
    if (norm == CSPN_NORM_NONE) {
        load_gvec<VEC, GT>(gb + (size_t)k * V + p.r, G);
        return;
    }
    load_shifted<VEC, GT>(gb + (size_t)k * V, p, dz3(k), dy3(k), dx3(k), D, H, W, G);
    if (norm == CSPN_NORM_8SUM_ABS) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) G[i] = fabsf(G[i]);
    }
}

// ---- host side ----

// f(Vec<4>{}) where quads_ok() holds, else f(Vec<1>{}): the VEC of the kernels a host function launches (cf. with_gate_type)
template <int N>
struct Vec {
    static constexpr int value = N;
};

template <class F>
auto with_vec(bool vec, F f) {
    return vec ? f(Vec<4>{}) : f(Vec<1>{});
}

}  // namespace cspn
