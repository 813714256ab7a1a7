// cspn_gate_norm.hip -- the demo's gate normalisation as a stand-alone streaming pass and its adjoint (reference cspn_paddle/demo.py:24,
// 34-36,47-49): guide [N][K][V] raw -> gate [N][K][V], w_k(p) = |g_k(p)| / sum_j |g_j(p)| per voxel p over the K = 3^d - 1 gate channels of
// one slice (K = 26 in 3D, 8 in 2D; 24 and 48 for the 2D 5 x 5 and 7 x 7 neighbourhoods of cspn2d_kxk.hip).  The arithmetic form is cspn_gate_norm.h's, which the fused persistent 3D instance uses as well.
//   forward   K * 4 B read + K * 4 B written per voxel
//   backward  dL/dg_k = sign(g_k) (dL/dw_k - sum_j w_j dL/dw_j) / S, S = sum_j |g_j|, sign(0) = 0 (torch's abs backward): S and w are
//             recomputed from g (no saved w, no workspace), every output element is written once (no atomics); 2 K * 4 B read +
//             K * 4 B written per voxel.  An all-zero voxel gives NaN in all K gradients, as torch does (0 * NaN).
// 16-byte loads (four voxels per thread) where V % 4 == 0 and every pointer is 16-byte aligned, one voxel per thread everywhere else.
// Index arithmetic in size_t: N K V reaches 1.3 G elements at config 5.
// GT: the storage type of the guide and of dL/dguide (cspn_gate16.h; the 16-bit forms serve the 3D module, K = 26): widened exactly as it
// is read, 8-byte accesses in the vector kernels; w and dL/dw stay float32, dL/dguide is rounded once at its store.
#include <initializer_list>

#include "cspn_common.h"
#include "cspn_gate16.h"
#include "cspn_gate_norm.h"

namespace cspn {

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float sign0(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }

template <int K, class GT = float>
__global__ __launch_bounds__(NT) void gate_absnorm_kernel(const store_t<GT>* __restrict__ g, float* __restrict__ w, size_t V, size_t total) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;   // voxel of the N V
    if (i >= total) return;
    const size_t n = i / V, p = i - n * V;
    const store_t<GT>* gb = g + n * K * V + p;
    float* wb = w + n * K * V + p;
    float x[K];
#pragma unroll
    for (int k = 0; k < K; ++k) x[k] = widen<GT>(gb[(size_t)k * V]);
    const float r = absnorm_rcp<K>([&](int k) { return x[k]; });
#pragma unroll
    for (int k = 0; k < K; ++k) wb[(size_t)k * V] = absnorm_gate(x[k], r);
}

template <int K, class GT = float>
__global__ __launch_bounds__(NT) void gate_absnorm_kernel4(const store_t<GT>* __restrict__ g, float* __restrict__ w, size_t V4, size_t total4) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;   // quad of the N V / 4
    if (i >= total4) return;
    const size_t n = i / V4, p = i - n * V4;
    float4* wb = reinterpret_cast<float4*>(w) + n * K * V4 + p;
    float4 x[K];
    if constexpr (std::is_same<GT, float>::value) {
        const float4* gb = reinterpret_cast<const float4*>(g) + n * K * V4 + p;
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = gb[(size_t)k * V4];
    } else {
        const store_t<GT>* gb = g + 4 * (n * K * V4 + p);
#pragma unroll
        for (int k = 0; k < K; ++k) x[k] = ld4g<GT>(gb + 4 * ((size_t)k * V4));
    }
    const float r0 = absnorm_rcp<K>([&](int k) { return x[k].x; }), r1 = absnorm_rcp<K>([&](int k) { return x[k].y; });
    const float r2 = absnorm_rcp<K>([&](int k) { return x[k].z; }), r3 = absnorm_rcp<K>([&](int k) { return x[k].w; });
#pragma unroll
    for (int k = 0; k < K; ++k)
        wb[(size_t)k * V4] = make_float4(absnorm_gate(x[k].x, r0), absnorm_gate(x[k].y, r1), absnorm_gate(x[k].z, r2), absnorm_gate(x[k].w, r3));
}

// one voxel's adjoint: x = raw gates, d = dL/dw in, out = dL/dg (d may be overwritten)
template <int K>
__device__ __forceinline__ void absnorm_adjoint(const float (&x)[K], float (&d)[K]) {
    const float r = absnorm_rcp<K>([&](int k) { return x[k]; });
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) t = fmaf(absnorm_gate(x[k], r), d[k], t);
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = sign0(x[k]) * ((d[k] - t) * r);
}

template <int K, class GT = float>
__global__ __launch_bounds__(NT) void gate_absnorm_backward_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ gw,
                                                                   store_t<GT>* __restrict__ gg, size_t V, size_t total) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const size_t n = i / V, p = i - n * V, o = n * K * V + p;
    float x[K], d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        x[k] = widen<GT>(g[o + (size_t)k * V]);
        d[k] = gw[o + (size_t)k * V];
    }
    absnorm_adjoint<K>(x, d);
#pragma unroll
    for (int k = 0; k < K; ++k) gg[o + (size_t)k * V] = narrow<GT>(d[k]);
}

template <int K, class GT = float>
__global__ __launch_bounds__(NT) void gate_absnorm_backward_kernel4(const store_t<GT>* __restrict__ g, const float* __restrict__ gw,
                                                                    store_t<GT>* __restrict__ gg, size_t V4, size_t total4) {
    const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
    if (i >= total4) return;
    const size_t n = i / V4, p = i - n * V4, o = n * K * V4 + p;
    const store_t<GT>* gb = g + 4 * o;
    const float4* db = reinterpret_cast<const float4*>(gw) + o;
    store_t<GT>* ob = gg + 4 * o;
    float4 x4[K], d4[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        x4[k] = ld4g<GT>(gb + 4 * ((size_t)k * V4));
        d4[k] = db[(size_t)k * V4];
    }
    float x[K], d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { x[k] = x4[k].x; d[k] = d4[k].x; }
    absnorm_adjoint<K>(x, d);
#pragma unroll
    for (int k = 0; k < K; ++k) { d4[k].x = d[k]; x[k] = x4[k].y; d[k] = d4[k].y; }
    absnorm_adjoint<K>(x, d);
#pragma unroll
    for (int k = 0; k < K; ++k) { d4[k].y = d[k]; x[k] = x4[k].z; d[k] = d4[k].z; }
    absnorm_adjoint<K>(x, d);
#pragma unroll
    for (int k = 0; k < K; ++k) { d4[k].z = d[k]; x[k] = x4[k].w; d[k] = d4[k].w; }
    absnorm_adjoint<K>(x, d);
#pragma unroll
    for (int k = 0; k < K; ++k) st4g<GT>(ob + 4 * ((size_t)k * V4), d4[k].x, d4[k].y, d4[k].z, d[k]);
}

// V % 4 == 0, the float32 tensors 16-byte aligned, the tensors of GT aligned to four elements
bool vec4_ok(size_t V, std::initializer_list<const void*> ptrs, std::initializer_list<const void*> gptrs = {}, int gdt = 0) {
    if (V % 4) return false;
    for (const void* p : ptrs)
        if ((uintptr_t)p & 15u) return false;
    for (const void* p : gptrs)
        if ((uintptr_t)p & gate_quad_mask(gdt)) return false;
    return true;
}

template <int K, class GT = float>
int absnorm_launch(const store_t<GT>* g, float* w, int N, size_t V, hipStream_t st) {
    if (vec4_ok(V, {w}, {g}, std::is_same<GT, float>::value ? 0 : 1)) {
        const size_t t4 = (size_t)N * (V / 4);
        hipLaunchKernelGGL((gate_absnorm_kernel4<K, GT>), dim3((unsigned)((t4 + NT - 1) / NT)), dim3(NT), 0, st, g, w, V / 4, t4);
    } else {
        const size_t t = (size_t)N * V;
        hipLaunchKernelGGL((gate_absnorm_kernel<K, GT>), dim3((unsigned)((t + NT - 1) / NT)), dim3(NT), 0, st, g, w, V, t);
    }
    return check_launch("gate_absnorm_kernel");
}

template <int K, class GT = float>
int absnorm_backward_launch(const store_t<GT>* g, const float* gw, store_t<GT>* gg, int N, size_t V, hipStream_t st) {
    if (vec4_ok(V, {gw}, {g, gg}, std::is_same<GT, float>::value ? 0 : 1)) {
        const size_t t4 = (size_t)N * (V / 4);
        hipLaunchKernelGGL((gate_absnorm_backward_kernel4<K, GT>), dim3((unsigned)((t4 + NT - 1) / NT)), dim3(NT), 0, st, g, gw, gg, V / 4, t4);
    } else {
        const size_t t = (size_t)N * V;
        hipLaunchKernelGGL((gate_absnorm_backward_kernel<K, GT>), dim3((unsigned)((t + NT - 1) / NT)), dim3(NT), 0, st, g, gw, gg, V, t);
    }
    return check_launch("gate_absnorm_backward_kernel");
}

// K = 48 (7 x 7): one voxel per thread in the adjoint -- four voxels' raw gates and gradients would not fit the registers
int absnorm_backward_launch48(const float* g, const float* gw, float* gg, int N, size_t V, hipStream_t st) {
    const size_t t = (size_t)N * V;
    hipLaunchKernelGGL(gate_absnorm_backward_kernel<48>, dim3((unsigned)((t + NT - 1) / NT)), dim3(NT), 0, st, g, gw, gg, V, t);
    return check_launch("gate_absnorm_backward_kernel");
}

}  // namespace

// K in {8, 24, 26, 48}, N >= 1, V >= 1, N V < 2^31 * 256 (one thread per voxel or quad): checked by the caller (cspn_abi.cpp)
int gate_absnorm(const float* g, float* w, int N, int K, size_t V, hipStream_t st) {
    switch (K) {
        case 26: return absnorm_launch<26>(g, w, N, V, st);
        case 24: return absnorm_launch<24>(g, w, N, V, st);
        case 48: return absnorm_launch<48>(g, w, N, V, st);
        default: return absnorm_launch<8>(g, w, N, V, st);
    }
}

int gate_absnorm_backward(const float* g, const float* gw, float* gg, int N, int K, size_t V, hipStream_t st) {
    switch (K) {
        case 26: return absnorm_backward_launch<26>(g, gw, gg, N, V, st);
        case 24: return absnorm_backward_launch<24>(g, gw, gg, N, V, st);
        case 48: return absnorm_backward_launch48(g, gw, gg, N, V, st);
        default: return absnorm_backward_launch<8>(g, gw, gg, N, V, st);
    }
}

// K = 26, gdt CSPN_DTYPE_F16 or CSPN_DTYPE_BF16 (checked by the caller)
int gate_absnorm_g16(const void* g, int gdt, float* w, int N, size_t V, hipStream_t st) {
    if (gdt == CSPN_DTYPE_F16) return absnorm_launch<26, __half>((const unsigned short*)g, w, N, V, st);
    return absnorm_launch<26, __hip_bfloat16>((const unsigned short*)g, w, N, V, st);
}

int gate_absnorm_backward_g16(const void* g, int gdt, const float* gw, void* gg, int N, size_t V, hipStream_t st) {
    if (gdt == CSPN_DTYPE_F16) return absnorm_backward_launch<26, __half>((const unsigned short*)g, gw, (unsigned short*)gg, N, V, st);
    return absnorm_backward_launch<26, __hip_bfloat16>((const unsigned short*)g, gw, (unsigned short*)gg, N, V, st);
}

}  // namespace cspn
