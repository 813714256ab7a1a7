// cspn3d_norm_backward.hip -- backward of the 3x3x3 propagation in its normalising / masked modes: the 3D form of the
// depth-completion contract (the forward is fold3d_kernel + step3d_kernel of cspn3d_stepwise.hip).
//
//   forward   off_k = (dz3, dy3, dx3)(k),  g~ = |g| (8SUM_ABS) or g,  zero outside the volume
//             G_k(p) = g~_k(p + off_k)                 (NONE: G_k(p) = g_k(p), S = 1, no centre term)
//             S = sum_j |G_j|,  wb_k = G_k / S,  sigma = sum_k wb_k,  m = sign(sparse) (0 without sparse),  u = 1 - m
//             w'_k = u wb_k,  coef = u (1 - sigma) + m (NONE: m),  c' = coef H_0
//             H_0 = feat,  H_{t+1}(p) = c'(p) + sum_k w'_k(p) H_t(p + off_k),  out = H_n
//   backward  A_n = grad_out,  A_t(q) = sum_k w'_k(q - off_k) A_{t+1}(q - off_k)
//             dW'_k(p) = sum_{t<n} A_{t+1}(p) H_t(p + off_k),  dC(p) = sum_{t<n} A_{t+1}(p)
//             grad_feat = A_0 + dC coef
//             dwb_k = u (dW'_k - dC H_0)                                   (NONE: grad_guidance_k = u dW'_k, done)
//             T = sum_j dwb_j G_j,  dG_k = dwb_k / S - sign(G_k) T / S^2   (sign(0) = 0; S = 0: NaN, as the forward)
//             grad_guidance_k(q) = dG_k(q - off_k) [x sign(g_k(q)) for 8SUM_ABS],  0 where q - off_k is outside
//
// Launches, all HBM-bound streaming, no atomics, every output element written once:
//   1. fold_norm3d_kernel: w' as a gate tensor [B][26][V] + the planes c' and coef, into the workspace
//   2. step_const3d_kernel x (n - 1): H_1 .. H_{n-1} (27 planes + H in, H out), only when grad_guidance is wanted
//   3. the n adjoint steps on w', read as the gates of the Paddle contract, keeping A_1 .. A_{n-1}, A_0 in the workspace: ONE launch of
//      the persistent kernel's transposed instance where it takes the call (W % 4 == 0, 16-byte aligned tensors, 3 <= n_iter <= 60, the
//      volume resident on the device: as backward3d()'s fused sweeps), else backward3d() of cspn3d_backward.hip, one launch per step
//   4. gate_grad_norm3d_kernel: dW' and dC in registers from the 2n value volumes, then the per-voxel fold adjoint: grad_feat, and
//      the consumer-sited dG over the w' planes (which nothing reads any more); NONE writes grad_guidance itself
//   5. gather_guidance3d_kernel: grad_guidance_k(q) from dG_k(q - off_k)
//
// GT is the storage type of guidance and grad_guidance (cspn_gate16.h): float, or __half / __hip_bfloat16 (cspn3d_backward_norm_g16).  The three
// kernels that touch the guidance read a 16-bit gate where they use it, widened exactly, and grad_guidance is the float32 value rounded once at
// its single store; w', c', coef, dG, every level and every sum stay float32, so grad_feat is bitwise the float32 call's on the widened guidance
// and grad_guidance that call's converted to the type.  step_const3d_kernel and the adjoint sweep never see the guidance.
#include <initializer_list>

#include "cspn_common.h"
#include "cspn_gate16.h"

namespace cspn {

namespace {

__host__ __device__ constexpr int ch3(int k) { return k < 13 ? k : k + 1; }  // skip the centre (index 13)
__host__ __device__ constexpr int dz3(int k) { return 1 - ch3(k) / 9; }
__host__ __device__ constexpr int dy3(int k) { return 1 - (ch3(k) / 3) % 3; }
__host__ __device__ constexpr int dx3(int k) { return 1 - ch3(k) % 3; }

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

// the thread's VEC consecutive elements of a guidance-typed plane, widened / narrowed: one 16-byte (float) or 8-byte (16-bit) access
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

// the fold of fold3d_kernel with w' laid out as a gate tensor: wp [B][26][V], cp = c' and kp = coef [B][V]
template <int VEC, class GT>
__global__ __launch_bounds__(256) void fold_norm3d_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ feat,
                                                           const float* __restrict__ sparse, float* __restrict__ wp,
                                                           float* __restrict__ cp, float* __restrict__ kp, int B, int D, int H, int W,
                                                           int norm) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, vox = (size_t)p.b * V + p.r;
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V;
    float G[26][VEC], S[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) S[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        load_G<VEC, GT>(gb, V, k, p, D, H, W, norm, G[k]);
#pragma unroll
        for (int i = 0; i < VEC; ++i) S[i] += fabsf(G[k][i]);
    }
    float sigma[VEC], h0[VEC], m[VEC], c[VEC], coef[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sigma[i] = 0.f; m[i] = 0.f; }
#pragma unroll
    for (int k = 0; k < 26; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (norm != CSPN_NORM_NONE) G[k][i] = G[k][i] / S[i];
            sigma[i] += G[k][i];
        }
    load_vec<VEC>(feat + vox, h0);
    if (sparse) {
        load_vec<VEC>(sparse + vox, m);
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[i] = signf(m[i]);
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float om = 1.f - m[i];
        coef[i] = (norm == CSPN_NORM_NONE) ? m[i] : om * (1.f - sigma[i]) + m[i];
        c[i] = coef[i] * h0[i];
        if (sparse) {
#pragma unroll
            for (int k = 0; k < 26; ++k) G[k][i] *= om;
        }
    }
    float* o = wp + (size_t)p.b * 26 * V + p.r;
#pragma unroll
    for (int k = 0; k < 26; ++k) store_vec<VEC>(o + (size_t)k * V, G[k]);
    store_vec<VEC>(cp + vox, c);
    store_vec<VEC>(kp + vox, coef);
}

// one forward step with the constant term: hout(p) = c'(p) + sum_k w'_k(p) hin(p + off_k)
template <int VEC>
__global__ __launch_bounds__(256) void step_const3d_kernel(const float* __restrict__ wp, const float* __restrict__ cp,
                                                            const float* __restrict__ hin, float* __restrict__ hout, int B, int D,
                                                            int H, int W) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, vox = (size_t)p.b * V + p.r;
    const float* hb = hin + (size_t)p.b * V;
    const float* wb = wp + (size_t)p.b * 26 * V + p.r;
    float acc[VEC];
    load_vec<VEC>(cp + vox, acc);
#pragma unroll
    for (int n = 0; n < 9; ++n) {   // neighbour rows (z + dz, y + dy); three x-taps each
        const int dz = 1 - n / 3, dy = 1 - n % 3;
        const int zz = p.z + dz, yy = p.y + dy;
        float h[VEC + 2];   // hin at columns x-1 .. x+VEC of the row, zero outside the volume
#pragma unroll
        for (int i = 0; i < VEC + 2; ++i) h[i] = 0.f;
        if (zz >= 0 && zz < D && yy >= 0 && yy < H) {
            const float* row = hb + ((size_t)zz * H + yy) * W;
            load_vec<VEC>(row + p.x, h + 1);
            if (p.x > 0) h[0] = row[p.x - 1];
            if (p.x + VEC < W) h[VEC + 1] = row[p.x + VEC];
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int c27 = n * 3 + t;
            if (c27 == 13) continue;
            const int k = c27 < 13 ? c27 : c27 - 1;
            const int dx = 1 - t;
            float w[VEC];
            load_vec<VEC>(wb + (size_t)k * V, w);
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(w[i], h[1 + i + dx], acc[i]);
        }
    }
    store_vec<VEC>(hout + vox, acc);
}

// dW'_k(p) = sum_t A_{t+1}(p) H_t(p + off_k) and dC(p) = sum_t A_{t+1}(p) in registers (H_0 = feat, H_t = hist + (t-1) total;
// A_n = gout, A_t = ahist + (t-1) total), then the fold's adjoint at the voxel:
//   gf (may be NULL) = A_0 + dC coef;  planes (may be NULL: then hist is not read) = the consumer-sited dG_k [B][26][V] in float32, or with
//   NONE the guidance gradient u dW'_k itself, in the guidance's type
template <int VEC, class GT>
__global__ __launch_bounds__(256) void gate_grad_norm3d_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ feat,
                                                                const float* __restrict__ sparse, const float* __restrict__ kp,
                                                                const float* __restrict__ hist, const float* __restrict__ ahist,
                                                                const float* __restrict__ gout, const float* __restrict__ a0,
                                                                void* __restrict__ planes, float* __restrict__ gf, int B, int D,
                                                                int H, int W, int n_iter, int norm) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, total = (size_t)B * V, vol = (size_t)p.b * V, vox = vol + p.r;
    float acc[26][VEC], dC[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) dC[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;
#pragma unroll 1
    for (int t = 0; t < n_iter; ++t) {
        const float* at = t == n_iter - 1 ? gout : ahist + (size_t)t * total;   // A_{t+1}
        float a[VEC];
        load_vec<VEC>(at + vox, a);
#pragma unroll
        for (int i = 0; i < VEC; ++i) dC[i] += a[i];
        if (!planes) continue;
        const float* ht = (t == 0 ? feat : hist + (size_t)(t - 1) * total) + vol;
#pragma unroll
        for (int n = 0; n < 9; ++n) {   // neighbour rows (z + dz, y + dy)
            const int dz = 1 - n / 3, dy = 1 - n % 3;
            const int zz = p.z + dz, yy = p.y + dy;
            float h[VEC + 2];
#pragma unroll
            for (int i = 0; i < VEC + 2; ++i) h[i] = 0.f;
            if (zz >= 0 && zz < D && yy >= 0 && yy < H) {
                const float* row = ht + ((size_t)zz * H + yy) * W;
                load_vec<VEC>(row + p.x, h + 1);
                if (p.x > 0) h[0] = row[p.x - 1];
                if (p.x + VEC < W) h[VEC + 1] = row[p.x + VEC];
            }
#pragma unroll
            for (int t3 = 0; t3 < 3; ++t3) {
                const int c27 = n * 3 + t3;
                if (c27 == 13) continue;
                const int k = c27 < 13 ? c27 : c27 - 1;
                const int dx = 1 - t3;
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[k][i] = fmaf(a[i], h[1 + i + dx], acc[k][i]);
            }
        }
    }
    if (gf) {
        float a[VEC], coef[VEC];
        load_vec<VEC>(a0 + vox, a);
        load_vec<VEC>(kp + vox, coef);
#pragma unroll
        for (int i = 0; i < VEC; ++i) a[i] = fmaf(dC[i], coef[i], a[i]);
        store_vec<VEC>(gf + vox, a);
    }
    if (!planes) return;
    float u[VEC], h0[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) u[i] = 0.f;
    if (sparse) load_vec<VEC>(sparse + vox, u);
#pragma unroll
    for (int i = 0; i < VEC; ++i) u[i] = 1.f - (sparse ? signf(u[i]) : 0.f);
    float* o = (float*)planes + (size_t)p.b * 26 * V + p.r;
    if (norm == CSPN_NORM_NONE) {
        store_t<GT>* og = (store_t<GT>*)planes + (size_t)p.b * 26 * V + p.r;   // (the same elements, of the guidance's type)
#pragma unroll
        for (int k = 0; k < 26; ++k) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[k][i] *= u[i];
            store_gvec<VEC, GT>(og + (size_t)k * V, acc[k]);
        }
        return;
    }
    load_vec<VEC>(feat + vox, h0);
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V;
    float S[VEC], T[VEC];
    unsigned pos[VEC], neg[VEC];   // bit k: G_k > 0 / G_k < 0 (a NaN gate sets neither: its dG is NaN through S)
#pragma unroll
    for (int i = 0; i < VEC; ++i) { S[i] = 0.f; T[i] = 0.f; pos[i] = 0u; neg[i] = 0u; }
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        float G[VEC];
        load_G<VEC, GT>(gb, V, k, p, D, H, W, norm, G);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            acc[k][i] = u[i] * (acc[k][i] - dC[i] * h0[i]);   // dwb_k
            S[i] += fabsf(G[i]);
            T[i] = fmaf(acc[k][i], G[i], T[i]);
            pos[i] |= (G[i] > 0.f ? 1u : 0u) << k;
            neg[i] |= (G[i] < 0.f ? 1u : 0u) << k;
        }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) T[i] = T[i] / (S[i] * S[i]);
#pragma unroll
    for (int k = 0; k < 26; ++k) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float sg = (float)((pos[i] >> k) & 1u) - (float)((neg[i] >> k) & 1u);
            acc[k][i] = acc[k][i] / S[i] - sg * T[i];
        }
        store_vec<VEC>(o + (size_t)k * V, acc[k]);
    }
}

// grad_guidance_k(q) = dG_k(q - off_k) [x sign(g_k(q)) for 8SUM_ABS], zero where q - off_k is outside the volume: a gather at q
template <int VEC, class GT>
__global__ __launch_bounds__(256) void gather_guidance3d_kernel(const float* __restrict__ dG, const store_t<GT>* __restrict__ g,
                                                                 store_t<GT>* __restrict__ gg, int B, int D, int H, int W, int norm) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, base = (size_t)p.b * 26 * V;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        float v[VEC];
        load_shifted<VEC, float>(dG + base + (size_t)k * V, p, -dz3(k), -dy3(k), -dx3(k), D, H, W, v);
        if (norm == CSPN_NORM_8SUM_ABS) {
            float s[VEC];
            load_gvec<VEC, GT>(g + base + (size_t)k * V + p.r, s);
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] *= s[i] > 0.f ? 1.f : (s[i] < 0.f ? -1.f : 0.f);
        }
        store_gvec<VEC, GT>(gg + base + (size_t)k * V + p.r, v);
    }
}

size_t planes_bytes(size_t total, int planes) { return round256(sizeof(float) * total * (size_t)planes); }

// the vector kernels' condition: four voxels of a thread share a row, every float32 tensor of the call is 16-byte aligned and the two
// guidance-typed ones to four of their elements (16 bytes, or 8 for a 16-bit type); NULL: absent
bool quads_ok(int W, int gdt, std::initializer_list<const void*> gates, std::initializer_list<const void*> tensors) {
    uintptr_t gbits = 0, bits = 0;
    for (const void* t : gates) gbits |= (uintptr_t)t;
    for (const void* t : tensors) bits |= (uintptr_t)t;
    return (W % 4) == 0 && (gbits & gate_quad_mask(gdt)) == 0 && (bits & 15u) == 0;
}

}  // namespace

// w' / dG (26 planes), c', coef, then the workspace of backward3d(): the levels H_1 .. H_{n-1}, A_1 .. A_{n-1}, A_0 and what the persistent
// kernel wants.  The same for every guidance type: everything in it is float32
size_t backward3d_norm_workspace(int B, int D, int H, int W, int n_iter) {
    const size_t total = (size_t)B * D * H * W;
    return planes_bytes(total, 26) + 2 * planes_bytes(total, 1) + backward3d_workspace(B, D, H, W, n_iter);
}

// where the adjoint sweep goes through the transposed instance of the persistent kernel (w' resident in registers across the n steps):
// the conditions of backward3d()'s fused sweeps, on every tensor of the call (g and gg of type gdt: aligned to four elements)
bool backward3d_norm_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, const void* gg, const float* gf,
                           int B, int D, int H, int W, int n_iter, const void* ws) {
    return quads_ok(W, gdt, {g, gg}, {feat, sparse, gout, gf, ws}) && n_iter >= 3 && persistent3d_supported(B, D, H, W, n_iter - 1) &&
           persistent3d_supported(B, D, H, W, n_iter);
}

// norm 8SUM / 8SUM_ABS, or NONE with a mask; gg and gf may each be NULL (not both).  stepwise_only: one launch per adjoint step also where
// backward3d_norm_fused() holds.  gdt: the storage type of g and gg (0 float32, CSPN_DTYPE_F16, CSPN_DTYPE_BF16)
int backward3d_norm(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, void* gg, float* gf, int B, int D,
                    int H, int W, int n_iter, int norm, void* ws, hipStream_t st, bool stepwise_only) {
    const size_t V = (size_t)D * H * W, total = (size_t)B * V;
    float* wp = (float*)ws;
    float* cp = (float*)((char*)ws + planes_bytes(total, 26));
    float* kp = (float*)((char*)cp + planes_bytes(total, 1));
    float* levels = (float*)((char*)kp + planes_bytes(total, 1));   // the layout of backward3d()
    float* hist = levels;                                          // H_1 .. H_{n-1}
    float* ahist = hist + (size_t)(n_iter - 1) * total;            // A_1 .. A_{n-1}
    float* a0 = ahist + (size_t)(n_iter - 1) * total;
    void* pws = (char*)levels + (backward3d_workspace(B, D, H, W, n_iter) - persistent3d_workspace(B, D, H, W));
    const bool vec = quads_ok(W, gdt, {g, gg}, {feat, sparse, gout, gf, ws});
    const bool fused = !stepwise_only && backward3d_norm_fused(g, gdt, feat, sparse, gout, gg, gf, B, D, H, W, n_iter, ws);
    const dim3 grid((unsigned)((total / (vec ? 4 : 1) + 255) / 256)), block(256);
#define CSPN_LAUNCH_VEC(kernel, ...)                                                 \
    do {                                                                              \
        if (vec) hipLaunchKernelGGL(kernel<4>, grid, block, 0, st, __VA_ARGS__);      \
        else hipLaunchKernelGGL(kernel<1>, grid, block, 0, st, __VA_ARGS__);          \
    } while (0)
#define CSPN_LAUNCH_VEC_GT(kernel, ...)                                                  \
    do {                                                                                  \
        if (vec) hipLaunchKernelGGL((kernel<4, GT>), grid, block, 0, st, __VA_ARGS__);    \
        else hipLaunchKernelGGL((kernel<1, GT>), grid, block, 0, st, __VA_ARGS__);        \
    } while (0)
    return with_gate_type(gdt, [&](auto gt) -> int {
        using GT = typename decltype(gt)::type;
        const store_t<GT>* gs = (const store_t<GT>*)g;
        CSPN_LAUNCH_VEC_GT(fold_norm3d_kernel, gs, feat, sparse, wp, cp, kp, B, D, H, W, norm);
        if (int e = check_launch("fold_norm3d_kernel")) return e;
        if (gg) {
            const float* src = feat;
            for (int t = 1; t < n_iter; ++t) {
                float* dst = hist + (size_t)(t - 1) * total;
                CSPN_LAUNCH_VEC(step_const3d_kernel, wp, cp, src, dst, B, D, H, W);
                src = dst;
            }
            if (int e = check_launch("step_const3d_kernel")) return e;
        }
        // the adjoint levels have no constant term: the Paddle contract's on w' (float32 whatever the guidance is).  Fused: step it = 1 .. n
        // of the transposed run produces A_{n-it}, volume n - it - 1 of ahist, the last one (A_0) its "out"; else backward3d()'s per-step
        // launches (A_0 only where grad_feat wants it)
        if (fused) {
            if (int e = persistent3d_run(wp, gout, a0, ahist, n_iter - 1, -1, true, B, D, H, W, n_iter, pws, st)) return e;
        } else if (int e = backward3d(wp, feat, gout, nullptr, gf ? a0 : nullptr, B, D, H, W, n_iter, levels, st, true)) {
            return e;
        }
        void* planes = !gg ? nullptr : (norm == CSPN_NORM_NONE ? gg : (void*)wp);
        CSPN_LAUNCH_VEC_GT(gate_grad_norm3d_kernel, gs, feat, sparse, kp, hist, ahist, gout, a0, planes, gf, B, D, H, W, n_iter, norm);
        if (int e = check_launch("gate_grad_norm3d_kernel")) return e;
        if (gg && norm != CSPN_NORM_NONE) {
            CSPN_LAUNCH_VEC_GT(gather_guidance3d_kernel, wp, gs, (store_t<GT>*)gg, B, D, H, W, norm);
            if (int e = check_launch("gather_guidance3d_kernel")) return e;
        }
        return 0;
    });
#undef CSPN_LAUNCH_VEC
#undef CSPN_LAUNCH_VEC_GT
}

}  // namespace cspn
