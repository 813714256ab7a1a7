// cspn3d_norm_backward.hip -- backward of the 3x3x3 propagation in its normalising / masked modes: the 3D form of the
// depth-completion contract (the forward is fold3d_kernel + step3d_kernel of cspn3d_stepwise.hip).  The voxel helpers
// (Pos, the vector loads and stores, load_G, gate_grad_level3, quads_ok, with_vec): cspn3d_voxel.h.
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
//   2. the forward step with the constant term x (n - 1): H_1 .. H_{n-1} (27 planes + H in, H out), only when grad_guidance is wanted; the
//      kernels are cspn3d_stepwise.hip's: step3d_direct_kernel<float, true> on w' (four voxels a thread), else step3d_kernel
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
// and grad_guidance that call's converted to the type.  The forward steps on w' and the adjoint sweep never see the guidance.
//
// C value channels on SHARED guidance (backward3d_norm_multi; feat / gout / gf [B][C][V], sparse [B][V]): launch 1 without c' (each channel's
// constant term is coef H_{0,c}), launch 2 is step3d_shared_kernel (w' and coef read once for the C channels), launch 3 the transposed
// multi-channel instance or backward3d()'s per-step launches channel by channel, launch 4 the MULTI instance of gate_grad_norm3d_kernel
// (dW' summed over c then t, D = sum_c dC_c H_{0,c}), launch 5 unchanged.
#include "cspn3d_voxel.h"

namespace cspn {

namespace {

// the fold of fold3d_kernel with w' laid out as a gate tensor: wp [B][26][V], cp = c' and kp = coef [B][V].  CP = false: no c' (feat and cp
// are not touched): what C value channels share, each forming its own coef H_0
template <int VEC, class GT, bool CP = true>
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
    if constexpr (CP) load_vec<VEC>(feat + vox, h0);
    if (sparse) {
        load_vec<VEC>(sparse + vox, m);
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[i] = signf(m[i]);
    }
    // c' in this file's rounding, ((1 - m) (1 - sigma) + m) h0: fold3d_kernel forms (1 - m) ((1 - sigma) h0) + m h0, and each output stays
    // bitwise what it has always been
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const float om = 1.f - m[i];
        coef[i] = (norm == CSPN_NORM_NONE) ? m[i] : om * (1.f - sigma[i]) + m[i];
        if constexpr (CP) c[i] = coef[i] * h0[i];
        if (sparse) {
#pragma unroll
            for (int k = 0; k < 26; ++k) G[k][i] *= om;
        }
    }
    float* o = wp + (size_t)p.b * 26 * V + p.r;
#pragma unroll
    for (int k = 0; k < 26; ++k) store_vec<VEC>(o + (size_t)k * V, G[k]);
    if constexpr (CP) store_vec<VEC>(cp + vox, c);
    store_vec<VEC>(kp + vox, coef);
}

// dW'_k(p) = sum_t A_{t+1}(p) H_t(p + off_k) and dC(p) = sum_t A_{t+1}(p) in registers (H_0 = feat, H_t = hist + (t-1) total;
// A_n = gout, A_t = ahist + (t-1) total), then the fold's adjoint at the voxel:
//   gf (may be NULL) = A_0 + dC coef;  planes (may be NULL: then hist is not read) = the consumer-sited dG_k [B][26][V] in float32, or with
//   NONE the guidance gradient u dW'_k itself, in the guidance's type
// MULTI: C value channels share the gates (feat, gout, gf and every level [B][C][V]; kp, sparse and the planes stay [B][V]): dW' is summed
// over the channels in the same registers, channel by channel and level by level inside one (a fixed order: bitwise reproducible), dC_c
// and grad_feat_c are each channel's own, and the fold's adjoint takes D = sum_c dC_c H_{0,c} where one channel has dC H_0
template <int VEC, class GT, bool MULTI = false>
__global__ __launch_bounds__(256) void gate_grad_norm3d_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ feat,
                                                                const float* __restrict__ sparse, const float* __restrict__ kp,
                                                                const float* __restrict__ hist, const float* __restrict__ ahist,
                                                                const float* __restrict__ gout, const float* __restrict__ a0,
                                                                void* __restrict__ planes, float* __restrict__ gf, int B, int D,
                                                                int H, int W, int n_iter, int norm, int C = 1) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const int nch = MULTI ? C : 1;
    const size_t V = (size_t)D * H * W, total = (size_t)B * nch * V, vox = (size_t)p.b * V + p.r;   // vox: the voxel in the shared planes
    float acc[26][VEC], dC[VEC], Dh[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) Dh[i] = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;
#pragma unroll 1
    for (int c = 0; c < nch; ++c) {
        const size_t vol = ((size_t)p.b * nch + c) * V, cvox = vol + p.r;   // the channel's volume, the voxel in it
#pragma unroll
        for (int i = 0; i < VEC; ++i) dC[i] = 0.f;
#pragma unroll 1
        for (int t = 0; t < n_iter; ++t) {
            const float* at = t == n_iter - 1 ? gout : ahist + (size_t)t * total;   // A_{t+1}
            float a[VEC];
            load_vec<VEC>(at + cvox, a);
#pragma unroll
            for (int i = 0; i < VEC; ++i) dC[i] += a[i];
            if (!planes) continue;
            gate_grad_level3<VEC>(acc, a, (t == 0 ? feat : hist + (size_t)(t - 1) * total) + vol, p, D, H, W);
        }
        if (gf) {
            float a[VEC], coef[VEC];
            load_vec<VEC>(a0 + cvox, a);
            load_vec<VEC>(kp + vox, coef);
#pragma unroll
            for (int i = 0; i < VEC; ++i) a[i] = fmaf(dC[i], coef[i], a[i]);
            store_vec<VEC>(gf + cvox, a);
        }
        if (MULTI && planes && norm != CSPN_NORM_NONE) {
            float h0[VEC];
            load_vec<VEC>(feat + cvox, h0);
#pragma unroll
            for (int i = 0; i < VEC; ++i) Dh[i] = fmaf(dC[i], h0[i], Dh[i]);
        }
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
    if constexpr (!MULTI) load_vec<VEC>(feat + vox, h0);
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
            if constexpr (MULTI) acc[k][i] = u[i] * (acc[k][i] - Dh[i]);   // dwb_k
            else acc[k][i] = u[i] * (acc[k][i] - dC[i] * h0[i]);
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
    char* levels = (char*)kp + planes_bytes(total, 1);   // the workspace of backward3d()
    const Backward3dLayout L(B, 1, D, H, W, n_iter, 0);
    float* hist = (float*)(levels + L.hist);     // H_1 .. H_{n-1}
    float* ahist = (float*)(levels + L.ahist);   // A_1 .. A_{n-1}
    float* a0 = (float*)(levels + L.a0);
    void* pws = levels + L.pers;
    const bool vec = quads_ok(W, gdt, {g, gg}, {feat, sparse, gout, gf, ws});
    const bool fused = !stepwise_only && backward3d_norm_fused(g, gdt, feat, sparse, gout, gg, gf, B, D, H, W, n_iter, ws);
    const dim3 grid((unsigned)((total / (vec ? 4 : 1) + 255) / 256)), block(256);
    return with_gate_type(gdt, [&](auto gt) -> int {
        using GT = typename decltype(gt)::type;
        return with_vec(vec, [&](auto v) -> int {
            constexpr int VEC = decltype(v)::value;
            const store_t<GT>* gs = (const store_t<GT>*)g;
            hipLaunchKernelGGL((fold_norm3d_kernel<VEC, GT>), grid, block, 0, st, gs, feat, sparse, wp, cp, kp, B, D, H, W, norm);
            if (int e = check_launch("fold_norm3d_kernel")) return e;
            if (gg) {   // H_1 .. H_{n-1}: the forward step with the constant term, on w' as the gate tensor it is laid out as
                const float* src = feat;
                for (int t = 1; t < n_iter; ++t) {
                    float* dst = hist + (size_t)(t - 1) * total;
                    if (vec) step3d_direct(wp, 0, src, dst, B, D, H, W, st, cp);
                    else step3d_folded(wp, cp, 26 * V, V, src, dst, B, D, H, W, st);
                    src = dst;
                }
                if (int e = check_launch("step_const3d_kernel")) return e;   // (the text from before the two steps moved to cspn3d_stepwise.hip)
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
            hipLaunchKernelGGL((gate_grad_norm3d_kernel<VEC, GT>), grid, block, 0, st, gs, feat, sparse, kp, hist, ahist, gout, a0, planes, gf, B, D, H, W,
                               n_iter, norm, 1);
            if (int e = check_launch("gate_grad_norm3d_kernel")) return e;
            if (gg && norm != CSPN_NORM_NONE) {
                hipLaunchKernelGGL((gather_guidance3d_kernel<VEC, GT>), grid, block, 0, st, wp, gs, (store_t<GT>*)gg, B, D, H, W, norm);
                if (int e = check_launch("gather_guidance3d_kernel")) return e;
            }
            return 0;
        });
    });
}

// ---- C value channels on shared guidance (feat / gout / gf [B][C][V], sparse NULL or [B][V]) ----

// the fold the channels share, once per call: w' [B][26][V] and coef [B][V]; each channel forms its own constant term coef H_{0,c}
int fold3d_shared(const void* g, int gdt, const float* sparse, float* wp, float* kp, int B, int D, int H, int W, int norm, bool vec, hipStream_t st) {
    const size_t total = (size_t)B * D * H * W;
    const dim3 grid((unsigned)((total / (vec ? 4 : 1) + 255) / 256)), block(256);
    with_gate_type(gdt, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_vec(vec, [&](auto v) {
            constexpr int VEC = decltype(v)::value;
            hipLaunchKernelGGL((fold_norm3d_kernel<VEC, GT, false>), grid, block, 0, st, (const store_t<GT>*)g, (const float*)nullptr, sparse, wp,
                               (float*)nullptr, kp, B, D, H, W, norm);
            return 0;
        });
    });
    return check_launch("fold_norm3d_kernel");
}

// w' / dG (26 planes) and coef, then the workspace of backward3d() on C channels: the levels H_1 .. H_{n-1}, A_1 .. A_{n-1}, each [B][C][V],
// A_0 and what the persistent kernel wants
size_t backward3d_norm_multi_workspace(int B, int C, int D, int H, int W, int n_iter) {
    const size_t total = (size_t)B * D * H * W;
    return planes_bytes(total, 26) + planes_bytes(total, 1) + backward3d_workspace(B, D, H, W, n_iter, C);
}

// where the adjoint sweep of all channels is ONE launch of the transposed multi-channel instance: backward3d()'s fused multi sweep
bool backward3d_norm_multi_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, const void* gg, const float* gf,
                                 int B, int C, int D, int H, int W, int n_iter, const void* ws) {
    return quads_ok(W, gdt, {g, gg}, {feat, sparse, gout, gf, ws}) && n_iter >= 3 && persistent3d_multi_supported(B, C, D, H, W, n_iter - 1) &&
           persistent3d_multi_supported(B, C, D, H, W, n_iter);
}

// backward3d_norm() for C > 1 channels: gg is the sum over the channels, written once per element
int backward3d_norm_multi(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, void* gg, float* gf, int B, int C,
                          int D, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, bool stepwise_only) {
    const size_t V = (size_t)D * H * W, total = (size_t)B * V, level = total * C;
    float* wp = (float*)ws;
    float* kp = (float*)((char*)ws + planes_bytes(total, 26));
    char* levels = (char*)kp + planes_bytes(total, 1);   // the workspace of backward3d()
    const Backward3dLayout L(B, C, D, H, W, n_iter, 0);
    float* hist = (float*)(levels + L.hist);     // H_1 .. H_{n-1}
    float* ahist = (float*)(levels + L.ahist);   // A_1 .. A_{n-1}
    float* a0 = (float*)(levels + L.a0);
    void* pws = levels + L.pers;
    const bool vec = quads_ok(W, gdt, {g, gg}, {feat, sparse, gout, gf, ws});
    const bool fused = !stepwise_only && backward3d_norm_multi_fused(g, gdt, feat, sparse, gout, gg, gf, B, C, D, H, W, n_iter, ws);
    const dim3 grid((unsigned)((total / (vec ? 4 : 1) + 255) / 256)), block(256);
    if (int e = fold3d_shared(g, gdt, sparse, wp, kp, B, D, H, W, norm, vec, st)) return e;
    if (gg) {   // H_1 .. H_{n-1} of every channel: one launch per level, w' and coef read once for the C channels
        const float* src = feat;
        for (int t = 1; t < n_iter; ++t) {
            float* dst = hist + (size_t)(t - 1) * level;
            if (int e = step3d_shared(wp, kp, feat, src, dst, B, C, D, H, W, vec, st)) return e;
            src = dst;
        }
    }
    // the adjoint levels on w' as the gates of the Paddle contract: the transposed multi-channel instance (w' resident across the steps and
    // the channels), else backward3d()'s per-step launches, channel by channel
    if (fused) {
        if (int e = persistent3d_run(wp, gout, a0, ahist, n_iter - 1, -1, true, B, D, H, W, n_iter, pws, st, P3Options(), C)) return e;
    } else if (int e = backward3d(wp, feat, gout, nullptr, gf ? a0 : nullptr, B, D, H, W, n_iter, levels, st, true, C)) {
        return e;
    }
    return with_gate_type(gdt, [&](auto gt) -> int {
        using GT = typename decltype(gt)::type;
        return with_vec(vec, [&](auto v) -> int {
            constexpr int VEC = decltype(v)::value;
            const store_t<GT>* gs = (const store_t<GT>*)g;
            void* planes = !gg ? nullptr : (norm == CSPN_NORM_NONE ? gg : (void*)wp);
            hipLaunchKernelGGL((gate_grad_norm3d_kernel<VEC, GT, true>), grid, block, 0, st, gs, feat, sparse, kp, hist, ahist, gout, a0, planes, gf, B, D, H,
                               W, n_iter, norm, C);
            if (int e = check_launch("gate_grad_norm3d_kernel")) return e;
            if (gg && norm != CSPN_NORM_NONE) {
                hipLaunchKernelGGL((gather_guidance3d_kernel<VEC, GT>), grid, block, 0, st, wp, gs, (store_t<GT>*)gg, B, D, H, W, norm);
                if (int e = check_launch("gather_guidance3d_kernel")) return e;
            }
            return 0;
        });
    });
}

}  // namespace cspn
