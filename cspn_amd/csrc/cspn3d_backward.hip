// cspn3d_backward.hip -- backward of the 3x3x3 propagation under the Paddle contract (gates used as given, centre-sited,
// no centre term, no mask: reference cspn_paddle/README.md:54-56; the op is differentiated by the demo's optimiser,
// cspn_paddle/demo.py:65-75, `feat` has stop_gradient=False).  Kernel source of the reference op is NOT in the tree
// (parity unpinned): the arithmetic is the adjoint of oracle/cspn_oracle.c's 3D forward, checked against
// autograd of the same recurrence in tests/.
//
//   forward   H_{t+1}(p) = sum_k g_k(p) H_t(p + off_k),  t = 0 .. n-1,  H_0 = feat,  out = H_n      (zero outside the volume)
//   adjoint   A_n = dL/dout,   A_t(q) = sum_k g_k(q - off_k) A_{t+1}(q - off_k)                       dL/dfeat = A_0
//   gates     dL/dg_k(p) = sum_t A_{t+1}(p) H_t(p + off_k)
//
// Three kinds of launches, each HBM-bound streaming: the forward steps that keep H_1 .. H_{n-1} (step3d_direct_kernel of
// cspn3d_stepwise.hip, only when the gate gradient is wanted), n adjoint steps (26 gate planes + A in, A out = 112 B/voxel
// each, like a forward step), and ONE gate-gradient pass that reads the 2n value volumes and writes the 26 planes once
// (26 x 4 accumulators per thread).  A single chained call (n = 1, how the Paddle graph uses the op) therefore moves
// 28 + 28 planes: the adjoint step and the gate-gradient pass, nothing else.
#include "cspn3d_voxel.h"

namespace cspn {

namespace {

// one adjoint step: aout(q) = sum_k g_k(q - off_k) ain(q - off_k); VEC = 4 (W % 4 == 0, 16-byte aligned tensors) or 1
// fbs: floats from one volume of ain / aout to the next (V, or C V when the call's C value channels share the gates: the caller
// passes the channel's first volume).  GT: the gate storage type (cspn_gate16.h); the shifted quads of a 16-bit plane are 8-byte reads at
// 2-byte alignment (ld4gu)
template <int VEC, class GT>
__global__ __launch_bounds__(256) void adjoint3d_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ ain,
                                                         float* __restrict__ aout, int B, int D, int H, int W, size_t fbs) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t HW = (size_t)H * W, V = (size_t)D * HW;
    const float* ab = ain + (size_t)p.b * fbs;
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
#pragma unroll
    for (int n = 0; n < 9; ++n) {   // source rows (z - dz, y - dy)
        const int dz = row_dz3(n), dy = row_dy3(n);
        float a[VEC + 2];   // ain at columns x-1 .. x+VEC of the source row
        if (!load_row3<VEC>(ab, p, -dz, -dy, D, H, W, a)) continue;   // (a row outside the volume has no gates to read either)
        const size_t ro = ((size_t)(p.z - dz) * H + (p.y - dy)) * W;
        for_taps3(n, [&](int k, int dx) {   // the source voxel of column x + i is x + i - dx
            const store_t<GT>* gp = gb + (size_t)k * V + ro + p.x - dx;
            float w[VEC];
            if (VEC == 4 && p.x - dx >= 0 && p.x - dx + 3 < W) {
                const float4 q = ld4gu<GT>(gp);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const int xs = p.x + i - dx;
                    w[i] = (xs >= 0 && xs < W) ? widen<GT>(gp[i]) : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) acc[i] = fmaf(w[i], a[1 + i - dx], acc[i]);
        });
    }
    store_vec<VEC>(aout + (size_t)p.b * fbs + p.r, acc);
}

// dL/dg_k(p) = sum_c sum_t A^c_{t+1}(p) H^c_t(p + off_k) over the C value channels that share the gates (reference
// cspn_paddle/README.md:56; C = 1: the plain op).  Every value tensor is [B][C][V]; level t of channel c: H_0 = feat,
// H_t = hist + (t-1) total; A_n = gout, A_t = ahist + (t-1) total (t = 1 .. n-1), total = B C V.  The sums are float32 whatever the
// type GT of gg: a 16-bit gradient is rounded once, at its store
template <int VEC, class GT>
__global__ __launch_bounds__(256) void gate_grad3d_kernel(const float* __restrict__ feat, const float* __restrict__ hist,
                                                           const float* __restrict__ ahist, const float* __restrict__ gout,
                                                           store_t<GT>* __restrict__ gg, int B, int D, int H, int W, int n_iter, int C) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t HW = (size_t)H * W, V = (size_t)D * HW, total = (size_t)B * C * V;
    float acc[26][VEC];
#pragma unroll
    for (int k = 0; k < 26; ++k)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[k][i] = 0.f;
#pragma unroll 1
    for (int ct = 0; ct < C * n_iter; ++ct) {
        const int cch = ct / n_iter, t = ct - cch * n_iter;
        const size_t vol = ((size_t)p.b * C + cch) * V, vox = vol + p.r;
        const float* ht = (t == 0 ? feat : hist + (size_t)(t - 1) * total) + vol;
        const float* at = t == n_iter - 1 ? gout : ahist + (size_t)t * total;   // A_{t+1}
        float a[VEC];
        load_vec<VEC>(at + vox, a);
        gate_grad_level3<VEC>(acc, a, ht, p, D, H, W);
    }
    store_t<GT>* o = gg + (size_t)p.b * 26 * V + p.r;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        if (VEC == 4) st4g<GT>(o + (size_t)k * V, acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
        else o[(size_t)k * V] = narrow<GT>(acc[k][0]);
    }
}

// the exact widening of a 16-bit gate tensor into float32, streaming: what the transposed persistent instance (ADJ) reads, since its
// prologue takes planes shifted by one element in x and has no 16-bit form
template <class GT>
__global__ __launch_bounds__(256) void widen_gates_kernel(const store_t<GT>* __restrict__ g, float* __restrict__ w, size_t n4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) *reinterpret_cast<float4*>(w + 4 * i) = ld4g<GT>(g + 4 * i);
}

}  // namespace

// n floats, n % 4 == 0, g 8-byte and w 16-byte aligned
int widen_gates(const void* g, int gdt, float* w, size_t n, hipStream_t st) {
    with_gate_type(gdt, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        if constexpr (!std::is_same<GT, float>::value)
            hipLaunchKernelGGL(widen_gates_kernel<GT>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, (const store_t<GT>*)g, w, n / 4);
        return 0;
    });
    return check_launch("widen_gates_kernel");
}

// the fused sweeps' conditions on the shape (the pointers' alignment is the call's)
static bool fused3d_shape(int B, int C, int D, int H, int W, int n_iter) {
    return (W % 4) == 0 && n_iter >= 3 &&
           (C == 1 ? persistent3d_supported(B, D, H, W, n_iter - 1) && persistent3d_supported(B, D, H, W, n_iter)
                   : persistent3d_multi_supported(B, C, D, H, W, n_iter - 1) && persistent3d_multi_supported(B, C, D, H, W, n_iter));
}

// levels kept: H_1 .. H_{n-1} and A_1 .. A_{n-1} (A_0 goes to grad_feat, or to one more volume when the caller does not want it); then the
// workspace of the persistent kernel (fused sweeps, n >= 3); gdt != 0 (16-bit gates): where the fused sweeps can take the call, the float32
// copy of the gates the transposed sweep reads follows
Backward3dLayout::Backward3dLayout(int B, int C, int D, int H, int W, int n_iter, int gdt) {
    const size_t level = sizeof(float) * (size_t)B * C * D * H * W, kept = n_iter > 0 ? n_iter - 1 : 0;
    hist = 0;
    ahist = kept * level;
    a0 = 2 * kept * level;
    pers = round256(a0 + level);
    bytes = pers + persistent3d_workspace(B, D, H, W);
    wide = 0;
    if (gdt && fused3d_shape(B, C, D, H, W, n_iter)) {
        wide = round256(bytes);
        bytes = wide + round256(26 * sizeof(float) * (size_t)B * D * H * W);
    }
}

size_t backward3d_workspace(int B, int D, int H, int W, int n_iter, int C, int gdt) { return Backward3dLayout(B, C, D, H, W, n_iter, gdt).bytes; }

// C > 1 (round 5; reference cspn_paddle/README.md:56, trained through at demo.py:65-75): feat / gout / gf hold C value channels per
// volume on shared gates, gg is the gate gradient summed over the channels.  Fused sweeps: ONE level-keeping forward launch and ONE
// transposed launch of the persistent kernel for all channels (its MULTI instantiations: the gates of a chunk stay in the registers
// while the steps run for channel after channel), then one gate-gradient pass that loops over the channels and writes the 26
// planes once.  Otherwise one launch per step and channel.
// gdt: the storage type of g and gg (0 float32, CSPN_DTYPE_F16, CSPN_DTYPE_BF16).  16-bit gates are read as they are by every kernel but the
// transposed persistent sweep, which reads one exact float32 copy made in the workspace; gg is the float32 sum rounded once at its store
int backward3d(const void* g, const float* feat, const float* gout, void* gg, float* gf, int B, int D, int H, int W,
               int n_iter, void* ws, hipStream_t st, bool stepwise_only, int C, int gdt) {
    const size_t V = (size_t)D * H * W, total = (size_t)B * C * V, fbs = (size_t)C * V;
    const Backward3dLayout L(B, C, D, H, W, n_iter, gdt);
    float* hist = (float*)((char*)ws + L.hist);     // H_1 .. H_{n-1}
    float* ahist = (float*)((char*)ws + L.ahist);   // A_1 .. A_{n-1}
    float* a0 = gf ? gf : (float*)((char*)ws + L.a0);
    void* pws = (char*)ws + L.pers;
    const bool vec = quads_ok(W, gdt, {g, gg}, {feat, gout, gf, ws});
    const dim3 grid((unsigned)(((size_t)B * V / (vec ? 4 : 1) + 255) / 256)), block(256);   // threads cover ONE channel's B volumes
    // fused sweeps: the persistent kernel (gates read once per sweep, resident in registers across the steps) in its
    // level-keeping and transposed variants -- forward H_1 .. H_{n-1} (n - 1 steps, the last one "out" = H_{n-1}), adjoint
    // A_{n-1} .. A_0 (n steps).  One launch per step otherwise.
    const bool fused = vec && !stepwise_only && (gdt ? L.wide != 0 : fused3d_shape(B, C, D, H, W, n_iter));   // (the layout has asked already)
    if (fused) {
        if (gg)
            if (int e = persistent3d_run(g, feat, hist + (size_t)(n_iter - 2) * total, hist, -1, 1, false, B, D, H, W, n_iter - 1, pws, st, P3Options(), C, gdt))
                return e;
        // step it of the adjoint run produces A_{n-it}: volume n - it - 1 of ahist; the last one (A_0) is its "out"
        if (gf || gg) {
            const void* ga = g;
            if (gdt) {
                float* wide = (float*)((char*)ws + L.wide);
                if (int e = widen_gates(g, gdt, wide, 26 * (size_t)B * V, st)) return e;
                ga = wide;
            }
            if (int e = persistent3d_run(ga, gout, a0, ahist, n_iter - 1, -1, true, B, D, H, W, n_iter, pws, st, P3Options(), C)) return e;
        }
    }
    return with_gate_type(gdt, [&](auto gt) -> int {
        using GT = typename decltype(gt)::type;
        return with_vec(vec, [&](auto v) -> int {
            constexpr int VEC = decltype(v)::value;
            const store_t<GT>* gs = (const store_t<GT>*)g;
            if (!fused)   // one launch per step and channel where the sweeps above did not run
                for (int c = 0; c < C; ++c) {
                    const size_t co = (size_t)c * V;
                    if (gg) {   // the value levels the gate gradient multiplies with
                        const float* src = feat + co;
                        for (int t = 1; t < n_iter; ++t) {
                            float* dst = hist + (size_t)(t - 1) * total + co;
                            if (int e = vec && C == 1 ? step3d_direct(g, gdt, src, dst, B, D, H, W, st) : step3d_scalar(g, gdt, src, dst, B, D, H, W, fbs, st))
                                return e;
                            src = dst;
                        }
                        if (int e = check_launch("3D forward levels")) return e;
                    }
                    // adjoint levels A_{n-1} .. A_1 (kept only if the gate gradient needs them: otherwise two volumes would do, but the
                    // workspace is sized for the general call) and A_0
                    const float* src = gout + co;
                    for (int t = n_iter - 1; t >= 0; --t) {
                        float* dst = (t == 0 ? a0 : ahist + (size_t)(t - 1) * total) + co;
                        if (t == 0 && !gf) break;   // A_0 is only the feature gradient
                        hipLaunchKernelGGL((adjoint3d_kernel<VEC, GT>), grid, block, 0, st, gs, src, dst, B, D, H, W, fbs);
                        src = dst;
                    }
                    if (int e = check_launch("adjoint3d_kernel")) return e;
                }
            if (gg) {
                hipLaunchKernelGGL((gate_grad3d_kernel<VEC, GT>), grid, block, 0, st, feat, hist, ahist, gout, (store_t<GT>*)gg, B, D, H, W, n_iter, C);
                if (int e = check_launch("gate_grad3d_kernel")) return e;
            }
            return 0;
        });
    });
}

}  // namespace cspn
