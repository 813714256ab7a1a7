// cspn3d_stepwise.hip -- 3x3x3 propagation (26 neighbours), one launch per iteration: the fold, and the three forward steps every 3D file
// launches (step3d_kernel on folded planes, step3d_direct_kernel on a gate tensor four voxels a thread, step3d_scalar_kernel on a gate
// tensor of any shape and alignment).
// API surface: reference cspn_paddle/demo.py:41-43,50-52 (fluid.layers.affinity_propagate,
// kernel source NOT in the reference tree -> parity unpinned; semantics = the 3D
// generalisation of cspn_pytorch/models/cspn.py:42-172, see oracle/cspn_oracle.c).
// Channel order and the neighbourhood helpers: cspn3d_voxel.h.
// At the end: the normalising / masked modes for C value channels on shared guidance (step3d_shared_kernel, forward3d_norm_multi).
#include "cspn3d_voxel.h"

namespace cspn {

// wf: [27][B*D*H*W] (26 folded weights + c').  GT: the gate storage type (cspn_gate16.h).  A 16-bit gate comes here in every mode: with
// norm NONE and no mask (a misaligned gate tensor of the Paddle contract) folding is the exact widening; in the normalising and masked modes
// (cspn3d_forward_norm_g16) each gate is widened where it is read and the sums, divisions and products are the float32 ones in the same order.
// fold_norm3d_kernel (cspn3d_norm_backward.hip) is the same fold, VEC voxels a thread, into another layout.  The two stay two: this one keeps
// its single bounds test per gate and its scalar registers -- written over the shared load_G it ran 2 % slower at config 5's volume
// (profiles/3d_stepwise_refactor.md) -- and they form c' differently, here (1 - m) ((1 - sigma) h0) + m h0, there ((1 - m) (1 - sigma) + m) h0:
// the two round differently and each output stays bitwise what it has always been
template <class GT>
__global__ __launch_bounds__(256) void fold3d_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ feat,
                                                      const float* __restrict__ sparse, float* __restrict__ wf,
                                                      int B, int D, int H, int W, int norm) {
    const Pos<1> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, total = (size_t)B * V, idx = (size_t)p.b * V + p.r;
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V;
    float G[26], S = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        float v;
        if (norm == CSPN_NORM_NONE) {
            v = widen<GT>(gb[k * V + p.r]);
        } else {
            const int zz = p.z + dz3(k), yy = p.y + dy3(k), xx = p.x + dx3(k);
            v = 0.f;
            if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W)
                v = widen<GT>(gb[k * V + ((size_t)zz * H + yy) * W + xx]);
            if (norm == CSPN_NORM_8SUM_ABS) v = fabsf(v);
        }
        G[k] = v;
        S += fabsf(v);
    }
    float sigma = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        if (norm != CSPN_NORM_NONE) G[k] = G[k] / S;
        sigma += G[k];
    }
    const float h0 = feat[idx];
    const float m = sparse ? signf(sparse[idx]) : 0.f;
    const float om = 1.f - m;
    float c = (norm == CSPN_NORM_NONE) ? 0.f : (1.f - sigma) * h0;
    if (sparse) {
        c = om * c + m * h0;
#pragma unroll
        for (int k = 0; k < 26; ++k) G[k] *= om;
    }
#pragma unroll
    for (int k = 0; k < 26; ++k) wf[k * total + idx] = G[k];
    wf[26 * total + idx] = c;
}

// one step on folded planes: hout(p) = c(p) + sum_k w_k(p) hin(p + off_k), one voxel a thread.  w_k(p) of batch b at w + b bs + k ps + r,
// c [B][V]: (bs, ps) = (V, B V) for the forward's [27][B V] planes (c = plane 26), (26 V, V) for the backward's gate-tensor layout [B][26][V]
__global__ __launch_bounds__(256) void step3d_kernel(const float* __restrict__ w, const float* __restrict__ c, const float* __restrict__ hin,
                                                      float* __restrict__ hout, int B, int D, int H, int W, size_t bs, size_t ps) {
    const Pos<1> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, vox = (size_t)p.b * V + p.r;
    const float* hb = hin + (size_t)p.b * V;
    const float* wb = w + (size_t)p.b * bs + p.r;
    float acc = c[vox];
#pragma unroll
    for (int n = 0; n < 9; ++n) {   // neighbour rows (z + dz, y + dy); three x-taps each
        float h[3];                 // hin at columns x-1 .. x+1 of the row, zero outside the volume
        load_row3<1>(hb, p, row_dz3(n), row_dy3(n), D, H, W, h);
        for_taps3(n, [&](int k, int dx) { acc = fmaf(wb[(size_t)k * ps], h[1 + dx], acc); });
    }
    hout[vox] = acc;
}

// The Paddle contract (norm_type NONE, no sparse): gates are used as given, centre-sited, no centre term
// (reference cspn_paddle/README.md:54-56, demo.py:41-52).  One iteration then needs exactly the algorithmic traffic of a
// single propagation step -- 26 gates + value in, value out = 112 B/voxel -- so it reads the gate tensor directly: no
// fold pass, no coefficient planes.  4 voxels per thread along x (16-byte loads of the gate planes; 8-byte loads of fp16 / bf16 planes,
// widened as they arrive).
// CONST: the accumulator starts at cp(p) instead of 0 -- the step of the normalising / masked backward on its folded planes
// (g = w' [B][26][V] float32, cp = c' [B][V]): hout(p) = c'(p) + sum_k w'_k(p) hin(p + off_k)
template <class GT, bool CONST>
__global__ __launch_bounds__(256) void step3d_direct_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ hin,
                                                             float* __restrict__ hout, int B, int D, int H, int W4,
                                                             const float* __restrict__ cp) {
    const int W = 4 * W4;
    const Pos<4> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W, vox = (size_t)p.b * V + p.r;
    const float* hb = hin + (size_t)p.b * V;
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V + p.r;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (CONST) load_vec<4>(cp + vox, acc);
#pragma unroll
    for (int n = 0; n < 9; ++n) {   // the 9 neighbour rows (dz, dy); three x-taps each
        float h[6];
        load_row3<4>(hb, p, row_dz3(n), row_dy3(n), D, H, W, h);
        for_taps3(n, [&](int k, int dx) {
            float w[4];
            load_gvec<4, GT>(gb + (size_t)k * V, w);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(w[i], h[1 + i + dx], acc[i]);
        });
    }
    store_vec<4>(hout + vox, acc);
}

// forward step on a gate tensor for the shapes / alignments step3d_direct_kernel does not take.  fbs: floats from one volume of hin / hout
// to the next (V, or C V when C value channels share the gates).
// It SKIPS a tap whose neighbour lies outside the volume; the other step kernels multiply the gate by a zero.  The two differ where a gate
// at a face of the volume is NaN or infinite (0 x NaN = NaN): that is the behaviour the scalar path has always had, and it is kept
namespace {
template <class GT>
__global__ __launch_bounds__(256) void step3d_scalar_kernel(const store_t<GT>* __restrict__ g, const float* __restrict__ hin,
                                                             float* __restrict__ hout, int B, int D, int H, int W, size_t fbs) {
    const Pos<1> p(B, D, H, W);
    if (!p.ok) return;
    const size_t HW = (size_t)H * W, V = (size_t)D * HW;
    const float* hb = hin + (size_t)p.b * fbs;
    const store_t<GT>* gb = g + (size_t)p.b * 26 * V + p.r;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 26; ++k) {
        const int c = ch3(k);   // (p.z + 1 - c / 9, not p.z + dz3(k): the other association moves this kernel's blocks)
        const int zz = p.z + 1 - c / 9, yy = p.y + 1 - (c / 3) % 3, xx = p.x + 1 - c % 3;
        if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W)
            acc = fmaf(widen<GT>(gb[(size_t)k * V]), hb[((size_t)zz * H + yy) * W + xx], acc);
    }
    hout[(size_t)p.b * fbs + p.r] = acc;
}
}  // namespace

// one step of the Paddle contract for other files (the backward keeps the value levels): W % 4 == 0, 16-byte aligned tensors (a 16-bit
// gate tensor: 8-byte aligned); gdt: the gate storage type (0 float32, CSPN_DTYPE_F16, CSPN_DTYPE_BF16).  cp != NULL (float32 gates
// only): the step with the constant term cp
int step3d_direct(const void* g, int gdt, const float* hin, float* hout, int B, int D, int H, int W, hipStream_t st, const float* cp) {
    const size_t total = (size_t)B * D * H * W;
    const dim3 grid((unsigned)((total / 4 + 255) / 256)), block(256);
    if (cp) {
        hipLaunchKernelGGL((step3d_direct_kernel<float, true>), grid, block, 0, st, (const float*)g, hin, hout, B, D, H, W / 4, cp);
        return 0;
    }
    return with_gate_type(gdt, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        hipLaunchKernelGGL((step3d_direct_kernel<GT, false>), grid, block, 0, st, (const store_t<GT>*)g, hin, hout, B, D, H, W / 4, cp);
        return 0;
    });
}

int step3d_folded(const float* w, const float* c, size_t bs, size_t ps, const float* hin, float* hout, int B, int D, int H, int W, hipStream_t st) {
    const size_t total = (size_t)B * D * H * W;
    hipLaunchKernelGGL(step3d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, c, hin, hout, B, D, H, W, bs, ps);
    return 0;
}

int step3d_scalar(const void* g, int gdt, const float* hin, float* hout, int B, int D, int H, int W, size_t fbs, hipStream_t st) {
    const size_t total = (size_t)B * D * H * W;
    return with_gate_type(gdt, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        hipLaunchKernelGGL(step3d_scalar_kernel<GT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const store_t<GT>*)g, hin, hout, B, D,
                           H, W, fbs);
        return 0;
    });
}

size_t stepwise3d_workspace(int B, int D, int H, int W, int n_iter) {
    (void)n_iter;
    // large enough for every mode: the 27 fold planes + what the persistent kernel wants (two value volumes = the ping-pong of
    // the per-step path, its exchange buffers)
    return 27 * (size_t)B * D * H * W * sizeof(float) + persistent3d_workspace(B, D, H, W);
}

// what the chosen path really needs: the Paddle contract (gates used as given, no mask) keeps two value volumes (+ the sync
// words of the persistent kernel), the folding modes 27 coefficient planes more
size_t forward3d_workspace(int B, int D, int H, int W, int n_iter, int norm, bool has_sparse) {
    (void)n_iter;
    if (norm == CSPN_NORM_NONE && !has_sparse && (W % 4) == 0) return persistent3d_workspace(B, D, H, W);
    return stepwise3d_workspace(B, D, H, W, n_iter);
}

// algo: 0 auto, 1 one launch per step, 2 persistent (gates resident across steps)
// gdt: the gate storage type (which modes take CSPN_DTYPE_F16 / CSPN_DTYPE_BF16 is the entry point's decision: cspn3d_forward_g16_algo the
// Paddle contract only, cspn3d_forward_norm_g16 every mode).  The dispatch is the float32 one with the gate pointer's 16-byte condition at 8
// bytes; the folding path reads the gates element by element, so their alignment plays no part in it
int stepwise3d_forward(const void* g, const float* feat, const float* sparse, float* out, int B, int D, int H,
                       int W, int n_iter, int norm, void* ws, hipStream_t st, int algo, int gdt) {
    const size_t V = (size_t)D * H * W, total = (size_t)B * V;
    float* wf = (float*)ws;
    const bool direct = norm == CSPN_NORM_NONE && sparse == nullptr && quads_ok(W, gdt, {g}, {feat, out, ws});
    if (algo == 2 && direct && !persistent3d_supported(B, D, H, W, n_iter)) {
        set_error("persistent 3D kernel does not take this call (needs W %% 4 == 0, 16-byte aligned tensors, 2 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    if (direct && algo != 1 && persistent3d_supported(B, D, H, W, n_iter))
        return persistent3d_forward(g, feat, out, B, D, H, W, n_iter, ws, st, gdt);
    if (direct) {
        float* pp[2] = {wf, wf + total};
        const float* src = feat;
        for (int it = 0; it < n_iter; ++it) {
            float* dst = (it == n_iter - 1) ? out : pp[it & 1];
            step3d_direct(g, gdt, src, dst, B, D, H, W, st);
            src = dst;
        }
        return check_launch("step3d_direct_kernel");
    }
    float* ping[2] = {wf + 27 * total, wf + 28 * total};
    with_gate_type(gdt, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        hipLaunchKernelGGL(fold3d_kernel<GT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const store_t<GT>*)g, feat, sparse, wf, B, D,
                           H, W, norm);
        return 0;
    });
    if (int e = check_launch("fold3d_kernel")) return e;
    // the normalising / masked modes fused: H_{t+1} = c' + sum_k w'_k H_t(p + off_k) with the folded planes resident in the
    // persistent kernel's registers (c' in LDS): fold once, then one pass over the 27 planes for all steps
    const bool aligned = quads_ok(W, 0, {}, {feat, out, ws});
    if (algo == 2 && !(aligned && persistent3d_supported(B, D, H, W, n_iter))) {
        set_error("persistent 3D kernel does not take this call (needs W %% 4 == 0, 16-byte aligned tensors, 2 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    if (algo != 1 && aligned && persistent3d_supported(B, D, H, W, n_iter))
        return persistent3d_forward_folded(wf, feat, out, B, D, H, W, n_iter, wf + 27 * total, st);
    const float* src = feat;
    for (int it = 0; it < n_iter; ++it) {
        float* dst = (it == n_iter - 1) ? out : ping[it & 1];
        step3d_folded(wf, wf + 26 * total, V, total, src, dst, B, D, H, W, st);
        src = dst;
    }
    return check_launch("step3d_kernel");
}

// ---- C value channels on shared guidance in the normalising / masked modes (feat / out [B][C][V], sparse NULL or [B][V]) ----

// one step of all C channels on the shared folded planes wp = w' [B][26][V] and kp = coef [B][V] (fold3d_shared):
// hout_c(p) = coef(p) h0_c(p) + sum_k w'_k(p) hin_c(p + off_k).  The 26 x VEC weights and coef of the thread's voxels are loaded once and
// stay in registers while the channels go by: 108 + 12 C bytes a voxel where C single-channel steps move 116 C
namespace {
template <int VEC>
__global__ __launch_bounds__(256) void step3d_shared_kernel(const float* __restrict__ wp, const float* __restrict__ kp, const float* __restrict__ h0,
                                                             const float* __restrict__ hin, float* __restrict__ hout, int B, int C, int D, int H,
                                                             int W) {
    const Pos<VEC> p(B, D, H, W);
    if (!p.ok) return;
    const size_t V = (size_t)D * H * W;
    const float* wb = wp + (size_t)p.b * 26 * V + p.r;
    float w[26][VEC], coef[VEC];
#pragma unroll
    for (int k = 0; k < 26; ++k) load_vec<VEC>(wb + (size_t)k * V, w[k]);
    load_vec<VEC>(kp + (size_t)p.b * V + p.r, coef);
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        const size_t vol = ((size_t)p.b * C + c) * V;
        float acc[VEC];
        load_vec<VEC>(h0 + vol + p.r, acc);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] *= coef[i];
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            float h[VEC + 2];
            load_row3<VEC>(hin + vol, p, row_dz3(n), row_dy3(n), D, H, W, h);
            for_taps3(n, [&](int k, int dx) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) acc[i] = fmaf(w[k][i], h[1 + i + dx], acc[i]);
            });
        }
        store_vec<VEC>(hout + vol + p.r, acc);
    }
}
}  // namespace

// vec: W % 4 == 0 and 16-byte aligned tensors (four voxels a thread), else one voxel a thread
int step3d_shared(const float* wp, const float* kp, const float* h0, const float* hin, float* hout, int B, int C, int D, int H, int W, bool vec,
                  hipStream_t st) {
    const size_t total = (size_t)B * D * H * W;
    const dim3 grid((unsigned)((total / (vec ? 4 : 1) + 255) / 256)), block(256);
    with_vec(vec, [&](auto v) {
        hipLaunchKernelGGL(step3d_shared_kernel<decltype(v)::value>, grid, block, 0, st, wp, kp, h0, hin, hout, B, C, D, H, W);
        return 0;
    });
    return check_launch("step3d_shared_kernel");
}

// w' (26 planes), coef, two levels [B][C][V] (the ping-pong of the per-step route), what the persistent kernel wants
static size_t level_bytes(int B, int C, int D, int H, int W) { return round256(sizeof(float) * (size_t)B * C * D * H * W); }

size_t forward3d_norm_multi_workspace(int B, int C, int D, int H, int W, int n_iter) {
    (void)n_iter;
    const size_t total = (size_t)B * D * H * W;
    return round256(26 * sizeof(float) * total) + round256(sizeof(float) * total) + 2 * level_bytes(B, C, D, H, W) + persistent3d_workspace(B, D, H, W);
}

// where the steps of all channels are ONE launch of the persistent kernel on the resident w' and coef
bool forward3d_norm_multi_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* out, int B, int C, int D, int H, int W,
                                int n_iter, const void* ws) {
    return quads_ok(W, gdt, {g}, {feat, sparse, out, ws}) && persistent3d_multi_supported(B, C, D, H, W, n_iter);
}

// every mode (NONE without a mask: coef = 0); algo as stepwise3d_forward
int forward3d_norm_multi(const void* g, int gdt, const float* feat, const float* sparse, float* out, int B, int C, int D, int H, int W, int n_iter,
                         int norm, void* ws, hipStream_t st, int algo) {
    const size_t total = (size_t)B * D * H * W;
    float* wp = (float*)ws;
    float* kp = (float*)((char*)ws + round256(26 * sizeof(float) * total));
    char* lev = (char*)kp + round256(sizeof(float) * total);
    float* pp[2] = {(float*)lev, (float*)(lev + level_bytes(B, C, D, H, W))};
    void* pws = lev + 2 * level_bytes(B, C, D, H, W);
    const bool vec = quads_ok(W, gdt, {g}, {feat, sparse, out, ws});
    const bool fused = forward3d_norm_multi_fused(g, gdt, feat, sparse, out, B, C, D, H, W, n_iter, ws);
    if (algo == 2 && !fused) {
        set_error("persistent 3D kernel does not take this call (needs W %% 4 == 0, 16-byte aligned tensors, 2 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    if (int e = fold3d_shared(g, gdt, sparse, wp, kp, B, D, H, W, norm, vec, st)) return e;
    if (algo != 1 && fused) return persistent3d_forward_shared(wp, kp, feat, out, B, C, D, H, W, n_iter, pws, st);
    const float* src = feat;
    for (int it = 0; it < n_iter; ++it) {
        float* dst = (it == n_iter - 1) ? out : pp[it & 1];
        if (int e = step3d_shared(wp, kp, feat, src, dst, B, C, D, H, W, vec, st)) return e;
        src = dst;
    }
    return 0;
}

}  // namespace cspn
