// cspn2d_backward.hip -- gradient of Affinity_Propagate.forward (reference cspn_pytorch/models/cspn.py:42-83) with respect
// to guidance and blur_depth: what torch autograd computes when reference train.py:196-198 back-propagates through the
// module.
//
// Forward, folded (cspn2d_stepwise.hip):  H_{t+1} = c' + sum_k w'_k * shift_k(H_t),  w'_k = (1-m) w_k,
//   c' = (1-m)(1-sigma) H_0 + m H_0,  w_k = G_k / S,  S = sum_j |G_j|,  G_k(p) = g~_k(p + off_k),  sigma = sum_k w_k.
// Adjoint:  A_N = dL/dout,   A_t(p) = sum_k (w'_k A_{t+1})(p - off_k)          (bwd_step_kernel, N launches)
//           dW'_k(p) = sum_t A_{t+1}(p) H_t(p + off_k),   dC(p) = sum_t A_{t+1}(p)   (bwd_final_kernel, from the two histories)
//           dL/dw_k = (1-m)(dW'_k - dC H_0);   dL/dH_0 = A_0 + dC ((1-m)(1-sigma) + m)
//           dL/dG_k = dL/dw_k / S - sign(G_k) (sum_j dL/dw_j G_j) / S^2          (torch: d|x|/dx = sign(x), 0 at 0)
//           dL/dg_k(p + off_k) = dL/dG_k(p)  [* sign(g) for '8sum_abs'];  elements no pixel reads get 0.
// CSPN_NORM_PRENORM (round 6): `guidance` is the reference's gate_wb (cspn.py:85-144), w_k(p) = wb_k(p) at the pixel itself: the chain ends at
//           dL/dwb_k = (1-m)(dW'_k - dC H_0),   dL/dH_0 = A_0 + dC ((1-m)(1 - sum_k wb_k) + m).
// Passes of 4, 8 .. 24 iterations on images the ring kernel takes: two sweeps of that kernel (forward keeping H_4, H_8 .. H_20 and the
// folded coefficients, adjoint keeping A_20 .. A_4) + bwd_final_mx_kernel, which recomputes the levels in between tile by tile and ends in
// bwd_epilogue4 (four columns a thread, v_rcp_f32).  Everything else: fold + one launch per step for both recursions (every level kept) +
// bwd_final_kernel, one pixel a thread on the helpers of cspn2d_pixel.h (IEEE division).
#include <cstdlib>
#include <type_traits>

#include "cspn2d_pixel.h"

namespace cspn {

// from cspn2d_stepwise.hip
__global__ void fold2d_kernel(const float* __restrict__ g, const float* __restrict__ blur, const float* __restrict__ sparse,
                              float* __restrict__ wf, int B, int H, int W, int norm);
__global__ void step2d_kernel(const float* __restrict__ wf, const float* __restrict__ hin, float* __restrict__ hout, int B,
                              int H, int W);

namespace {

// wt_k(p) = w'_k(p - off_k) (0 outside): the adjoint stencil then reads its eight coefficient planes at p itself, like
// the forward step does
__global__ __launch_bounds__(256) void transpose_w_kernel(const float* __restrict__ wf, float* __restrict__ wt, int B, int H,
                                                           int W) {
    const size_t HW = (size_t)H * W, total = (size_t)B * HW;
    const Pixel p(B, H, W);
    if (!p.ok) return;
    for_taps2([&](int k, int dy, int dx) {
        wt[k * total + p.idx] = load_tap2(wf + k * total + (size_t)p.b * HW, p.y, p.x, -dy, -dx, H, W);
    });
}

// A_t(p) = sum_k wt_k(p) A_{t+1}(p - off_k)  (its own tap loop, as step2d_kernel: see there)
__global__ __launch_bounds__(256) void bwd_step_kernel(const float* __restrict__ wt, const float* __restrict__ ain,
                                                        float* __restrict__ aout, int B, int H, int W) {
    const size_t HW = (size_t)H * W, total = (size_t)B * HW;
    const Pixel p(B, H, W);
    if (!p.ok) return;
    const float* ab = ain + (size_t)p.b * HW;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int yy = p.y - dy2(k), xx = p.x - dx2(k);
        float a = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) a = ab[(size_t)yy * W + xx];
        acc = fmaf(wt[k * total + p.idx], a, acc);
    }
    aout[p.idx] = acc;
}

// final pass of the stepwise sweeps (every level kept): hh = H_1 .. H_{N-1} (H_0 = blur), ah = A_0 .. A_{N-1}
__global__ __launch_bounds__(256) void bwd_final_kernel(const float* __restrict__ g, const float* __restrict__ blur,
                                                         const float* __restrict__ sparse, const float* __restrict__ hh,
                                                         const float* __restrict__ ah,
                                                         const float* __restrict__ gout,
                                                         float* __restrict__ gg, float* __restrict__ gb, int B, int H, int W,
                                                         int n_iter, int norm) {
    const size_t HW = (size_t)H * W, total = (size_t)B * HW;
    const Pixel p(B, H, W);
    if (!p.ok) return;
    const size_t idx = p.idx, base = (size_t)p.b * HW;
    const int r = p.r;
    const Nbrs n(p.y, p.x, r, H, W);
    float dW[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, dC = 0.f;
    for (int t = 0; t < n_iter; ++t) {
        float a;
        if (t + 1 == n_iter) a = gout[idx];
        else a = ah[(size_t)(t + 1) * total + idx];
        const float* ht = (t == 0) ? blur : hh + (size_t)(t - 1) * total;
        dC += a;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float hv = 0.f;
            if (n.ok[k]) hv = ht[base + n.off[k]];
            dW[k] = fmaf(a, hv, dW[k]);
        }
    }
    const float h0 = blur[idx];
    const float m = sparse ? signf(sparse[idx]) : 0.f;
    const float om = 1.f - m;
    const float a0 = ah[idx];
    const float* gbp = g + (size_t)p.b * 8 * HW;
    float* ggp = gg ? gg + (size_t)p.b * 8 * HW : nullptr;
    if (norm == CSPN_NORM_NONE) {  // gates used as given, centre-sited, no centre term: c' = m H_0
        if (gb) gb[idx] = a0 + dC * m;
        if (gg) {
#pragma unroll
            for (int k = 0; k < 8; ++k) ggp[k * HW + r] = om * dW[k];
        }
        return;
    }
    if (norm == CSPN_NORM_PRENORM) {  // the planes are the reference's gate_wb, read at the pixel itself: w'_k = (1-m) wb_k, c' = ((1-m)(1-sigma) + m) H_0
        float sigma = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) sigma += gbp[k * HW + r];
        if (gb) gb[idx] = a0 + dC * (om * (1.f - sigma) + m);
        if (gg) {
#pragma unroll
            for (int k = 0; k < 8; ++k) ggp[k * HW + r] = om * (dW[k] - dC * h0);
        }
        return;
    }
    float G[8], raw[8], dw[8], sigma = 0.f;
    const float S = gather_gates2(gbp, HW, n, norm, G, raw);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        sigma += G[k] / S;
        dw[k] = om * (dW[k] - dC * h0);
    }
    if (gb) gb[idx] = a0 + dC * (om * (1.f - sigma) + m);
    if (gg) norm_adjoint2(dw, G, raw, S, n, p.y, p.x, r, ggp, HW, H, W, norm);
}

// ---- helpers of the final pass of the assembly sweeps: one group of 4 columns per thread ------------------------------
__device__ __forceinline__ float dpp_shr1(float v) {   // within each row of 16 lanes: lane i <- lane i-1 (first lane: 0)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));   // row_shr:1
}
__device__ __forceinline__ float dpp_shl1(float v) {   // within each row of 16 lanes: lane i <- lane i+1 (last lane: 0)
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x101, 0xf, 0xf, true));   // row_shl:1
}
__device__ __forceinline__ float4 ld4u(const float* p) {   // 16 bytes, 4-byte aligned
    float4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void st4u(float* p, float4 v) { __builtin_memcpy(p, &v, 16); }
// dL/dguidance of channels on shared guidance (cspn2d_backward_multi_f32): channel 0 stores, every later channel adds its part
__device__ __forceinline__ void st4u_acc(float* p, float4 v, bool acc) {
    if (acc) { const float4 o = ld4u(p); v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w); }
    st4u(p, v);
}
__device__ __forceinline__ void st4a_acc(float* p, float4 v, bool acc) {   // 16-byte aligned
    if (acc) { const float4 o = *reinterpret_cast<const float4*>(p); v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w); }
    *reinterpret_cast<float4*>(p) = v;
}

// ---- the end of the final pass for one group of 4 columns (b, y, x .. x + 3): from dW'_k and dC through the fold,
// the normalisation and the neighbour-sited gather to dL/dguidance and dL/dblur_depth (see the file header)
// INTERIOR: every run (row y - 1 .. y + 1, columns x - 1 .. x + 4) lies inside the image -- no bounds checks, no border zero fill
template <bool INTERIOR>
__device__ __forceinline__ void bwd_epilogue4(const float* __restrict__ g, const float* __restrict__ blur, const float* __restrict__ sparse,
                                              const float* __restrict__ a0p, float* __restrict__ gg, float* __restrict__ gb, int b, int y,
                                              int x, size_t idx, size_t HW, int H, int W, int norm, const float (&dW)[8][4],
                                              const float (&dC)[4], bool acc = false) {
    // ---- epilogue: the chain through the fold, the normalisation and the neighbour-sited gather (see the file header)
    const float4 h0q = *reinterpret_cast<const float4*>(blur + idx);
    const float h0[4] = {h0q.x, h0q.y, h0q.z, h0q.w};
    float m[4] = {0.f, 0.f, 0.f, 0.f};
    if (sparse) {
        const float4 sq = *reinterpret_cast<const float4*>(sparse + idx);
        m[0] = signf(sq.x); m[1] = signf(sq.y); m[2] = signf(sq.z); m[3] = signf(sq.w);
    }
    const float4 a0q = *reinterpret_cast<const float4*>(a0p + idx);
    const float a0[4] = {a0q.x, a0q.y, a0q.z, a0q.w};
    const float* gbp = g + (size_t)b * 8 * HW;
    float* ggp = gg ? gg + (size_t)b * 8 * HW : nullptr;
    if (norm == CSPN_NORM_NONE) {  // gates used as given, centre-sited, no centre term: c' = m H_0
        if (gb) *reinterpret_cast<float4*>(gb + idx) = make_float4(a0[0] + dC[0] * m[0], a0[1] + dC[1] * m[1], a0[2] + dC[2] * m[2],
                                                                    a0[3] + dC[3] * m[3]);
        if (ggp) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                st4a_acc(ggp + k * HW + (size_t)y * W + x,
                         make_float4((1.f - m[0]) * dW[k][0], (1.f - m[1]) * dW[k][1], (1.f - m[2]) * dW[k][2], (1.f - m[3]) * dW[k][3]), acc);
        }
        return;
    }
    if (norm == CSPN_NORM_PRENORM) {  // gate_wb as given, at the pixel itself (see bwd_final_kernel): no normalisation chain, no scatter
        float sg[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(gbp + k * HW + (size_t)y * W + x);
            sg[0] += q.x; sg[1] += q.y; sg[2] += q.z; sg[3] += q.w;
        }
        float om[4], ch[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { om[i] = 1.f - m[i]; ch[i] = dC[i] * h0[i]; }
        if (gb) *reinterpret_cast<float4*>(gb + idx) = make_float4(a0[0] + dC[0] * (om[0] * (1.f - sg[0]) + m[0]), a0[1] + dC[1] * (om[1] * (1.f - sg[1]) + m[1]),
                                                                    a0[2] + dC[2] * (om[2] * (1.f - sg[2]) + m[2]), a0[3] + dC[3] * (om[3] * (1.f - sg[3]) + m[3]));
        if (ggp) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                st4a_acc(ggp + k * HW + (size_t)y * W + x,
                         make_float4(om[0] * (dW[k][0] - ch[0]), om[1] * (dW[k][1] - ch[1]), om[2] * (dW[k][2] - ch[2]), om[3] * (dW[k][3] - ch[3])), acc);
        }
        return;
    }
    // G_k(p) = g~_k(p + off_k): a run of four columns of plane k in row y + dy_k starting at x + dx_k, zero outside the image; the
    // eight runs stay in registers for the second half (the coefficient registers of the level loop are free by now)
    auto run = [&](int k, float (&v)[4]) -> bool {
        const int yy = y + dy2(k), xs = x + dx2(k);
        v[0] = v[1] = v[2] = v[3] = 0.f;
        if (!INTERIOR && (yy < 0 || yy >= H)) return false;
        const float* src = gbp + k * HW + (size_t)yy * W;
        if (INTERIOR || (xs >= 0 && xs + 3 < W)) {
            const float4 q = ld4u(src + xs);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (xs + i >= 0 && xs + i < W) v[i] = src[xs + i];
        }
        return true;
    };
    float om[4], ch[4], S[4] = {0.f, 0.f, 0.f, 0.f}, T1[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) { om[i] = 1.f - m[i]; ch[i] = dC[i] * h0[i]; }
    float vk[8][4];
    bool rowin[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        rowin[k] = run(k, vk[k]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float G = norm == CSPN_NORM_8SUM_ABS ? fabsf(vk[k][i]) : vk[k][i];
            S[i] += fabsf(vk[k][i]);
            gs[i] += G;
            T1[i] = fmaf(om[i] * (dW[k][i] - ch[i]), G, T1[i]);
        }
    }
    float rS[4], t2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { rS[i] = __builtin_amdgcn_rcpf(S[i]); t2[i] = T1[i] * rS[i] * rS[i]; }   // (v_rcp_f32: 1 ulp; three IEEE divisions per pixel were ~150 instructions per thread)
    if (gb) {
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = a0[i] + dC[i] * (om[i] * (1.f - gs[i] * rS[i]) + m[i]);
        *reinterpret_cast<float4*>(gb + idx) = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (ggp) {
        // g_k(q) with q - off_k outside the image is read by no pixel (the gather sees the zero padding instead): gradient 0
        // (only groups on the image's border have such elements)
        if (!INTERIOR && (y == 0 || y == H - 1 || x == 0 || x + 4 >= W)) {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int ys = y - dy2(k);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xq = x + i - dx2(k);
                    if (ys < 0 || ys >= H || xq < 0 || xq >= W) ggp[k * HW + (size_t)y * W + x + i] = 0.f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float (&v)[4] = vk[k];
            if (!rowin[k]) continue;  // the zero padding is a constant
            const int yy = y + dy2(k), xs = x + dx2(k);
            float d[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float G = norm == CSPN_NORM_8SUM_ABS ? fabsf(v[i]) : v[i];
                const float sg = G > 0.f ? 1.f : (G < 0.f ? -1.f : 0.f);
                float r = om[i] * (dW[k][i] - ch[i]) * rS[i] - sg * t2[i];
                if (norm == CSPN_NORM_8SUM_ABS) r *= v[i] > 0.f ? 1.f : (v[i] < 0.f ? -1.f : 0.f);
                d[i] = r;
            }
            float* dst = ggp + k * HW + (size_t)yy * W;   // g_k(p + off_k) is read by pixel p only
            if (INTERIOR || (xs >= 0 && xs + 3 < W)) st4u_acc(dst + xs, make_float4(d[0], d[1], d[2], d[3]), acc);
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (xs + i >= 0 && xs + i < W) dst[xs + i] = acc ? dst[xs + i] + d[i] : d[i];
            }
        }
    }
}

// ---- final pass from CHECKPOINTS: the sweeps keep every fourth level only -------------------------------------------------------
// The forward sweep stores H_4, H_8 .. H_20, the adjoint sweep A_20, A_16 .. A_4 (generator option hist_every; H_0 = blur and
// A_24 = dL/dout are inputs): 10 level planes through HBM instead of 46.  This pass recomputes the three levels in between,
// tile by tile: a block of 768 threads owns a REGION of 48 rows x 16 groups of 4 columns and produces the TILE that is left
// 4 pixels inside it (40 x 56); thread = one group (a wave = 4 region rows of 16 lanes, so the columns beside a group come
// from the neighbouring lane of the 16-lane DPP row, the rows above / below through LDS).  Per segment s = 0, 4 .. 20:
//   for t = s+3 .. s+1:  A_t(q) = sum_k (w'_k A_{t+1})(q - off_k)              (the adjoint levels first, each parked in LDS)
//   H_{s+1..s+3} = c' + sum_k w'_k shift_k(H)            (pull form; valid one pixel further inside the region per step)
//   for l = 0 .. 3:      dW'_k += A_{s+l+1} H_{s+l}(. + off_k), dC += A_{s+l+1}
// the adjoint step in PUSH form, so that both recurrences use the thread's own, centre-sited w'_k(p) -- loaded once per tile, no
// coefficient traffic per step: p sends P_k = w'_k(p) A_{t+1}(p) to q = p + off_k; what goes to the row below / above is summed
// over its three columns first (one quad each through LDS), the in-row part stays in the lanes.  c' is not stored:
// c' = H_0 (1 - sum_k w'_k) for the normalising modes (any sparse sign), m H_0 for norm NONE.  Outside the image everything is
// exactly 0, as in the forward's zero padding.  The grid is 1-D; the hardware deals block i to XCD i % 8, and every XCD gets a
// contiguous run of tiles (numbered along x, then y, then the batch), so that the tiles whose regions overlap run on the same XCD at
// about the same time and share its L2.
//
// MIXED pixel pairs (the trick of the forward ring).  With a group's four pixels in image order (c0, c1, c2, c3) the
// pairs the x +- 1 taps multiply with -- (c-1, c0), (c1, c2), (c3, c+1) -- straddle the aligned register pairs and have to be copied
// together for every row of every step (a third of the instructions of the first version of this pass were such v_mov).  Here a
// group lives in REGISTER order (c0, c3, c1, c2) -- the order the sweeps store their checkpoints in anyway --, X = (c0, c3),
// Y = (c1, c2), D = (c3 of the lane before, c0 of the lane after: two DPP moves), and every packed FMA combines the dx = +1 tap of
// its low pixel with the dx = -1 tap of its high pixel:
//   X += (w_+(c0), w_-(c3)) * Y      X += (w_-(c0), w_+(c3)) * D      X += (w_0(c0), w_0(c3)) * X
//   Y += (w_-(c1), w_+(c2)) * X      Y += (w_0(c1), w_0(c2)) * Y      Ysw += (w_-(c2), w_+(c1)) * Y   (Y += swap(Ysw) once per step)
// per row of taps (w_+, w_0, w_- = the row's dx = +1, 0, -1 coefficients), with the coefficient pairs mixed ONCE per tile.  The same
// pairs serve the adjoint step in push form (products with A instead of H; what leaves for the next lane goes through the same two
// DPP moves) and the gradient accumulators dW', which stay mixed until the epilogue.  No operand is ever copied: an H step with its 16
// products is 32 v_pk_fma_f32 + 6 DPP + 3 swaps, an adjoint step 16 packed multiplies / FMAs + 6 DPP + 1 swap (the pass is bound by
// VALU issue, not by memory).
constexpr int CK = 4, CK_GR = 16, CK_TG = CK_GR - 2, NCKP = 24 / CK - 1;   // NCKP: level planes a sweep keeps

typedef float v2f __attribute__((ext_vector_type(2)));

// workgroup barrier for LDS traffic only: __syncthreads() also waits for every global load in flight (vmcnt 0), i.e. for the next
// segment's checkpoints that are meant to arrive under this segment's arithmetic
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }


__device__ __forceinline__ float4 img_to_reg(float4 q) { return make_float4(q.x, q.w, q.y, q.z); }   // (c0..c3) -> (c0,c3,c1,c2)
__device__ __forceinline__ v2f swp2(v2f v) { return __builtin_shufflevector(v, v, 1, 0); }

template <int CK_ROWS, bool MULTI>
__global__ __launch_bounds__(CK_ROWS * CK_GR) __attribute__((amdgpu_waves_per_eu(CK_ROWS / 16, CK_ROWS / 16))) void bwd_final_mx_kernel(
    const float* __restrict__ g, const float* __restrict__ blur, const float* __restrict__ sparse, const float* __restrict__ hh,
    const float* __restrict__ ah, const float* __restrict__ wf, const float* __restrict__ a0p, const float* __restrict__ gout,
    float* __restrict__ gg, float* __restrict__ gb, int B, int H, int W, int norm, int nseg, int C, int c) {
    // C > 1: B guidance images of C channels each (cspn2d_backward_multi_f32); this launch takes channel c of every image: the
    // level / coefficient planes and the 1-channel tensors are [B*C][H][W] (image-channel b * C + c), gg [B][8][H][W] gets the channel's part
    // added to what the launches of channels 0 .. c - 1 left there
    constexpr int CK_NT = CK_ROWS * CK_GR, CK_TR = CK_ROWS - 2 * CK;
    const int NSEG = nseg;   // n_iter / 4 segments of four levels (round 5: n_iter = 4, 8 .. 24; 6 for the reference's 24)
    __shared__ __attribute__((aligned(16))) float4 sH[2][CK_NT];       // H_{s+l} of the region, two planes alternating (REGISTER order inside a quad)
    __shared__ __attribute__((aligned(16))) float4 sA[CK][CK_NT];      // A_{s+1} .. A_{s+4}: every thread's own group only
    __shared__ __attribute__((aligned(16))) float4 sT[2][2][CK_NT];    // [parity][to the row below | above]
    const int tid = threadIdx.x, gx = tid & (CK_GR - 1), ry = tid >> 4;
    const int W4 = W >> 2;
    const int nbx = (W4 + CK_TG - 1) / CK_TG, nby = (H + CK_TR - 1) / CK_TR, ntile = nbx * nby * B, per = (ntile + 7) / 8;
    const int tile = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);   // XCD-aware tile order (above)
    if (tile >= ntile || (int)(blockIdx.x >> 3) >= per) return;   // (whole block: no barrier is left waiting)
    const int bx = tile % nbx, by = (tile / nbx) % nby, b = tile / (nbx * nby);
    const int y = by * CK_TR - CK + ry, xg = bx * CK_TG - 1 + gx;
    const bool inimg = y >= 0 && y < H && xg >= 0 && xg < W4;
    const bool intile = inimg && ry >= CK && ry < CK_ROWS - CK && gx >= 1 && gx < CK_GR - 1;
    const int x = 4 * (inimg ? xg : 0);
    // (MULTI false: the single-channel kernel exactly -- C = 1, c = 0 as constants, no accumulation)
    const int Cm = MULTI ? C : 1, cm = MULTI ? c : 0;
    const size_t HW = (size_t)H * W, total = (size_t)B * Cm * HW;
    const size_t idx = ((size_t)b * Cm + cm) * HW + (size_t)(inimg ? y : 0) * W + x;
    const bool acc = MULTI && c > 0;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    // (idx is a valid group of its row even for threads outside the image -- clamped above --: load unconditionally, select the value.
    // A conditional load through this lambda had been compiled to four FLAT dword loads, which also tie up lgkmcnt, the counter
    // every LDS barrier below waits on)
    auto ld = [&](const float* p) {
        typedef float v4g __attribute__((ext_vector_type(4)));
        const v4g v = *(const __attribute__((address_space(1))) v4g*)(p + idx);   // one global_load_dwordx4
        return inimg ? make_float4(v.x, v.y, v.z, v.w) : z4;
    };
    // coefficient pairs, mixed once per tile.  Row of taps d = 0 (dy = +1: k = 0, 1, 2), 1 (dy = 0: k = 3, 4), 2 (dy = -1: k = 5, 6, 7);
    // in a row: w_+ = the dx = +1 tap, w_0 = dx = 0, w_- = dx = -1
    v2f mAX[3], mBX[3], mAYs[3], mBY[3], n0X[3], n0Y[3], cpX, cpY;
    {
        const float4 h0 = ld(blur);
        float4 wq[8];
        float sw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            wq[k] = ld(wf + (size_t)k * total);
            sw[0] += wq[k].x; sw[1] += wq[k].y; sw[2] += wq[k].z; sw[3] += wq[k].w;
        }
        constexpr int KP[3] = {0, 3, 5}, K0[3] = {1, 1, 6}, KM[3] = {2, 4, 7};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            mAX[d] = v2f{wq[KP[d]].x, wq[KM[d]].w};    // (w_+(c0), w_-(c3))
            mBX[d] = v2f{wq[KM[d]].x, wq[KP[d]].w};    // (w_-(c0), w_+(c3))
            mAYs[d] = v2f{wq[KM[d]].z, wq[KP[d]].y};   // (w_-(c2), w_+(c1))
            mBY[d] = v2f{wq[KM[d]].y, wq[KP[d]].z};    // (w_-(c1), w_+(c2))
            n0X[d] = d == 1 ? v2f{0.f, 0.f} : v2f{wq[K0[d]].x, wq[K0[d]].w};
            n0Y[d] = d == 1 ? v2f{0.f, 0.f} : v2f{wq[K0[d]].y, wq[K0[d]].z};
        }
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        if (sparse) { const float4 sq = ld(sparse); m[0] = signf(sq.x); m[1] = signf(sq.y); m[2] = signf(sq.z); m[3] = signf(sq.w); }
        const float h0a[4] = {h0.x, h0.y, h0.z, h0.w};
        float c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = inimg ? (norm == CSPN_NORM_NONE ? m[i] * h0a[i] : h0a[i] * (1.f - sw[i])) : 0.f;
        cpX = v2f{c[0], c[3]}; cpY = v2f{c[1], c[2]};
    }
    const v2f zero2 = {0.f, 0.f};
    v2f dAX[3], dBX[3], dAYs[3], dBY[3], dN0X[3], dN0Y[3], dCX = zero2, dCY = zero2;   // the gradient accumulators, mixed like the coefficients
#pragma unroll
    for (int d = 0; d < 3; ++d) dAX[d] = dBX[d] = dAYs[d] = dBY[d] = dN0X[d] = dN0Y[d] = zero2;
    // the LDS slots of the group below / above (indices, not pointers: a pointer to a level plane that passes through a lambda or a select
    // becomes a generic pointer and its reads flat loads; at the region's first / last row the thread reads its own row again: halo)
    const int tdn_i = ry < CK_ROWS - 1 ? tid + CK_GR : tid, tup_i = ry > 0 ? tid - CK_GR : tid;
    auto seg_h = [&](int j) { return ld(j == 0 ? blur : hh + (size_t)(j - 1) * total); };                       // H_{4j}
    auto seg_a = [&](int j) { return ld(j == NSEG - 1 ? gout : ah + (size_t)(NSEG - 2 - j) * total); };         // A_{4j+4}
    const bool wave_in_tile_rows = (ry & ~3) >= CK && (ry & ~3) < CK_ROWS - CK;   // a wave = 4 region rows: the first / last wave only feeds
    // the adjoint levels of a segment first, then its H steps (7 barriers per segment, one dependent chain at a time); the whole segment loop
    // twice: blocks whose region lies inside the image (two thirds of them at KITTI size) need no "outside the image -> 0" selects
    float4 nh = seg_h(0), na = seg_a(0);   // the checkpoints are requested one segment ahead
    int par = 0;
    auto segments = [&](auto masked) {
        constexpr bool MASKED = decltype(masked)::value;
#pragma unroll 1
        for (int j = 0; j < NSEG; ++j) {
            // (the sweeps' planes are in register order already; blur / dL/dout are in image order)
            float4 hq = j == 0 ? img_to_reg(nh) : nh;
            const float4 aq4 = j == NSEG - 1 ? img_to_reg(na) : na;
            if (j + 1 < NSEG) { nh = seg_h(j + 1); na = seg_a(j + 1); }
            // ---- the adjoint levels first: A_{s+4} -> A_{s+3}, A_{s+2}, A_{s+1} (push form), each parked in the thread's own LDS slot
            v2f aX = v2f{aq4.x, aq4.y}, aY = v2f{aq4.z, aq4.w};
            sA[CK - 1][tid] = aq4;
#pragma unroll 1
            for (int l = CK - 1; l >= 1; --l) {
                const v2f aYs = swp2(aY);
                v2f tX[3], tY[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const v2f M = mBX[d] * aX;                                   // (P_-(c0), P_+(c3)): what leaves for the neighbouring lanes
                    tX[d] = v2f{dpp_shr1(M[1]), dpp_shl1(M[0])};                 // (P_+(c3 of the lane before), P_-(c0 of the lane after))
                    tX[d] = __builtin_elementwise_fma(mBY[d], aY, tX[d]);        // + (P_-(c1), P_+(c2))
                    tY[d] = mAX[d] * aX;                                         // (P_+(c0), P_-(c3))
                    tY[d] = __builtin_elementwise_fma(mAYs[d], aYs, tY[d]);      // + (P_-(c2), P_+(c1))
                    if (d != 1) {
                        tX[d] = __builtin_elementwise_fma(n0X[d], aX, tX[d]);
                        tY[d] = __builtin_elementwise_fma(n0Y[d], aY, tY[d]);
                    }
                }
                sT[par][0][tid] = make_float4(tX[0][0], tX[0][1], tY[0][0], tY[0][1]);   // dy = +1: to the row below
                sT[par][1][tid] = make_float4(tX[2][0], tX[2][1], tY[2][0], tY[2][1]);   // dy = -1: to the row above
                lds_barrier();
                const float4 fa = sT[par][0][tup_i];     // from the row above, sent down
                const float4 fb = sT[par][1][tdn_i];     // from the row below, sent up
                par ^= 1;
                aX = tX[1] + v2f{fa.x, fa.y} + v2f{fb.x, fb.y};
                aY = tY[1] + v2f{fa.z, fa.w} + v2f{fb.z, fb.w};
                if (MASKED && !inimg) { aX = zero2; aY = zero2; }
                sA[l - 1][tid] = make_float4(aX[0], aX[1], aY[0], aY[1]);
            }
            // ---- then H_s -> H_{s+3}; the row pairs of a step are also what A_{t+1} multiplies with for dW'
            sH[0][tid] = hq;
            lds_barrier();
#pragma unroll 1
            for (int l = 0; l < CK; ++l) {
                const float4 q[3] = {sH[l & 1][tdn_i], hq, sH[l & 1][tup_i]};   // rows y + 1, y, y - 1 (at the region's first / last row: the own row again, halo)
                v2f Xr[3], Yr[3], Dr[3];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    Xr[d] = v2f{q[d].x, q[d].y};
                    Yr[d] = v2f{q[d].z, q[d].w};
                    Dr[d] = v2f{dpp_shr1(q[d].y), dpp_shl1(q[d].x)};   // (c3 of the lane before, c0 of the lane after; 0 at the region's edge: halo)
                }
                if (wave_in_tile_rows) {
                    const float4 aq = sA[l][tid];   // A_{s+l+1}
                    const v2f bX = v2f{aq.x, aq.y}, bY = v2f{aq.z, aq.w}, bYs = swp2(bY);
                    dCX += bX;
                    dCY += bY;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        dAX[d] = __builtin_elementwise_fma(bX, Yr[d], dAX[d]);
                        dBX[d] = __builtin_elementwise_fma(bX, Dr[d], dBX[d]);
                        dBY[d] = __builtin_elementwise_fma(bY, Xr[d], dBY[d]);
                        dAYs[d] = __builtin_elementwise_fma(bYs, Yr[d], dAYs[d]);
                        if (d != 1) {
                            dN0X[d] = __builtin_elementwise_fma(bX, Xr[d], dN0X[d]);
                            dN0Y[d] = __builtin_elementwise_fma(bY, Yr[d], dN0Y[d]);
                        }
                    }
                }
                if (l == CK - 1) break;
                v2f nX = cpX, nY = cpY, nYs = mAYs[0] * Yr[0];
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    nX = __builtin_elementwise_fma(mAX[d], Yr[d], nX);
                    nX = __builtin_elementwise_fma(mBX[d], Dr[d], nX);
                    nY = __builtin_elementwise_fma(mBY[d], Xr[d], nY);
                    if (d != 0) nYs = __builtin_elementwise_fma(mAYs[d], Yr[d], nYs);
                    if (d != 1) {
                        nX = __builtin_elementwise_fma(n0X[d], Xr[d], nX);
                        nY = __builtin_elementwise_fma(n0Y[d], Yr[d], nY);
                    }
                }
                nY += swp2(nYs);
                if (MASKED && !inimg) { nX = zero2; nY = zero2; }
                hq = make_float4(nX[0], nX[1], nY[0], nY[1]);
                sH[(l + 1) & 1][tid] = hq;   // (the plane read two steps ago: everybody is past the barrier in between)
                lds_barrier();
            }
        }
    };
    const int ry0 = by * CK_TR - CK, xg0 = bx * CK_TG - 1;
    const bool blk_in = ry0 >= 0 && ry0 + CK_ROWS <= H && xg0 >= 0 && xg0 + CK_GR <= W4;
    if (blk_in) segments(std::false_type{});
    else segments(std::true_type{});
    if (!intile) return;
    // un-mix: dW'_k per pixel in image order, as the epilogue wants it
    float dWs[8][4], dCs[4] = {dCX[0], dCY[0], dCY[1], dCX[1]};
    constexpr int KP[3] = {0, 3, 5}, K0[3] = {1, 1, 6}, KM[3] = {2, 4, 7};
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        dWs[KP[d]][0] = dAX[d][0];  dWs[KM[d]][3] = dAX[d][1];
        dWs[KM[d]][0] = dBX[d][0];  dWs[KP[d]][3] = dBX[d][1];
        dWs[KM[d]][2] = dAYs[d][0]; dWs[KP[d]][1] = dAYs[d][1];
        dWs[KM[d]][1] = dBY[d][0];  dWs[KP[d]][2] = dBY[d][1];
        if (d != 1) {
            dWs[K0[d]][0] = dN0X[d][0]; dWs[K0[d]][3] = dN0X[d][1];
            dWs[K0[d]][1] = dN0Y[d][0]; dWs[K0[d]][2] = dN0Y[d][1];
        }
    }
    if (blk_in) bwd_epilogue4<true>(g, blur, sparse, a0p, gg, gb, b, y, x, idx, HW, H, W, norm, dWs, dCs, acc);
    else bwd_epilogue4<false>(g, blur, sparse, a0p, gg, gb, b, y, x, idx, HW, H, W, norm, dWs, dCs, acc);
}

}  // namespace

constexpr size_t FRONT_PAD = 65536;  // bytes kept addressable in front of the folded planes (the adjoint sweep reads plane 0
                                     // one row up and one pixel left of its first row)
// n_iter = 4, 8 .. 24 (round 5; rounds 3-4: 24 only).  The sweeps always run the ring's 24 levels; for n_iter < 24 the levels beyond n_iter are
// computed and ignored: the forward's result H_n is its checkpoint plane n/4 - 1, the adjoint sweep started from A_n = dL/dout leaves A_{n-4-4i} in its
// plane i and A_0 in plane n/4 - 1 (both in register order: reg_to_img_plane below), and the final pass runs n/4 segments.
static bool asm_path(int B, int H, int W, int n_iter) {
    return n_iter >= 4 && n_iter <= 24 && (n_iter % 4) == 0 && tsw2d_supported(B, H, W) && 4ull * W + 16 <= FRONT_PAD &&
           (unsigned long long)B * H * W * 32ull < (1ull << 32);  // 8 coefficient planes of per-lane byte offsets
}

// checkpointed: [FRONT_PAD][H_4 .. H_20][w'_0 .. w'_7][A_20 .. A_4][A_0][a scratch output] + 256 -- what the forward sweep leaves behind
// first, so that its first two parts are the history a training forward keeps
Backward2dLayout Backward2dLayout::checkpointed(int B, int H, int W) {
    const size_t plane = sizeof(float) * (size_t)B * H * W;
    Backward2dLayout L;
    L.ckpt = true;
    L.hh = FRONT_PAD;
    L.wf = L.hh + NCKP * plane;
    L.wt = 0;
    L.ah = L.history = L.wf + 8 * plane;
    L.a0 = L.ah + NCKP * plane;
    L.scratch = L.a0 + plane;
    L.adjoint = L.scratch - L.ah + 256;
    L.bytes = L.scratch + plane + 256;
    return L;
}

// stepwise: [w' x 9][wt x 8][H_1 .. H_{N-1}][A_0 .. A_{N-1}]
Backward2dLayout::Backward2dLayout(int B, int H, int W, int n_iter) {
    if (asm_path(B, H, W, n_iter)) { *this = checkpointed(B, H, W); return; }
    const size_t plane = sizeof(float) * (size_t)B * H * W;
    ckpt = false;
    wf = 0;
    wt = 9 * plane;
    hh = wt + 8 * plane;
    ah = hh + (size_t)(n_iter > 0 ? n_iter - 1 : 0) * plane;
    bytes = ah + (size_t)n_iter * plane;
    a0 = scratch = history = adjoint = 0;
}

size_t backward2d_workspace(int B, int H, int W, int n_iter) { return Backward2dLayout(B, H, W, n_iter).bytes; }

// a level plane in the sweeps' register order (c0,c3,c1,c2 per aligned 4-column group) -> image order
__global__ __launch_bounds__(256) void reg_to_img_plane_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t n4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) { const float4 q = src[i]; dst[i] = make_float4(q.x, q.z, q.w, q.y); }
}
static void reg_to_img_plane(const float* src, float* dst, size_t total, hipStream_t st) {
    hipLaunchKernelGGL(reg_to_img_plane_kernel, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, (const float4*)src, (float4*)dst, total / 4);
}

// final pass of the assembly-sweep backward: from the checkpoints of both sweeps.  C > 1: B guidance images, the sweeps ran over B * C
// image-channels; one launch per channel, in channel order, each adding its part of dL/dguidance to what the one before left
static void launch_final_mx(const float* g, const float* blur, const float* sparse, const float* hh, const float* ah, const float* wf,
                            const float* a0, const float* gout, float* gg, float* gb, int B, int H, int W, int norm, int nseg, hipStream_t st,
                            int C = 1) {
    constexpr int ROWS = 48, TROWS = ROWS - 2 * CK;   // region rows; 24, 32 and 64 measured slower (profiles/r03_backward_checkpoints.md, r05_backward_final_mx_ab.md)
    const int ntile = ((W / 4 + CK_TG - 1) / CK_TG) * ((H + TROWS - 1) / TROWS) * B, per = (ntile + 7) / 8;
    for (int c = 0; c < C; ++c)
        hipLaunchKernelGGL((C > 1 ? bwd_final_mx_kernel<ROWS, true> : bwd_final_mx_kernel<ROWS, false>), dim3((unsigned)(per * 8)), dim3(ROWS * CK_GR), 0,
                           st, g, blur, sparse, hh, ah, wf, a0, gout, gg, gb, B, H, W, norm, nseg, C, c);
}

// the end of both checkpointed backwards: the adjoint sweep over the folded planes wf (a propagation whose coefficients are those planes read
// neighbour-sited with the channel order reversed, generator option adj), keeping every fourth of its levels in ah; A_0 into image order; the
// final pass, which recomputes the levels in between
static int adjoint_and_final(const float* g, const float* blur, const float* sparse, const float* gout, const float* hh, const float* wf, float* ah,
                             float* a0, float* gg, float* gb, int B, int H, int W, int n_iter, int norm, hipStream_t st, int C) {
    const size_t total = (size_t)B * H * W;
    const int nseg = n_iter / CK;
    if (int e = tsw2d_adjoint_pass(wf, gout, a0, B, H, W, st, ah)) return e;
    if (nseg <= NCKP) reg_to_img_plane(ah + (size_t)(nseg - 1) * total, a0, total, st);   // A_0 of a sweep shorter than the ring
    launch_final_mx(g, blur, sparse, hh, ah, wf, a0, gout, gg, gb, B / C, H, W, norm, nseg, st, C);
    return check_launch("bwd_final_mx_kernel");
}

bool backward2d_multi_supported(int BC, int H, int W, int n_iter) { return asm_path(BC, H, W, n_iter); }

int backward2d(const float* g, const float* blur, const float* sparse, const float* gout, float* gg, float* gb, int B, int H,
               int W, int n_iter, int norm, void* ws, hipStream_t st, int C) {
    const size_t total = (size_t)B * H * W;
    const Backward2dLayout L(B, H, W, n_iter);
    auto at = [&](size_t off) { return (float*)((char*)ws + off); };
    if (C > 1 && !L.ckpt) { set_error("channels on shared guidance: the assembly sweeps only"); return CSPN_E_UNSUPPORTED; }
    if (L.ckpt) {
        // both sweeps run in the fused ring kernel (cspn2d_tsw.hip), each keeping every fourth of its levels: the forward
        // as it is (it also leaves the 8 folded coefficient planes right behind its level planes), then the adjoint
        if (int e = tsw2d_pass(g, blur, blur, sparse, at(L.scratch), B, H, W, norm, st, at(L.hh), 0, 0, C)) return e;
        return adjoint_and_final(g, blur, sparse, gout, at(L.hh), at(L.wf), at(L.ah), at(L.a0), gg, gb, B, H, W, n_iter, norm, st, C);
    }
    float *wf = at(L.wf), *wt = at(L.wt);   // folded coefficients; transposed ones of the adjoint stencil
    float *hh = at(L.hh), *ah = at(L.ah);   // H_1 .. H_{N-1}; A_0 .. A_{N-1}
    const unsigned blocks = (unsigned)((total + 255) / 256);
    hipLaunchKernelGGL(fold2d_kernel, dim3(blocks), dim3(256), 0, st, g, blur, sparse, wf, B, H, W, norm);
    if (int e = check_launch("fold2d_kernel")) return e;
    for (int t = 1; t < n_iter; ++t)
        hipLaunchKernelGGL(step2d_kernel, dim3(blocks), dim3(256), 0, st, wf, t == 1 ? blur : hh + (size_t)(t - 2) * total,
                           hh + (size_t)(t - 1) * total, B, H, W);
    hipLaunchKernelGGL(transpose_w_kernel, dim3(blocks), dim3(256), 0, st, wf, wt, B, H, W);
    for (int t = n_iter - 1; t >= 0; --t)
        hipLaunchKernelGGL(bwd_step_kernel, dim3(blocks), dim3(256), 0, st, wt,
                           t == n_iter - 1 ? gout : ah + (size_t)(t + 1) * total, ah + (size_t)t * total, B, H, W);
    if (int e = check_launch("bwd_step_kernel")) return e;
    hipLaunchKernelGGL(bwd_final_kernel, dim3(blocks), dim3(256), 0, st, g, blur, sparse, hh, ah, gout, gg, gb, B,
                       H, W, n_iter, norm);
    return check_launch("bwd_final_kernel");
}

// ---- training mode: the forward keeps its checkpoints (the checkpointed layout's first two parts), the backward starts from them ----
size_t history2d_bytes(int B, int H, int W, int n_iter) { return asm_path(B, H, W, n_iter) ? Backward2dLayout::checkpointed(B, H, W).history : 0; }

int forward2d_history(const float* g, const float* blur, const float* sparse, float* out, void* history, int B, int H, int W,
                      int n_iter, int norm, void* ws, hipStream_t st, int C) {
    float* hh = (float*)((char*)history + Backward2dLayout::checkpointed(B, H, W).hh);
    (void)ws;
    if (int e = tsw2d_pass(g, blur, blur, sparse, out, B, H, W, norm, st, hh, 0, 0, C)) return e;   // (n_iter < 24: `out` = level 24 for a moment)
    const int nseg = n_iter / CK;
    if (nseg <= NCKP) {   // the result is the checkpoint H_n
        reg_to_img_plane(hh + (size_t)(nseg - 1) * B * H * W, out, (size_t)B * H * W, st);
        return check_launch("reg_to_img_plane_kernel");
    }
    return 0;
}

// the workspace holds the layout's parts behind the history, from `ah`, without the scratch output
size_t backward2d_history_workspace(int B, int H, int W) { return Backward2dLayout::checkpointed(B, H, W).adjoint; }

int backward2d_history(const float* g, const float* blur, const float* sparse, const float* gout, const void* history, float* gg,
                       float* gb, int B, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, int C) {
    const Backward2dLayout L = Backward2dLayout::checkpointed(B, H, W);
    const char* hist = (const char*)history;
    char* adj = (char*)ws;   // starts at the layout's `ah`
    return adjoint_and_final(g, blur, sparse, gout, (const float*)(hist + L.hh), (const float*)(hist + L.wf), (float*)adj, (float*)(adj + (L.a0 - L.ah)),
                             gg, gb, B, H, W, n_iter, norm, st, C);
}

}  // namespace cspn
