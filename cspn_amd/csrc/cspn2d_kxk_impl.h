// cspn2d_kxk_impl.h -- the 2D K x K engine's kernels and host paths, included by the translation units that instantiate them:
// cspn2d_kxk.hip (neighbour distance one, every contract), cspn2d_kxk_dil.hip (the dilated folded / assembling contracts) and
// cspn2d_kxk_pin.hip (the folded / assembling contracts pinned to the measured depth with a per-pixel confidence: kxk_fold_pin,
// kxk_unfold_pixel_pin and the host paths' PIN argument, at every dilation).
// The 2D NONE op (Paddle contract: gates used as given, centre-sited, no centre term, any sign) over a K x K
// neighbourhood, K = 2R+1 in {5, 7}, forward and backward.  gate [N][KK][H][W], KK = K*K - 1; values [N][C][H][W], the C channels
// share the gates (reference cspn_paddle/README.md:54-56).
//   channel order  gate channel k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre (R, R); its neighbour
//                  offset is (dy, dx) = (R - t, R - l) (K = 3 gives the DY / DX of the 3 x 3 op)
//   forward        H_{t+1}(p) = sum_k g_k(p) H_t(p + off_k), zero outside the image, summed in channel order
//   adjoint        A_t(q) = sum_k g_k(q - off_k) A_{t+1}(q - off_k)   (A_n = dL/dout, dL/dx = A_0)
//   gate gradient  dL/dg_k(p) = sum_{t<n} sum_c A_{t+1}(p) H_t(p + off_k), accumulated in registers over t, then c; written once
// Every kernel runs one 64 x 16 pixel tile per workgroup of 256 threads, four adjacent pixels of a row per thread; the values of the
// tile plus an R-wide halo (zeros outside the image) are staged in LDS once per channel.  The forward and the adjoint step hold the
// KK x 4 gates a thread needs in registers and loop over the C channels, so the gates are read once per step for all channels.
// Bytes per pixel: forward step 4 KK + 8 C; adjoint step the same; gate gradient 8 n C + 4 KK.
// Below them, the depth-completion contract of Affinity_Propagate over K x K (K = 3, 5 or 7): folded into w' and a bias b by kxk_fold,
// run by the same step with BIAS, and differentiated by the same adjoint step, the gate gradient with BIAS, kxk_unfold_pixel and
// kxk_unsite.
// Last, the demo module's contract (ABS): the guide is raw, a_k = |g_k| enters the multiply-add and the sum is scaled by 1 / S,
// S(p) = sum_k a_k(p) in channel order, after it.  The gates are centre-sited, so the thread that steps a pixel holds all of its gates
// and forms S from them; the adjoint step holds the gates of shifted pixels and reads 1 / S from a plane (kxk_rsum) while it stages
// A; the gate gradient's epilogue re-reads the guide a channel at a time: no normalised gate and no dL/dw is ever stored.
// The assembling contract (CSPN++: a per-pixel weighted sum of collected levels, out = sum_j conf_j H_{s_j}) is the folded contract with an
// epilogue: the collecting forward step also updates out from the level it has in registers, the injecting adjoint step adds
// conf_j grad_out to the adjoint level it stores, and kxk_conf_grad reduces grad_out H_{s_j} over the channels.
// Gate storage type GT: float, or __half / __hip_bfloat16 (the *_g16 entry points).  A 16-bit gate is widened to float32 exactly where
// it is used, every multiply-add and sum is the float32 one in the same order, so the results are bitwise those of the float instance
// on the widened gates; a gradient with respect to a 16-bit tensor is accumulated in float32 and rounded once (to nearest even,
// subnormals kept) at its single store.  Values, levels, w', b, the mask and grad_x are float32 throughout.
// Dilation D (a trailing template argument, default 1): the neighbour offset of the folded and the assembling contract becomes
// D (R - t, R - l).  The halo is R D wide, a thread's row window 4 + 2 R D floats, its tap j + (2R - l) D (forward, gate gradient) or
// j + l D (adjoint); siting and un-siting read at the dilated offset.  Every index is written as the D = 1 expression with its constants
// and its loop variable each times D (y + R D - t D, not y + (R - t) D), so that a D = 1 instance compiles to the code it was before D existed.  The dilated steps exist for the float32 w' only (a 16-bit guidance costs the fold-side kernels).
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <type_traits>

#include "cspn_common.h"
#include "cspn_gate16.h"

namespace cspn {

namespace {

constexpr int NT = 256;
constexpr int QX = 16;          // threads per tile row (four pixels each)
constexpr int TW = 4 * QX;      // tile width in pixels
constexpr int TH = NT / QX;     // tile height in rows

struct Tile {
    int n, y, x0, ly, lq, y0, xt0;
};

__device__ __forceinline__ Tile tile_of(int tiles_x, int tiles_y) {
    int b = blockIdx.x;
    Tile t;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    t.n = b / tiles_y;
    t.ly = threadIdx.x / QX;
    t.lq = threadIdx.x % QX;
    t.y0 = ty * TH;
    t.xt0 = tx * TW;
    t.y = t.y0 + t.ly;
    t.x0 = t.xt0 + 4 * t.lq;
    return t;
}

// the plane s [H][W] of the tile's rows y0 - R .. y0 + TH + R - 1 and columns xt0 - R .. xt0 + TW + R - 1 into lds, zeros outside the image;
// R: the halo, the stencil's radius times its dilation
template <int R>
__device__ __forceinline__ void stage(float* lds, const float* __restrict__ s, int y0, int xt0, int H, int W) {
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    for (int i = threadIdx.x; i < SW * SH; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - R + r, gx = xt0 - R + c;
        lds[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? s[gy * W + gx] : 0.f;
    }
}

// the four gates of pixels x0 .. x0+3 as a thread holds them: float as four registers, 16-bit packed two to a register and widened at
// the multiply-add (fp16 by the mixed-precision FMA's operand select, bf16 by a shift or a mask)
template <class GT>
struct Quad {
    uint32_t p[2];
    __device__ __forceinline__ void clear() { p[0] = p[1] = 0u; }
    // keeps the packed form live across the channel loop: without it the compiler hoists the widening out of the loop and holds four
    // registers per quad, as the float instance does
    __device__ __forceinline__ void pin() { asm volatile("" : "+v"(p[0]), "+v"(p[1])); }
    __device__ __forceinline__ void pin_sign() {}
    __device__ __forceinline__ void put(int j, unsigned short v) { p[j >> 1] |= (uint32_t)v << (16 * (j & 1)); }
    __device__ __forceinline__ float get(int j) const {
        if constexpr (std::is_same<GT, __half>::value) return widen<GT>((unsigned short)(p[j >> 1] >> (16 * (j & 1))));
        else return __uint_as_float((j & 1) ? (p[j >> 1] & 0xffff0000u) : (p[j >> 1] << 16));
    }
    // |gate|: the odd bf16 element drops its sign in the mask that widens it, the rest as a source modifier of the multiply-add
    __device__ __forceinline__ float mag(int j) const {
        if constexpr (std::is_same<GT, __half>::value) return fabsf(get(j));
        else return (j & 1) ? __uint_as_float(p[j >> 1] & 0x7fff0000u) : fabsf(__uint_as_float(p[j >> 1] << 16));
    }
};
template <>
struct Quad<float> {
    float v[4];
    __device__ __forceinline__ void clear() { v[0] = v[1] = v[2] = v[3] = 0.f; }
    __device__ __forceinline__ void pin() {}
    // ABS: keeps |gate| from being computed once in front of the channel loop, so that it folds into the multiply-add as a source modifier
    __device__ __forceinline__ void pin_sign() { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
    __device__ __forceinline__ void put(int j, float x) { v[j] = x; }
    __device__ __forceinline__ float get(int j) const { return v[j]; }
    __device__ __forceinline__ float mag(int j) const { return fabsf(v[j]); }
};

// stage for the adjoint of the ABS contract: A / S as A * (1 / S).  rs: the plane [H][W] of 1 / S that kxk_rsum wrote, or NULL (a single
// step, which has no workspace): 1 / S is then formed here from the pixel's KK gates gb [KK][H][W], the same sum and division
template <int R, int KK, class GT>
__device__ __forceinline__ void stage_scaled(float* lds, const float* __restrict__ s, const float* __restrict__ rs, const store_t<GT>* __restrict__ gb,
                                             int y0, int xt0, int H, int W) {
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    if (rs) {
        for (int i = threadIdx.x; i < SW * SH; i += NT) {
            const int r = i / SW, c = i - r * SW;
            const int gy = y0 - R + r, gx = xt0 - R + c;
            lds[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? s[gy * W + gx] * rs[gy * W + gx] : 0.f;
        }
        return;
    }
    for (int i = threadIdx.x; i < SW * SH; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - R + r, gx = xt0 - R + c;
        float v = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            float S = 0.f;
            for (int k = 0; k < KK; ++k) S += fabsf(widen<GT>(gb[(size_t)k * H * W + gy * W + gx]));
            v = s[gy * W + gx] * (1.f / S);
        }
        lds[i] = v;
    }
}

// four pixels x0 .. x0+3 of row y (p = row offset of x0), widened; VEC: W % 4 == 0 and the plane aligned to four elements (16 bytes
// for float, 8 for a 16-bit type; a quad is then all in or all out)
template <bool VEC, class T = float>
__device__ __forceinline__ void load4(float (&v)[4], const store_t<T>* __restrict__ p, bool row_in, int x0, int W) {
    if constexpr (std::is_same<T, float>::value) {
        if (VEC) {
            const float4 q = (row_in && x0 < W) ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (row_in && x0 + j < W) ? p[j] : 0.f;
        }
    } else {
        if (VEC) {
            const uint2 q = (row_in && x0 < W) ? *reinterpret_cast<const uint2*>(p) : make_uint2(0u, 0u);
            v[0] = widen<T>((unsigned short)q.x); v[1] = widen<T>((unsigned short)(q.x >> 16));
            v[2] = widen<T>((unsigned short)q.y); v[3] = widen<T>((unsigned short)(q.y >> 16));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (row_in && x0 + j < W) ? widen<T>(p[j]) : 0.f;
        }
    }
}

// a guarded 2-byte gate load without a branch: the address is p where ok, else safe (any element inside the tensor), the value selected
// afterwards.  A load inside the guard's branch has its pack behind a full vmcnt wait, which serialises a thread's gate loads
__device__ __forceinline__ unsigned short load16(const unsigned short* __restrict__ p, bool ok, const unsigned short* __restrict__ safe) {
    const unsigned short v = *(ok ? p : safe);
    return ok ? v : (unsigned short)0;
}

// the same four gates as the thread keeps them over the channel loop; safe: an element inside the gate tensor (16-bit scalar path)
template <bool VEC, class GT>
__device__ __forceinline__ void load_quad(Quad<GT>& g, const store_t<GT>* __restrict__ p, bool row_in, int x0, int W,
                                          const store_t<GT>* __restrict__ safe) {
    if constexpr (std::is_same<GT, float>::value) {
        load4<VEC>(g.v, p, row_in, x0, W);
    } else if (VEC) {
        const uint2 q = (row_in && x0 < W) ? *reinterpret_cast<const uint2*>(p) : make_uint2(0u, 0u);
        g.p[0] = q.x; g.p[1] = q.y;
    } else {
        g.clear();
#pragma unroll
        for (int j = 0; j < 4; ++j) g.put(j, load16(p + j, row_in && x0 + j < W, safe));
    }
}

template <bool VEC, class T = float>
__device__ __forceinline__ void store4(store_t<T>* __restrict__ p, const float (&v)[4], bool row_in, int x0, int W) {
    if (!row_in) return;
    if constexpr (std::is_same<T, float>::value) {
        if (VEC) {
            if (x0 < W) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) p[j] = v[j];
        }
    } else {
        if (VEC) {
            if (x0 < W)
                *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)narrow<T>(v[0]) | ((uint32_t)narrow<T>(v[1]) << 16),
                                                          (uint32_t)narrow<T>(v[2]) | ((uint32_t)narrow<T>(v[3]) << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x0 + j < W) p[j] = narrow<T>(v[j]);
        }
    }
}

// gate channel of the pair (t, l), l != R or t != R
template <int K>
__host__ __device__ constexpr int chan(int t, int l) { return t * K + l - (t * K + l > (K / 2) * (K + 1) ? 1 : 0); }

// what a collecting forward step and an injecting adjoint step take besides the step's own arguments (the assembling contract at the
// end of this file); the confidences conf [B][T][H][W] are shared by the C channels and, with a mask per channel, by the cpg images
// of a guidance image
struct Collect {
    const float* cj;   // the conf plane of the level this step produces, of guidance image 0; forward: NULL where that level is not collected
    const float* c0;   // forward, first step: the conf plane of a collected level 0 (conf_0 src joins the sum from the staged pixel), else NULL
    float* out;        // forward: the assembled output [N][C][H][W]; written, not read, unless accumulate
    const float* g;    // adjoint: grad_out [N][C][H][W]
    size_t stride;     // floats between the conf planes of two guidance images: T H W
    int cpg;           // images per guidance image (NormGeo)
    int accumulate;    // forward: out holds the levels collected so far
};

// one forward step for all C channels: dst = step(src).  VEC: W % 4 == 0, dst 16-byte aligned, gate aligned to four elements
// BIAS: the accumulator starts from bias [N][C][H][W] (the folded normalising contract, kxk_fold), 16-byte aligned where VEC
// ABS: gate is the raw guide; |gate| in the multiply-add, the sum times 1 / S before the store (0 * inf = NaN where a pixel's gates are all zero)
// COLLECT: after the stencil sum the thread also updates the assembled output of its four pixels, out (+)= conf_j acc (and conf_0 src in
// the first step); dst NULL: the level itself is not kept (the last one without a history); VEC: also out and conf 16-byte aligned
template <int K, bool VEC, bool BIAS, class GT, bool ABS, bool COLLECT, int D = 1>
__device__ __forceinline__ void forward_step_body(const store_t<GT>* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst, int C, int H,
                                                  int W, int tiles_x, int tiles_y, const float* __restrict__ bias, const Collect& col) {
    constexpr int R = K / 2, KK = K * K - 1, RD = R * D, SW = TW + 2 * RD;
    __shared__ float lds[(TH + 2 * RD) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    Quad<GT> g[KK];
    const store_t<GT>* gp = gate + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) load_quad<VEC, GT>(g[k], gp + (size_t)k * HW, row_in, T.x0, W, gate);
    // 1 / S of the thread's four pixels waits in LDS while the stencil runs: K = 7 in float32 has no register left for it
    __shared__ float4 rsl[ABS ? NT : 1];
    if constexpr (ABS) {
        float S[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KK; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] += g[k].mag(j);
        rsl[threadIdx.x] = make_float4(1.f / S[0], 1.f / S[1], 1.f / S[2], 1.f / S[3]);   // read back by this thread alone
    }
    // COLLECT: the epilogue's operands wait in LDS as well: conf_j, conf_0 and, per channel, what out holds.  Their loads are issued with
    // the gates' and the staged plane's and ride on those waits; loaded behind the stencil they are a dependent round trip to memory
    // per tile, loaded in front of it into registers they cost the step an occupancy (K = 7: 294 registers, one wave)
    __shared__ float4 park[COLLECT ? 3 * NT : 1];
    if constexpr (COLLECT) {
        const size_t cb = (size_t)(T.n / col.cpg) * col.stride + pix;
        float w[4];
        if (col.cj) {
            load4<VEC>(w, col.cj + cb, row_in, T.x0, W);
            park[threadIdx.x] = make_float4(w[0], w[1], w[2], w[3]);
        }
        if (col.c0) {
            load4<VEC>(w, col.c0 + cb, row_in, T.x0, W);
            park[NT + threadIdx.x] = make_float4(w[0], w[1], w[2], w[3]);
        }
    }
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)T.n * C + c) * HW;
        __syncthreads();   // the previous channel's reads of lds are done
        stage<RD>(lds, src + plane, T.y0, T.xt0, H, W);
        if constexpr (COLLECT) {
            if (col.accumulate) {
                float a[4];
                load4<VEC>(a, col.out + plane + pix, row_in, T.x0, W);
                park[2 * NT + threadIdx.x] = make_float4(a[0], a[1], a[2], a[3]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KK; ++k) g[k].pin();
        if constexpr (ABS) {
#pragma unroll
            for (int k = 0; k < KK; ++k) g[k].pin_sign();
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (BIAS) load4<VEC>(acc, bias + plane + pix, row_in, T.x0, W);
#pragma unroll
        for (int t = 0; t < K; ++t) {
            float row[4 + 2 * RD];   // row y + (R - t) D, columns x0 - R D .. x0 + 3 + R D
#pragma unroll
            for (int i = 0; i < 4 + 2 * RD; ++i) row[i] = lds[(T.ly + 2 * RD - t * D) * SW + 4 * T.lq + i];
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(ABS ? g[k].mag(j) : g[k].get(j), row[j + 2 * RD - l * D], acc[j]);
            }
        }
        if constexpr (ABS) {
            const float4 q = rsl[threadIdx.x];
            acc[0] *= q.x; acc[1] *= q.y; acc[2] *= q.z; acc[3] *= q.w;
        }
        if constexpr (COLLECT) {
            // the epilogue starts here, behind the stencil (the sums are operands, so this cannot move above it, and memory is clobbered,
            // so the parked values are read back, not kept): hoisted, it costs the step registers it does not have
            int px = pix;
            asm volatile("" : "+v"(px), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) : : "memory");
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            if (col.accumulate) {
                const float4 q = park[2 * NT + threadIdx.x];
                a[0] = q.x; a[1] = q.y; a[2] = q.z; a[3] = q.w;
            }
            if (col.c0) {   // level 0: the thread's own pixels of src, still staged
                const float4 q = park[NT + threadIdx.x];
                const float w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = w[j] * lds[(T.ly + RD) * SW + 4 * T.lq + RD + j];
            }
            if (col.cj) {
                const float4 q = park[threadIdx.x];
                const float w[4] = {q.x, q.y, q.z, q.w};
                const bool first = !col.accumulate && !col.c0;   // conf * acc as it is: with conf = 1 the bits of the level
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = first ? w[j] * acc[j] : fmaf(w[j], acc[j], a[j]);
            }
            store4<VEC>(col.out + plane + px, a, row_in, T.x0, W);
            if (dst) store4<VEC>(dst + plane + px, acc, row_in, T.x0, W);
        } else {
            store4<VEC>(dst + plane + pix, acc, row_in, T.x0, W);
        }
    }
}

template <int K, bool VEC, bool BIAS = false, class GT = float, bool ABS = false, int D = 1>
__global__ __launch_bounds__(NT) void kxk_forward_step(const store_t<GT>* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst,
                                                       int C, int H, int W, int tiles_x, int tiles_y, const float* __restrict__ bias) {
    forward_step_body<K, VEC, BIAS, GT, ABS, false, D>(gate, src, dst, C, H, W, tiles_x, tiles_y, bias, Collect{});
}

// the collecting form of the folded contract's step (float32 w' and b)
template <int K, bool VEC, int D = 1>
__global__ __launch_bounds__(NT) void kxk_forward_step_collect(const float* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst, int C,
                                                               int H, int W, int tiles_x, int tiles_y, const float* __restrict__ bias, Collect col) {
    forward_step_body<K, VEC, true, float, false, true, D>(gate, src, dst, C, H, W, tiles_x, tiles_y, bias, col);
}

// one adjoint step for all C channels: dst = step^T(src).  The gate of pixel q and channel k is read at q - off_k (zero outside the
// image); VEC: W % 4 == 0 and dst 16-byte aligned, 16-bit gates 8-byte aligned
// ABS: gate is the raw guide; src is staged times 1 / S (rs [N][H][W], or NULL: stage_scaled) and the stencil runs on |gate|
// INJECT: dst = step^T(src) + conf_j grad_out, added in the store epilogue (col.cj, col.g); VEC: also grad_out and conf 16-byte aligned
template <int K, bool VEC, class GT, bool ABS, bool INJECT, int D = 1>
__device__ __forceinline__ void adjoint_step_body(const store_t<GT>* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst, int C, int H,
                                                  int W, int tiles_x, int tiles_y, const float* __restrict__ rs, const Collect& col) {
    static_assert(D == 1 || (std::is_same<GT, float>::value && !ABS), "the dilated steps run on the folded contract's float32 w' only");
    constexpr int R = K / 2, KK = K * K - 1, RD = R * D, SW = TW + 2 * RD;
    __shared__ float lds[(TH + 2 * RD) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    Quad<GT> g[KK];
    const store_t<GT>* gb = gate + (size_t)T.n * KK * HW;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int py = T.y - R * D + t * D;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l);
            if constexpr (VEC && !std::is_same<GT, float>::value) {
                // 16-bit, W % 4 == 0 and the gates 8-byte aligned: the four gates x0 + d .. x0 + d + 3 (d = l - R) are a 64-bit window of
                // the aligned quads at x0 - 4, x0 and x0 + 4 (each all inside the row or all outside: zero): one or two 8-byte loads and
                // a funnel shift, no 2-byte load and no pack
                const store_t<GT>* row = gb + (size_t)k * HW + py * W;
                auto quad = [&](int x) {
                    return (yin && T.x0 < W && x >= 0 && x < W) ? *reinterpret_cast<const uint2*>(row + x) : make_uint2(0u, 0u);
                };
                const int s = l - R;   // compile-time after unrolling
                const uint2 b = quad(T.x0);
                uint32_t w[4];
                if (s < 0) {
                    const uint2 a = quad(T.x0 - 4);
                    w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
                } else {
                    const uint2 a = s > 0 ? quad(T.x0 + 4) : make_uint2(0u, 0u);
                    w[0] = b.x; w[1] = b.y; w[2] = a.x; w[3] = a.y;
                }
                const int e = s < 0 ? 4 + s : s, i = e >> 1;   // first element of the window in w, its word
                if (e & 1) {
                    g[k].p[0] = (w[i] >> 16) | (w[i + 1] << 16);
                    g[k].p[1] = (w[i + 1] >> 16) | (w[i + 2] << 16);
                } else {
                    g[k].p[0] = w[i];
                    g[k].p[1] = w[i + 1];
                }
                continue;
            }
            g[k].clear();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = T.x0 + j - R * D + l * D;
                const bool ok = yin && T.x0 + j < W && px >= 0 && px < W;
                if constexpr (std::is_same<GT, float>::value) {
                    if (ok) g[k].put(j, gb[(size_t)k * HW + py * W + px]);
                } else {
                    g[k].put(j, load16(gb + (size_t)k * HW + py * W + px, ok, gb));
                }
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)T.n * C + c) * HW;
        __syncthreads();
        if constexpr (ABS) stage_scaled<R, KK, GT>(lds, src + plane, rs ? rs + (size_t)T.n * HW : nullptr, gb, T.y0, T.xt0, H, W);
        else stage<RD>(lds, src + plane, T.y0, T.xt0, H, W);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KK; ++k) g[k].pin();
        if constexpr (ABS) {
#pragma unroll
            for (int k = 0; k < KK; ++k) g[k].pin_sign();
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            float row[4 + 2 * RD];   // row y - (R - t) D, columns x0 - R D .. x0 + 3 + R D
#pragma unroll
            for (int i = 0; i < 4 + 2 * RD; ++i) row[i] = lds[(T.ly + t * D) * SW + 4 * T.lq + i];
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(ABS ? g[k].mag(j) : g[k].get(j), row[j + l * D], acc[j]);
            }
        }
        if constexpr (INJECT) {
            int pix = T.y * W + T.x0;
            asm volatile("" : "+v"(pix), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) : : "memory");   // behind the stencil, as the collecting step's
            float w[4], go[4];
            load4<VEC>(w, col.cj + (size_t)(T.n / col.cpg) * col.stride + pix, row_in, T.x0, W);
            load4<VEC>(go, col.g + plane + pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[j], go[j], acc[j]);
        }
        store4<VEC>(dst + plane + T.y * W + T.x0, acc, row_in, T.x0, W);
    }
}

template <int K, bool VEC, class GT = float, bool ABS = false, int D = 1>
__global__ __launch_bounds__(NT) void kxk_adjoint_step(const store_t<GT>* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst,
                                                       int C, int H, int W, int tiles_x, int tiles_y, const float* __restrict__ rs) {
    adjoint_step_body<K, VEC, GT, ABS, false, D>(gate, src, dst, C, H, W, tiles_x, tiles_y, rs, Collect{});
}

// the injecting form, on the folded contract's float32 w'
template <int K, bool VEC, int D = 1>
__global__ __launch_bounds__(NT) void kxk_adjoint_step_inject(const float* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst, int C,
                                                              int H, int W, int tiles_x, int tiles_y, Collect col) {
    adjoint_step_body<K, VEC, float, false, true, D>(gate, src, dst, C, H, W, tiles_x, tiles_y, nullptr, col);
}

// the assembling contract's own reduction, per guidance image b and pixel p: dc(b,p) = sum_c G(b,c,p) lev(b,c,p), summed in channel order
// and written once (dc NULL: left out), and top(b,c,p) = cj(b,p) G(b,c,p), the scaled top adjoint level (top NULL: left out).  G, lev and
// top are [B][C][H][W]; cj and dc are one plane of [B][T][H][W] (stride: T H W).  VEC: W % 4 == 0 and all five 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(NT) void kxk_conf_grad(const float* __restrict__ G, const float* __restrict__ lev, const float* __restrict__ cj,
                                                    float* __restrict__ dc, float* __restrict__ top, size_t stride, int C, int H, int W, int tiles_x,
                                                    int tiles_y) {
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float w[4] = {0.f, 0.f, 0.f, 0.f}, sum[4] = {0.f, 0.f, 0.f, 0.f};
    if (top) load4<VEC>(w, cj + (size_t)T.n * stride + pix, row_in, T.x0, W);
    for (int c = 0; c < C; ++c) {
        const size_t at = ((size_t)T.n * C + c) * HW + pix;
        float go[4], h[4];
        load4<VEC>(go, G + at, row_in, T.x0, W);
        if (dc) {
            load4<VEC>(h, lev + at, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j] = fmaf(go[j], h[j], sum[j]);
        }
        if (top) {
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = w[j] * go[j];
            store4<VEC>(top + at, h, row_in, T.x0, W);
        }
    }
    if (dc) store4<VEC>(dc + (size_t)T.n * stride + pix, sum, row_in, T.x0, W);
}

// dL/dg for all KK channels of the tile: the levels H_0 = x, H_t = hist + (t - 1) L (t >= 1) and A_t = alev + (t - 1) L (t < n),
// A_n = gout, L = N C H W.  Accumulated over t = 0 .. n-1, then c = 0 .. C-1, written once (a 16-bit gg: rounded once, there).
// VEC: W % 4 == 0 and gg aligned to four elements.
// BIAS: also db [N][C][H][W] = sum_t A_{t+1} (dL/dbias of the folded contract); the loops then run over c, then t, and GATES = false
// leaves out the gate gradient (no H level is read, gg and hist unused); db 16-byte aligned where VEC
// ABS: the sums are dW of the ABS contract; the epilogue re-reads the raw guide (aligned to four elements where VEC) one channel at a
// time, twice, and writes dL/dg_k = sign(g_k) (dW_k - (sum_j |g_j| dW_j) r) r, r = 1 / S, sign(0) = 0
template <int K, bool VEC, bool BIAS = false, bool GATES = true, class GT = float, bool ABS = false, int D = 1>
__global__ __launch_bounds__(NT) void kxk_gate_grad(const float* __restrict__ x, const float* __restrict__ hist, const float* __restrict__ alev,
                                                    const float* __restrict__ gout, store_t<GT>* __restrict__ gg, int n_iter, size_t L, int C, int H,
                                                    int W, int tiles_x, int tiles_y, float* __restrict__ db, const store_t<GT>* __restrict__ guide) {
    static_assert(D == 1 || (BIAS && !ABS), "the dilated gate gradient is the folded contract's");
    constexpr int R = K / 2, KK = K * K - 1, RD = R * D, SW = TW + 2 * RD;
    __shared__ float lds[(TH + 2 * RD) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float acc[KK][4];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
    if constexpr (!BIAS) {
        for (int it = 0; it < n_iter; ++it) {
            const float* hl = it == 0 ? x : hist + (size_t)(it - 1) * L;
            const float* al = it + 1 == n_iter ? gout : alev + (size_t)it * L;
            for (int c = 0; c < C; ++c) {
                const size_t plane = ((size_t)T.n * C + c) * HW;
                __syncthreads();
                stage<RD>(lds, hl + plane, T.y0, T.xt0, H, W);
                float a[4];
                load4<false>(a, al + plane + pix, row_in, T.x0, W);
                __syncthreads();
#pragma unroll
                for (int t = 0; t < K; ++t) {
                    float row[4 + 2 * RD];
#pragma unroll
                    for (int i = 0; i < 4 + 2 * RD; ++i) row[i] = lds[(T.ly + 2 * RD - t * D) * SW + 4 * T.lq + i];
#pragma unroll
                    for (int l = 0; l < K; ++l) {
                        if (t == R && l == R) continue;
                        const int k = chan<K>(t, l);
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(a[j], row[j + 2 * RD - l * D], acc[k][j]);
                    }
                }
            }
        }
    } else {
        for (int c = 0; c < C; ++c) {
            const size_t plane = ((size_t)T.n * C + c) * HW;
            float d[4] = {0.f, 0.f, 0.f, 0.f};
            for (int it = 0; it < n_iter; ++it) {
                const float* al = it + 1 == n_iter ? gout : alev + (size_t)it * L;
                float a[4];
                load4<false>(a, al + plane + pix, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] += a[j];
                if constexpr (GATES) {
                    const float* hl = it == 0 ? x : hist + (size_t)(it - 1) * L;
                    __syncthreads();
                    stage<RD>(lds, hl + plane, T.y0, T.xt0, H, W);
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < K; ++t) {
                        float row[4 + 2 * RD];
#pragma unroll
                        for (int i = 0; i < 4 + 2 * RD; ++i) row[i] = lds[(T.ly + 2 * RD - t * D) * SW + 4 * T.lq + i];
#pragma unroll
                        for (int l = 0; l < K; ++l) {
                            if (t == R && l == R) continue;
                            const int k = chan<K>(t, l);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(a[j], row[j + 2 * RD - l * D], acc[k][j]);
                        }
                    }
                }
            }
            store4<VEC>(db + plane + pix, d, row_in, T.x0, W);
        }
    }
    if constexpr (ABS) {
        // four channels of the guide at a time, each group's loads through a pointer laundered after the group before it: left alone
        // the compiler gathers all KK loads above the sums and keeps their values for the second pass, in registers the kernel does not have
        constexpr int GB = 4;
        static_assert(KK % GB == 0, "the epilogue walks the guide four channels at a time");
        const store_t<GT>* up = guide + (size_t)T.n * KK * HW + pix;
        store_t<GT>* gp = gg + (size_t)T.n * KK * HW + pix;
        float S[4] = {0.f, 0.f, 0.f, 0.f}, dot[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k0 = 0; k0 < KK; k0 += GB) {
            float g[GB][4];
#pragma unroll
            for (int i = 0; i < GB; ++i) load4<VEC, GT>(g[i], up + (size_t)(k0 + i) * HW, row_in, T.x0, W);
#pragma unroll
            for (int i = 0; i < GB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    S[j] += fabsf(g[i][j]);
                    dot[j] = fmaf(fabsf(g[i][j]), acc[k0 + i][j], dot[j]);
                }
            asm volatile("" : "+v"(up), "+v"(dot[3]));   // the next four loads wait for these sums
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            S[j] = 1.f / S[j];
            dot[j] *= S[j];
        }
#pragma unroll
        for (int k0 = 0; k0 < KK; k0 += GB) {
            float g[GB][4];
#pragma unroll
            for (int i = 0; i < GB; ++i) load4<VEC, GT>(g[i], up + (size_t)(k0 + i) * HW, row_in, T.x0, W);
#pragma unroll
            for (int i = 0; i < GB; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[i][j] = signf(g[i][j]) * ((acc[k0 + i][j] - dot[j]) * S[j]);
                store4<VEC, GT>(gp + (size_t)(k0 + i) * HW, g[i], row_in, T.x0, W);
            }
            asm volatile("" : "+v"(up) : "v"(g[GB - 1][3]));
        }
        return;
    }
    if constexpr (GATES) {
        store_t<GT>* gp = gg + (size_t)T.n * KK * HW + pix;
#pragma unroll
        for (int k = 0; k < KK; ++k) store4<VEC, GT>(gp + (size_t)k * HW, acc[k], row_in, T.x0, W);
    }
}

// 1 / S of the ABS contract for the adjoint steps: rs [N][H][W] = 1 / sum_k |guide_k|, the sum and the division of kxk_forward_step.
// VEC: W % 4 == 0, guide aligned to four elements, rs 16-byte aligned
template <int K, bool VEC, class GT = float>
__global__ __launch_bounds__(NT) void kxk_rsum(const store_t<GT>* __restrict__ guide, float* __restrict__ rs, int H, int W, int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const store_t<GT>* up = guide + (size_t)T.n * KK * HW + pix;
    float S[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        float g[4];
        load4<VEC, GT>(g, up + (size_t)k * HW, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] += fabsf(g[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) S[j] = 1.f / S[j];
    store4<VEC>(rs + (size_t)T.n * HW + pix, S, row_in, T.x0, W);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
// four elements of the gate storage type: 16 bytes for float, 8 for a 16-bit type
template <class GT>
bool aligned_quad(const void* p) { return ((uintptr_t)p & (4 * sizeof(store_t<GT>) - 1)) == 0; }

struct Grid {
    int tx, ty;
    unsigned blocks;
};

Grid grid_of(int N, int H, int W) {
    Grid g;
    g.tx = (W + TW - 1) / TW;
    g.ty = (H + TH - 1) / TH;
    g.blocks = (unsigned)((size_t)N * g.tx * g.ty);
    return g;
}

// ---- the depth-completion contract (reference cspn.py:42-144 generalised to K x K) folded into the step above:
//   G_k(p) = g_k(p + off_k) (|g| for 8SUM_ABS), wb_k = G_k / sum_j |G_j|, c = 1 - sum_k wb_k, m = sign(sparse), u = 1 - m
//   H_{t+1}(p) = sum_k w'_k(p) H_t(p + off_k) + b(p),   w'_k = u wb_k (centre-sited, what kxk_forward_step reads), b = (u c + m) blur
// A mask of one plane per image (none, or [B,1]) keeps one w' for the C channels; a mask per channel ([B,C], C > 1) folds the channels into
// the batch: N' = B C images of one channel, each with its own w', cpg = C images per guidance image.

// G_k of the four pixels x0 .. x0+3 of row y: the guidance read at the neighbour (zero outside the image), abs for 8SUM_ABS
template <int K, class GT, int D = 1>
__device__ __forceinline__ void sited_gates(float (&G)[K * K - 1][4], const store_t<GT>* __restrict__ gb, bool row_in, int y, int x0, int H, int W,
                                            bool ab) {
    constexpr int R = K / 2;
    const int HW = H * W;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int py = y + R * D - t * D;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = x0 + j + R * D - l * D;
                const float v = (yin && x0 + j < W && px >= 0 && px < W) ? widen<GT>(gb[(size_t)k * HW + py * W + px]) : 0.f;
                G[k][j] = ab ? fabsf(v) : v;
            }
        }
    }
}

// m = sign(sparse) and u = 1 - m of image n (one plane per image, or none)
__device__ __forceinline__ void mask4(float (&m)[4], float (&u)[4], const float* __restrict__ sparse, int n, int HW, int pix, bool row_in, int x0,
                                      int W) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (sparse) load4<false>(s, sparse + (size_t)n * HW + pix, row_in, x0, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = signf(s[j]);
        u[j] = 1.f - m[j];
    }
}

// the pinned contract's mask: s = sparse, m = sign(s) pin_conf and u = 1 - m of image n (both one plane per image).  VEC: W % 4 == 0, sparse
// and pinc 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void mask4_pin(float (&m)[4], float (&u)[4], float (&s)[4], const float* __restrict__ sparse, const float* __restrict__ pinc, int n,
                                          int HW, int pix, bool row_in, int x0, int W) {
    float p[4];
    load4<VEC>(s, sparse + (size_t)n * HW + pix, row_in, x0, W);
    load4<VEC>(p, pinc + (size_t)n * HW + pix, row_in, x0, W);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        m[j] = signf(s[j]) * p[j];
        u[j] = 1.f - m[j];
    }
}

// w' [N'][KK][H][W] and b [N'][Cv][H][W] of image n' (guidance image n' / cpg).  VEC: W % 4 == 0, blur 16-byte aligned
template <int K, bool VEC, class GT = float, int D = 1>
__global__ __launch_bounds__(NT) void kxk_fold(const store_t<GT>* __restrict__ guid, const float* __restrict__ blur, const float* __restrict__ sparse,
                                               float* __restrict__ wp, float* __restrict__ bias, int Cv, int cpg, int norm, int H, int W, int tiles_x,
                                               int tiles_y) {
    constexpr int KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float G[KK][4];
    sited_gates<K, GT, D>(G, guid + (size_t)(T.n / cpg) * KK * HW, row_in, T.y, T.x0, H, W, norm == CSPN_NORM_8SUM_ABS);
    float S[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f}, m[4], u[4];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] += fabsf(G[k][j]);
    mask4(m, u, sparse, T.n, HW, pix, row_in, T.x0, W);
    float* wq = wp + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wb = G[k][j] / S[j];   // 0 / 0 = NaN, as the reference's torch.div
            gs[j] += wb;
            G[k][j] = u[j] * wb;
        }
        store4<VEC>(wq + (size_t)k * HW, G[k], row_in, T.x0, W);
    }
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = u[j] * (1.f - gs[j]) + m[j];
    for (int c = 0; c < Cv; ++c) {
        const size_t plane = ((size_t)T.n * Cv + c) * HW + pix;
        float v[4];
        load4<VEC>(v, blur + plane, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] *= f[j];
        store4<VEC>(bias + plane, v, row_in, T.x0, W);
    }
}

// kxk_fold of the pinned contract, a sibling kernel (kxk_fold itself stays the text, and so the code, it was): m = sign(sparse) pinc,
// w' = u wb, b = (u c) blur + m sparse, in this form: with pinc = 1 and blur = sparse where sparse > 0 it is (u c + m) blur bit for bit, with
// pinc = 0 the b of a call without a mask.  VEC: W % 4 == 0, blur, sparse and pinc 16-byte aligned
template <int K, bool VEC, class GT = float, int D = 1>
__global__ __launch_bounds__(NT) void kxk_fold_pin(const store_t<GT>* __restrict__ guid, const float* __restrict__ blur, const float* __restrict__ sparse,
                                                   const float* __restrict__ pinc, float* __restrict__ wp, float* __restrict__ bias, int Cv, int cpg,
                                                   int norm, int H, int W, int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float G[KK][4];
    sited_gates<K, GT, D>(G, guid + (size_t)(T.n / cpg) * KK * HW, row_in, T.y, T.x0, H, W, norm == CSPN_NORM_8SUM_ABS);
    float S[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f}, m[4], u[4];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) S[j] += fabsf(G[k][j]);
    float sv[4];
    mask4_pin<VEC>(m, u, sv, sparse, pinc, T.n, HW, pix, row_in, T.x0, W);
    float* wq = wp + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wb = G[k][j] / S[j];   // 0 / 0 = NaN, as the reference's torch.div
            gs[j] += wb;
            G[k][j] = u[j] * wb;
        }
        store4<VEC>(wq + (size_t)k * HW, G[k], row_in, T.x0, W);
    }
    float f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = u[j] * (1.f - gs[j]);
    for (int c = 0; c < Cv; ++c) {
        const size_t plane = ((size_t)T.n * Cv + c) * HW + pix;
        float v[4];
        load4<VEC>(v, blur + plane, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(m[j], sv[j], f[j] * v[j]);
        store4<VEC>(bias + plane, v, row_in, T.x0, W);
    }
}

// the pixel-local part of the fold's adjoint, per guidance image b and pixel p, images n' = b cpg + i:
//   dwb_k = sum_i u_i (dw'_{n',k} - sum_c blur_{n',c} db_{n',c}),  dG_k = (dwb_k - sign(G_k) sum_j wb_j dwb_j) / S  -> dw' of image b cpg
//   (in place: every element is read and written by the same thread), and where gx is given
//   gx_{n',c} = A_0 + (u_i c + m_i) db_{n',c} (gx holds A_0).  need_g = false: only the second.  VEC: W % 4 == 0, blur and gx 16-byte aligned
template <int K, bool VEC, class GT = float, int D = 1>
__global__ __launch_bounds__(NT) void kxk_unfold_pixel(const store_t<GT>* __restrict__ guid, const float* __restrict__ blur, const float* __restrict__ sparse,
                                                       float* __restrict__ dwp, const float* __restrict__ db, float* __restrict__ gx, int need_g, int Cv,
                                                       int cpg, int norm, int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const store_t<GT>* gb = guid + (size_t)T.n * KK * HW;
    const bool ab = norm == CSPN_NORM_8SUM_ABS;
    // G_k of the four pixels (kxk_fold's sited_gates, one channel at a time: the passes below re-read it from the cache rather than
    // keep KK x 4 values live)
    auto gate = [&](int t, int l, float (&v)[4]) {
        const int k = chan<K>(t, l), py = T.y + R * D - t * D;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int px = T.x0 + j + R * D - l * D;
            const float g = (yin && T.x0 + j < W && px >= 0 && px < W) ? widen<GT>(gb[(size_t)k * HW + py * W + px]) : 0.f;
            v[j] = ab ? fabsf(g) : g;
        }
    };
    float S[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < K; ++t)
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            float v[4];
            gate(t, l, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] += fabsf(v[j]);
        }
    const int n0 = T.n * cpg;
    if (need_g) {
        // u_i and sum_c blur db of image n0 + i
        auto ubd = [&](int i, float (&u)[4], float (&bd)[4]) {
            float m[4];
            mask4(m, u, sparse, n0 + i, HW, pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) bd[j] = 0.f;
            for (int c = 0; c < Cv; ++c) {
                const size_t plane = ((size_t)(n0 + i) * Cv + c) * HW + pix;
                float v[4], d[4];
                load4<VEC>(v, blur + plane, row_in, T.x0, W);
                load4<VEC>(d, db + plane, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) bd[j] = fmaf(v[j], d[j], bd[j]);
            }
        };
        float u0[4], bd0[4];
        ubd(0, u0, bd0);
        auto dwb = [&](int k, float (&d)[4]) {
            load4<VEC>(d, dwp + ((size_t)n0 * KK + k) * HW + pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = u0[j] * (d[j] - bd0[j]);
            for (int i = 1; i < cpg; ++i) {
                float u[4], bd[4], e[4];
                ubd(i, u, bd);
                load4<VEC>(e, dwp + ((size_t)(n0 + i) * KK + k) * HW + pix, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = fmaf(u[j], e[j] - bd[j], d[j]);
            }
        };
        float dot[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < K; ++t)
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                float v[4], d[4];
                gate(t, l, v);
                dwb(chan<K>(t, l), d);
#pragma unroll
                for (int j = 0; j < 4; ++j) dot[j] = fmaf(v[j] / S[j], d[j], dot[j]);
            }
        for (int t = 0; t < K; ++t)
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
                float v[4], d[4];
                gate(t, l, v);
                dwb(k, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = (d[j] - signf(v[j]) * dot[j]) / S[j];
                store4<VEC>(dwp + ((size_t)n0 * KK + k) * HW + pix, d, row_in, T.x0, W);
            }
    }
    if (!gx) return;
    for (int t = 0; t < K; ++t)
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            float v[4];
            gate(t, l, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) gs[j] += v[j] / S[j];   // c = 1 - sum_k wb_k, in channel order as kxk_fold
        }
    for (int i = 0; i < cpg; ++i) {
        float m[4], u[4];
        mask4(m, u, sparse, n0 + i, HW, pix, row_in, T.x0, W);
        for (int c = 0; c < Cv; ++c) {
            const size_t plane = ((size_t)(n0 + i) * Cv + c) * HW + pix;
            float a[4], d[4];
            load4<VEC>(a, gx + plane, row_in, T.x0, W);
            load4<VEC>(d, db + plane, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = fmaf(u[j] * (1.f - gs[j]) + m[j], d[j], a[j]);
            store4<VEC>(gx + plane, a, row_in, T.x0, W);
        }
    }
}

// kxk_unfold_pixel of the pinned contract, a sibling kernel (kxk_unfold_pixel itself stays the text, and so the code, it was; the two share
// mask4_pin's contract with kxk_fold_pin and the channel order of sited_gates): m = sign(sparse) pinc, dwb_k and dG_k as above with that u,
//   gx_{n',c} = A_0 + (u_i c) db_{n',c}, and per mask plane n'
//   gsp_{n'} = m sum_c db_{n',c}   and   gpp_{n'} = sign(sparse) (sum_c db_{n',c} (sparse - c blur_{n',c}) - sum_k wb_k dw'_{n',k})
//   (each may be NULL), the last sum in channel order and formed before dw' is overwritten in place; gpp needs dw' whatever need_g says.
//   Every element is written once.  VEC: W % 4 == 0, blur, gx, sparse, pinc, gsp and gpp 16-byte aligned
template <int K, bool VEC, class GT = float, int D = 1>
__global__ __launch_bounds__(NT) void kxk_unfold_pixel_pin(const store_t<GT>* __restrict__ guid, const float* __restrict__ blur,
                                                           const float* __restrict__ sparse, const float* __restrict__ pinc, float* __restrict__ dwp,
                                                           const float* __restrict__ db, float* __restrict__ gx, float* __restrict__ gsp,
                                                           float* __restrict__ gpp, int need_g, int Cv, int cpg, int norm, int H, int W, int tiles_x,
                                                           int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const store_t<GT>* gb = guid + (size_t)T.n * KK * HW;
    const bool ab = norm == CSPN_NORM_8SUM_ABS;
    // G_k of the four pixels (kxk_fold's sited_gates, one channel at a time: the passes below re-read it from the cache rather than
    // keep KK x 4 values live)
    auto gate = [&](int t, int l, float (&v)[4]) {
        const int k = chan<K>(t, l), py = T.y + R * D - t * D;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int px = T.x0 + j + R * D - l * D;
            const float g = (yin && T.x0 + j < W && px >= 0 && px < W) ? widen<GT>(gb[(size_t)k * HW + py * W + px]) : 0.f;
            v[j] = ab ? fabsf(g) : g;
        }
    };
    float S[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < K; ++t)
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            float v[4];
            gate(t, l, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] += fabsf(v[j]);
        }
    const int n0 = T.n * cpg;
    // dL/dsparse and dL/dpin come first: they read dw' of image n0, which the guidance gradient below overwrites in place
    if (gsp || gpp) {
        float cc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < K; ++t)
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                float v[4];
                gate(t, l, v);
#pragma unroll
                for (int j = 0; j < 4; ++j) cc[j] += v[j] / S[j];
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) cc[j] = 1.f - cc[j];
        for (int i = 0; i < cpg; ++i) {
            const size_t mp = (size_t)(n0 + i) * HW + pix;
            float m[4], u[4], s[4], ds[4] = {0.f, 0.f, 0.f, 0.f}, e[4] = {0.f, 0.f, 0.f, 0.f};
            mask4_pin<VEC>(m, u, s, sparse, pinc, n0 + i, HW, pix, row_in, T.x0, W);
            for (int c = 0; c < Cv; ++c) {
                const size_t plane = ((size_t)(n0 + i) * Cv + c) * HW + pix;
                float v[4], d[4];
                load4<VEC>(v, blur + plane, row_in, T.x0, W);
                load4<VEC>(d, db + plane, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ds[j] += d[j];
                    e[j] = fmaf(d[j], s[j] - cc[j] * v[j], e[j]);
                }
            }
            if (gpp) {
                float wd[4] = {0.f, 0.f, 0.f, 0.f};
                for (int t = 0; t < K; ++t)
                    for (int l = 0; l < K; ++l) {
                        if (t == R && l == R) continue;
                        float v[4], d[4];
                        gate(t, l, v);
                        load4<VEC>(d, dwp + ((size_t)(n0 + i) * KK + chan<K>(t, l)) * HW + pix, row_in, T.x0, W);
#pragma unroll
                        for (int j = 0; j < 4; ++j) wd[j] = fmaf(v[j] / S[j], d[j], wd[j]);
                    }
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = signf(s[j]) * (e[j] - wd[j]);
                store4<VEC>(gpp + mp, e, row_in, T.x0, W);
            }
            if (gsp) {
#pragma unroll
                for (int j = 0; j < 4; ++j) ds[j] *= m[j];
                store4<VEC>(gsp + mp, ds, row_in, T.x0, W);
            }
        }
    }
    if (need_g) {
        // u_i and sum_c blur db of image n0 + i
        auto ubd = [&](int i, float (&u)[4], float (&bd)[4]) {
            float m[4], s[4];
            mask4_pin<VEC>(m, u, s, sparse, pinc, n0 + i, HW, pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) bd[j] = 0.f;
            for (int c = 0; c < Cv; ++c) {
                const size_t plane = ((size_t)(n0 + i) * Cv + c) * HW + pix;
                float v[4], d[4];
                load4<VEC>(v, blur + plane, row_in, T.x0, W);
                load4<VEC>(d, db + plane, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) bd[j] = fmaf(v[j], d[j], bd[j]);
            }
        };
        float u0[4], bd0[4];
        ubd(0, u0, bd0);
        auto dwb = [&](int k, float (&d)[4]) {
            load4<VEC>(d, dwp + ((size_t)n0 * KK + k) * HW + pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) d[j] = u0[j] * (d[j] - bd0[j]);
            for (int i = 1; i < cpg; ++i) {
                float u[4], bd[4], e[4];
                ubd(i, u, bd);
                load4<VEC>(e, dwp + ((size_t)(n0 + i) * KK + k) * HW + pix, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = fmaf(u[j], e[j] - bd[j], d[j]);
            }
        };
        float dot[4] = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < K; ++t)
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                float v[4], d[4];
                gate(t, l, v);
                dwb(chan<K>(t, l), d);
#pragma unroll
                for (int j = 0; j < 4; ++j) dot[j] = fmaf(v[j] / S[j], d[j], dot[j]);
            }
        for (int t = 0; t < K; ++t)
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
                float v[4], d[4];
                gate(t, l, v);
                dwb(k, d);
#pragma unroll
                for (int j = 0; j < 4; ++j) d[j] = (d[j] - signf(v[j]) * dot[j]) / S[j];
                store4<VEC>(dwp + ((size_t)n0 * KK + k) * HW + pix, d, row_in, T.x0, W);
            }
    }
    if (!gx) return;
    for (int t = 0; t < K; ++t)
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            float v[4];
            gate(t, l, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) gs[j] += v[j] / S[j];   // c = 1 - sum_k wb_k, in channel order as kxk_fold
        }
    for (int i = 0; i < cpg; ++i) {
        float m[4], u[4], s[4];
        mask4_pin<VEC>(m, u, s, sparse, pinc, n0 + i, HW, pix, row_in, T.x0, W);
        for (int c = 0; c < Cv; ++c) {
            const size_t plane = ((size_t)(n0 + i) * Cv + c) * HW + pix;
            float a[4], d[4];
            load4<VEC>(a, gx + plane, row_in, T.x0, W);
            load4<VEC>(d, db + plane, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = fmaf(u[j] * (1.f - gs[j]), d[j], a[j]);
            store4<VEC>(gx + plane, a, row_in, T.x0, W);
        }
    }
}

// un-siting, a gather: dL/dguidance_k(q) = dG_k(q - off_k) (zero outside the image), times sign(g_k(q)) for 8SUM_ABS; dG of image b at
// dg + b cpg KK H W.  VEC: W % 4 == 0, guid and gg aligned to four elements.  A 16-bit gg is rounded here, at its only store
template <int K, bool VEC, class GT = float, int D = 1>
__global__ __launch_bounds__(NT) void kxk_unsite(const float* __restrict__ dg, const store_t<GT>* __restrict__ guid, store_t<GT>* __restrict__ gg, int cpg, int norm,
                                                 int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const float* db = dg + (size_t)T.n * cpg * KK * HW;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int py = T.y - R * D + t * D;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = T.x0 + j - R * D + l * D;
                v[j] = (yin && T.x0 + j < W && px >= 0 && px < W) ? db[(size_t)k * HW + py * W + px] : 0.f;
            }
            const size_t at = ((size_t)T.n * KK + k) * HW + pix;
            if (norm == CSPN_NORM_8SUM_ABS) {
                float g[4];
                load4<VEC, GT>(g, guid + at, row_in, T.x0, W);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] *= signf(g[j]);
            }
            store4<VEC, GT>(gg + at, v, row_in, T.x0, W);
        }
    }
}

// ---- the host dispatch: a runtime value as a template argument of a generic lambda (Tag / with_gate_type: cspn_gate16.h) ----
// K as a constant out of the contract's list (checked by the caller to be one of them)
template <int K0, int... Ks, class F>
int with_k(int K, F&& f) {
    if constexpr (sizeof...(Ks) == 0) return f(std::integral_constant<int, K0>{});
    else return K == K0 ? f(std::integral_constant<int, K0>{}) : with_k<Ks...>(K, f);
}

// a flag as std::bool_constant: VEC of a launch, which is then written once
template <class F>
auto with_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// the dilations of the folded and the assembling contract besides 1, the one list: a value added here is instantiated (with_dilation,
// cspn2d_kxk_dil.hip) and accepted (kxk_dilation_ok)
template <int... Ds>
struct DilationList {};
using Dilations = DilationList<2>;

template <class F, int... Ds>
int with_dilation(DilationList<Ds...>, int D, F&& f) { return with_k<Ds...>(D, f); }

template <int... Ds>
bool dilation_listed(DilationList<Ds...>, int D) { return ((D == Ds) || ...); }

template <int K, bool BIAS = false, class GT = float, bool ABS = false, int D = 1>
int forward_step(const store_t<GT>* gate, const float* src, float* dst, const Grid& G, int C, int H, int W, hipStream_t st, const float* bias) {
    with_bool(W % 4 == 0 && aligned_quad<GT>(gate) && aligned16(dst) && (!BIAS || aligned16(bias)), [&](auto vec) {
        hipLaunchKernelGGL((kxk_forward_step<K, decltype(vec)::value, BIAS, GT, ABS, D>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty,
                           bias);
    });
    return check_launch("kxk_forward_step");
}

template <int K, bool BIAS = false, class GT = float, bool ABS = false, int D = 1>
int forward_steps(const store_t<GT>* gate, const float* x, float* out, float* hist, int N, int C, int H, int W, int n_iter, void* ws, hipStream_t st,
                  const float* bias = nullptr) {
    const Grid G = grid_of(N, H, W);
    const size_t L = (size_t)N * C * H * W;
    float* ping = (float*)ws;
    float* pong = ping + kxk_level_floats(L);
    const float* src = x;
    for (int it = 1; it <= n_iter; ++it) {
        float* dst = it == n_iter ? out : (hist ? hist + (size_t)(it - 1) * L : ((it & 1) ? ping : pong));
        if (int e = forward_step<K, BIAS, GT, ABS, D>(gate, src, dst, G, C, H, W, st, bias)) return e;
        src = dst;
    }
    return 0;
}

template <int K, class GT = float, bool ABS = false, int D = 1>
int adjoint_step(const store_t<GT>* gate, const float* src, float* dst, const Grid& G, int C, int H, int W, hipStream_t st, const float* rs) {
    with_bool(W % 4 == 0 && aligned16(dst) && (std::is_same<GT, float>::value || aligned_quad<GT>(gate)), [&](auto vec) {
        hipLaunchKernelGGL((kxk_adjoint_step<K, decltype(vec)::value, GT, ABS, D>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty, rs);
    });
    return check_launch("kxk_adjoint_step");
}

// the adjoint steps A_{n-1} .. A_last into alev (A_t at alev + (t - 1) L), A_0 into gx; ABS: rs as kxk_adjoint_step takes it
template <int K, class GT = float, bool ABS = false, int D = 1>
int adjoint_steps(const store_t<GT>* gate, const float* gout, float* gx, float* alev, int last, int N, int C, int H, int W, int n_iter, hipStream_t st,
                  const float* rs = nullptr) {
    const Grid G = grid_of(N, H, W);
    const size_t L = (size_t)N * C * H * W;
    for (int t = n_iter - 1; t >= last; --t) {
        const float* src = t + 1 == n_iter ? gout : alev + (size_t)t * L;
        float* dst = t == 0 ? gx : alev + (size_t)(t - 1) * L;
        if (int e = adjoint_step<K, GT, ABS, D>(gate, src, dst, G, C, H, W, st, rs)) return e;
    }
    return 0;
}

// ABS: gate is the raw guide; with n_iter >= 2 the plane of 1 / S follows the adjoint levels in ws (kxk_absnorm_alev_bytes)
template <int K, class GT = float, bool ABS = false>
int backward_run(const store_t<GT>* gate, const float* x, const float* hist, const float* gout, store_t<GT>* gg, float* gx, int N, int C, int H, int W,
                 int n_iter, void* ws, hipStream_t st) {
    const Grid G = grid_of(N, H, W);
    const size_t L = (size_t)N * C * H * W;
    float* alev = (float*)ws;   // A_1 .. A_{n-1}, level t at alev + (t - 1) L
    const float* rs = nullptr;
    if (ABS && n_iter >= 2) {
        float* r = (float*)((char*)ws + kxk_absnorm_alev_bytes(L, n_iter));
        with_bool(W % 4 == 0 && aligned_quad<GT>(gate), [&](auto vec) {
            hipLaunchKernelGGL((kxk_rsum<K, decltype(vec)::value, GT>), dim3(G.blocks), dim3(NT), 0, st, gate, r, H, W, G.tx, G.ty);
        });
        if (int e = check_launch("kxk_rsum")) return e;
        rs = r;
    }
    // the adjoint steps: A_{n-1} .. A_1 always (the gate gradient reads them), A_0 = dL/dx where asked for
    if (int e = adjoint_steps<K, GT, ABS>(gate, gout, gx, alev, gx ? 0 : (gg ? 1 : n_iter), N, C, H, W, n_iter, st, rs)) return e;
    if (!gg) return 0;
    with_bool(W % 4 == 0 && aligned_quad<GT>(gg) && (!ABS || aligned_quad<GT>(gate)), [&](auto vec) {
        hipLaunchKernelGGL((kxk_gate_grad<K, decltype(vec)::value, false, true, GT, ABS>), dim3(G.blocks), dim3(NT), 0, st, x, hist, alev, gout, gg, n_iter, L,
                           C, H, W, G.tx, G.ty, nullptr, gate);
    });
    return check_launch("kxk_gate_grad");
}

// the views of the folded contract: N' images of Cv channels, cpg of them per guidance image
struct NormGeo {
    int N, Cv, cpg;
    size_t L;
};

NormGeo norm_geo(int B, int C, int sparse_C, int H, int W) {
    const bool pc = sparse_C > 1;
    return NormGeo{pc ? B * C : B, pc ? 1 : C, pc ? C : 1, (size_t)B * C * H * W};
}

// PIN (a trailing template argument of the host paths below, default off): the pinned contract, pin (KxkPin, cspn_common.h) its confidence
// and where dL/dsparse and dL/dpin go.  Only the fold and its adjoint differ; the steps between them are the unpinned contract's
template <int K, class GT = float, int D = 1, bool PIN = false>
int fold(const store_t<GT>* guid, const float* blur, const float* sparse, float* wp, float* bias, const NormGeo& g, int norm, int H, int W, hipStream_t st,
         const KxkPin& pin = KxkPin{}) {
    const Grid G = grid_of(g.N, H, W);
    if constexpr (PIN) {
        with_bool(W % 4 == 0 && aligned16(blur) && aligned16(sparse) && aligned16(pin.conf), [&](auto vec) {
            hipLaunchKernelGGL((kxk_fold_pin<K, decltype(vec)::value, GT, D>), dim3(G.blocks), dim3(NT), 0, st, guid, blur, sparse, pin.conf, wp, bias, g.Cv,
                               g.cpg, norm, H, W, G.tx, G.ty);
        });
        return check_launch("kxk_fold_pin");
    } else {
        with_bool(W % 4 == 0 && aligned16(blur), [&](auto vec) {
            hipLaunchKernelGGL((kxk_fold<K, decltype(vec)::value, GT, D>), dim3(G.blocks), dim3(NT), 0, st, guid, blur, sparse, wp, bias, g.Cv, g.cpg, norm, H, W,
                               G.tx, G.ty);
        });
        return check_launch("kxk_fold");
    }
}

// the steps run on the float32 w' and b whatever the guidance's type
template <int K, class GT = float, int D = 1, bool PIN = false>
int norm_forward(const store_t<GT>* guid, const float* blur, const float* sparse, float* out, float* hist, int B, int C, int sparse_C, int H, int W,
                 int n_iter, int norm, void* ws, hipStream_t st, const KxkPin& pin = KxkPin{}) {
    constexpr int KK = K * K - 1;
    const NormGeo g = norm_geo(B, C, sparse_C, H, W);
    float* wp = (float*)ws;
    float* bias = wp + kxk_level_floats((size_t)g.N * KK * H * W);
    if (int e = fold<K, GT, D, PIN>(guid, blur, sparse, wp, bias, g, norm, H, W, st, pin)) return e;
    return forward_steps<K, true, float, false, D>(wp, blur, out, hist, g.N, g.Cv, H, W, n_iter, bias + kxk_level_floats(g.L), st, bias);
}

// the parts of the folded contract's backward workspace: w' and b, dL/dw' and dL/db, A_1 .. A_{n-1}, and what follows them (the assembling
// contract's scaled top level)
struct NormBackwardWs {
    float *wp, *bias, *dwp, *dbp, *alev, *top;
};

template <int K>
NormBackwardWs norm_backward_ws(void* ws, const NormGeo& g, int H, int W, int n_iter) {
    const size_t P = kxk_level_floats((size_t)g.N * (K * K - 1) * H * W);
    NormBackwardWs w;
    w.wp = (float*)ws;
    w.bias = w.wp + P;
    w.dwp = w.bias + kxk_level_floats(g.L);
    w.dbp = w.dwp + P;
    w.alev = w.dbp + kxk_level_floats(g.L);
    w.top = (float*)((char*)w.alev + round256(sizeof(float) * g.L * (size_t)(n_iter - 1)));
    return w;
}

// after the adjoint steps: the gate gradient with dL/db (atop: the top adjoint level A_n), the fold's adjoint per pixel, the gather back
// PIN: dL/dpin needs dL/dw' as the guidance gradient does, so it too asks for the gate gradient's GATES pass (and its history)
template <int K, class GT = float, int D = 1, bool PIN = false>
int norm_backward_finish(const store_t<GT>* guid, const float* blur, const float* sparse, const float* hist, const float* atop, store_t<GT>* gg, float* gx,
                         int B, const NormGeo& g, const NormBackwardWs& w, int H, int W, int n_iter, int norm, hipStream_t st, const KxkPin& pin = KxkPin{}) {
    float *dwp = w.dwp, *dbp = w.dbp, *alev = w.alev;
    const float* gout = atop;
    const Grid G = grid_of(g.N, H, W);
    const bool vec = W % 4 == 0;   // dwp and dbp: workspace
    with_bool(vec, [&](auto v) {
        with_bool(gg != nullptr || (PIN && pin.gp != nullptr), [&](auto gates) {
            hipLaunchKernelGGL((kxk_gate_grad<K, decltype(v)::value, true, decltype(gates)::value, float, false, D>), dim3(G.blocks), dim3(NT), 0, st, blur, hist, alev, gout,
                               dwp, n_iter, g.L, g.Cv, H, W, G.tx, G.ty, dbp, nullptr);
        });
    });
    if (int e = check_launch("kxk_gate_grad")) return e;
    const Grid GB = grid_of(B, H, W);
    if constexpr (PIN) {
        with_bool(vec && aligned16(blur) && (!gx || aligned16(gx)) && aligned16(sparse) && aligned16(pin.conf) && (!pin.gs || aligned16(pin.gs)) &&
                      (!pin.gp || aligned16(pin.gp)),
                  [&](auto v) {
                      hipLaunchKernelGGL((kxk_unfold_pixel_pin<K, decltype(v)::value, GT, D>), dim3(GB.blocks), dim3(NT), 0, st, guid, blur, sparse, pin.conf, dwp,
                                         dbp, gx, pin.gs, pin.gp, gg ? 1 : 0, g.Cv, g.cpg, norm, H, W, GB.tx, GB.ty);
                  });
    } else {
        with_bool(vec && aligned16(blur) && (!gx || aligned16(gx)), [&](auto v) {
            hipLaunchKernelGGL((kxk_unfold_pixel<K, decltype(v)::value, GT, D>), dim3(GB.blocks), dim3(NT), 0, st, guid, blur, sparse, dwp, dbp, gx, gg ? 1 : 0,
                               g.Cv, g.cpg, norm, H, W, GB.tx, GB.ty);
        });
    }
    if (int e = check_launch("kxk_unfold_pixel")) return e;
    if (!gg) return 0;
    with_bool(vec && aligned_quad<GT>(guid) && aligned_quad<GT>(gg), [&](auto v) {
        hipLaunchKernelGGL((kxk_unsite<K, decltype(v)::value, GT, D>), dim3(GB.blocks), dim3(NT), 0, st, dwp, guid, gg, g.cpg, norm, H, W, GB.tx, GB.ty);
    });
    return check_launch("kxk_unsite");
}

template <int K, class GT = float, int D = 1, bool PIN = false>
int norm_backward(const store_t<GT>* guid, const float* blur, const float* sparse, const float* hist, const float* gout, store_t<GT>* gg, float* gx, int B, int C,
                  int sparse_C, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, const KxkPin& pin = KxkPin{}) {
    const NormGeo g = norm_geo(B, C, sparse_C, H, W);
    const NormBackwardWs w = norm_backward_ws<K>(ws, g, H, W, n_iter);
    if (int e = fold<K, GT, D, PIN>(guid, blur, sparse, w.wp, w.bias, g, norm, H, W, st, pin)) return e;
    if (int e = adjoint_steps<K, float, false, D>(w.wp, gout, gx, w.alev, gx ? 0 : 1, g.N, g.Cv, H, W, n_iter, st)) return e;
    return norm_backward_finish<K, GT, D, PIN>(guid, blur, sparse, hist, gout, gg, gx, B, g, w, H, W, n_iter, norm, st, pin);
}

// ---- the assembling contract: out = sum_j conf_j H_{s_j} over the levels of the folded contract, s_0 < .. < s_{T-1} = n (host array steps),
// conf [B][T][H][W].  hist: NULL, or H_1 .. H_n (level t at hist + (t - 1) B C H W: H_n is no longer the output) ----
template <int K, class GT = float, int D = 1, bool PIN = false>
int assemble_forward(const store_t<GT>* guid, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out, float* hist,
                     int B, int C, int sparse_C, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, const KxkPin& pin = KxkPin{}) {
    constexpr int KK = K * K - 1;
    const NormGeo g = norm_geo(B, C, sparse_C, H, W);
    const size_t HW = (size_t)H * W;
    float* wp = (float*)ws;
    float* bias = wp + kxk_level_floats((size_t)g.N * KK * HW);
    float* ping = bias + kxk_level_floats(g.L);
    float* pong = ping + kxk_level_floats(g.L);
    if (int e = fold<K, GT, D, PIN>(guid, blur, sparse, wp, bias, g, norm, H, W, st, pin)) return e;
    const Grid G = grid_of(g.N, H, W);
    const float* src = blur;
    int j = steps[0] == 0 ? 1 : 0;
    const float* c0 = j ? conf : nullptr;   // a collected level 0 rides on the first step
    bool started = false;
    for (int it = 1; it <= n_iter; ++it) {
        const bool hit = j < T && steps[j] == it;
        float* dst = hist ? hist + (size_t)(it - 1) * g.L : (it == n_iter ? nullptr : ((it & 1) ? ping : pong));
        if (!hit && !c0) {
            if (int e = forward_step<K, true, float, false, D>(wp, src, dst, G, g.Cv, H, W, st, bias)) return e;
        } else {
            const Collect col{hit ? conf + (size_t)j * HW : nullptr, c0, out, nullptr, (size_t)T * HW, g.cpg, started ? 1 : 0};
            with_bool(W % 4 == 0 && aligned16(wp) && aligned16(dst) && aligned16(bias) && aligned16(out) && aligned16(conf), [&](auto vec) {
                hipLaunchKernelGGL((kxk_forward_step_collect<K, decltype(vec)::value, D>), dim3(G.blocks), dim3(NT), 0, st, wp, src, dst, g.Cv, H, W, G.tx, G.ty,
                                   bias, col);
            });
            if (int e = check_launch("kxk_forward_step_collect")) return e;
            started = true;
            c0 = nullptr;
            j += hit;
        }
        src = dst;
    }
    return 0;
}

// gg, gx and gc (dL/dconf [B][T][H][W]) may each be NULL; ws: the folded backward's, then the scaled top level A_n = conf_{T-1} grad_out
template <int K, class GT = float, int D = 1, bool PIN = false>
int assemble_backward(const store_t<GT>* guid, const float* blur, const float* sparse, const float* conf, const int* steps, int T, const float* hist,
                      const float* gout, store_t<GT>* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int n_iter, int norm, void* ws,
                      hipStream_t st, const KxkPin& pin = KxkPin{}) {
    const NormGeo g = norm_geo(B, C, sparse_C, H, W);
    const NormBackwardWs w = norm_backward_ws<K>(ws, g, H, W, n_iter);
    const size_t HW = (size_t)H * W, stride = (size_t)T * HW;
    const bool levels = gg || gx || (PIN && (pin.gs || pin.gp));   // the adjoint sweep runs
    const Grid GB = grid_of(B, H, W);
    for (int j = 0; j < T; ++j) {   // dL/dconf_j, and with the last one the top level
        float* top = levels && j == T - 1 ? w.top : nullptr;
        float* dc = gc ? gc + (size_t)j * HW : nullptr;
        if (!top && !dc) continue;
        const float* lev = steps[j] == 0 ? blur : hist + (size_t)(steps[j] - 1) * g.L;
        const float* cj = conf + (size_t)j * HW;
        with_bool(W % 4 == 0 && aligned16(gout) && aligned16(conf) && (!dc || (aligned16(lev) && aligned16(gc))), [&](auto vec) {
            hipLaunchKernelGGL((kxk_conf_grad<decltype(vec)::value>), dim3(GB.blocks), dim3(NT), 0, st, gout, lev, cj, dc, top, stride, C, H, W, GB.tx, GB.ty);
        });
        if (int e = check_launch("kxk_conf_grad")) return e;
    }
    if (!levels) return 0;
    if (int e = fold<K, GT, D, PIN>(guid, blur, sparse, w.wp, w.bias, g, norm, H, W, st, pin)) return e;
    const Grid G = grid_of(g.N, H, W);
    int j = T - 2;   // the next collected level below the one being produced
    for (int t = n_iter - 1; t >= (gx ? 0 : 1); --t) {
        const float* src = t + 1 == n_iter ? w.top : w.alev + (size_t)t * g.L;
        float* dst = t == 0 ? gx : w.alev + (size_t)(t - 1) * g.L;
        if (j >= 0 && steps[j] == t) {
            const Collect col{conf + (size_t)j * HW, nullptr, nullptr, gout, stride, g.cpg, 0};
            with_bool(W % 4 == 0 && aligned16(dst) && aligned16(gout) && aligned16(conf), [&](auto vec) {
                hipLaunchKernelGGL((kxk_adjoint_step_inject<K, decltype(vec)::value, D>), dim3(G.blocks), dim3(NT), 0, st, w.wp, src, dst, g.Cv, H, W, G.tx, G.ty,
                                   col);
            });
            if (int e = check_launch("kxk_adjoint_step_inject")) return e;
            --j;
        } else if (int e = adjoint_step<K, float, false, D>(w.wp, src, dst, G, g.Cv, H, W, st, nullptr)) {
            return e;
        }
    }
    return norm_backward_finish<K, GT, D, PIN>(guid, blur, sparse, hist, w.top, gg, gx, B, g, w, H, W, n_iter, norm, st, pin);
}

}  // namespace

}  // namespace cspn
