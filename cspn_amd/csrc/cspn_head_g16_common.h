// cspn_head_g16_common.h -- what the 16-bit heads (cspn_head_kxk_g16.hip: 24 / 48 planes, 16-bit guidance; cspn_head_g16.hip: 8 planes, float32 guidance)
// share: the fragment types and the single rounding, the weights' repack into operand fragments, and the dL/dW GEMM, which takes dL/dguidance and dL/dblur as
// DT planes and any plane count O.  The layouts are described at the top of cspn_head_kxk_g16.hip.
#pragma once
#include <cstdint>

#include "cspn_head_kxk_common.h"

namespace cspn {
namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef unsigned short us;

template <bool BF>
__device__ __forceinline__ f16v mfma16(u4 a, u4 b, f16v c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// the single rounding of a float32 value to DT: to nearest even, overflow to +-inf, subnormals kept, NaN stays NaN
template <bool BF>
__device__ __forceinline__ us narrow(float v) {
    if constexpr (!BF) return __builtin_bit_cast(us, (_Float16)v);
    else {
        const uint32_t u = __float_as_uint(v);
        if ((u & 0x7fffffffu) > 0x7f800000u) return (us)0x7fc0;
        return (us)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
    }
}

__device__ __forceinline__ u4 pack8(const us (&v)[8]) {
    u4 r;
#pragma unroll
    for (int m = 0; m < 4; ++m) r[m] = (uint32_t)v[2 * m] | ((uint32_t)v[2 * m + 1] << 16);
    return r;
}

// the weights of both heads, rounded to DT, as operand fragments: wp[(kb * 9 + tap) * Nr + row] = 8 DT over k = kb * 8 + j.  k_channel (forward): k = channel,
// row = plane; else (dL/dx): k = plane, row = channel.  Zeros beyond O planes / C channels and for the blur plane (o = O - 1) without a blur head.
template <bool BF>
__global__ __launch_bounds__(256) void hk16_pack_kernel(const float* __restrict__ wg, const float* __restrict__ wb, us* __restrict__ wp, int C, int O, int Nk8,
                                                        int Nr, int k_channel) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Nk8 * 9 * Nr * 8) return;
    const int jj = idx & 7, u = idx >> 3;
    const int row = u % Nr, tap = (u / Nr) % 9, kb = u / (Nr * 9);
    const int k = kb * 8 + jj;
    const int c = k_channel ? k : row, o = k_channel ? row : k;
    float v = 0.f;
    if (c < C) {
        if (o < O - 1) v = wg[((size_t)o * C + c) * 9 + tap];
        else if (o == O - 1 && wb) v = wb[(size_t)c * 9 + tap];
    }
    wp[idx] = narrow<BF>(v);
}

// ---- dL/dW ----------------------------------------------------------------------------------------------------------------------------
// D[row T = o * 9 + r * 3 + k][channel] += sum over pixels g[o][2i - 1 + r][2j - 1 + k] x[channel][i][j].  A tile = 16 consecutive pixels of an input row: lanes
// 0-31 take pixels jb .. jb + 7, lanes 32-63 the next eight: one matrix step per (row block, channel block).  blockIdx.y = the group of DW_TB row blocks; a wave
// takes a contiguous share of the tiles.
constexpr int DW_TILE = 16;

template <bool BF, int NB>
__global__ __launch_bounds__(256, 2) void hk16_bwd_w_kernel(const us* __restrict__ x, const us* __restrict__ gg, const us* __restrict__ gb, float* __restrict__ part,
                                                             int C, int c0, int h, int w, int H, int W, int O, int tiles, int tiles_w, int hfed, int nwave) {
    __shared__ float red[DwSize<NB>::floats];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = blockIdx.x * 4 + wv, lane = threadIdx.x & 63;
    const int tg = blockIdx.y;
    const int t0 = wave < nwave ? (int)((long long)tiles * wave / nwave) : 0, t1 = wave < nwave ? (int)((long long)tiles * (wave + 1) / nwave) : 0;
    const int half = lane >> 5, id = lane & 31;
    const size_t HWo = (size_t)H * W, hw = (size_t)h * w;
    const int rows = 9 * O;
    const int ntb = (rows + 31) / 32 - tg * DW_TB;                 // row blocks of this group that hold rows at all (wave-uniform)
    int tr[DW_TB], tk[DW_TB];
    const us* tsrc[DW_TB];             // plane of image 0 (a padding row / no blur head: some valid plane, never used)
    bool tvalid[DW_TB];
    size_t tstep[DW_TB];               // from one image to the next
#pragma unroll
    for (int tb = 0; tb < DW_TB; ++tb) {
        const int t = (tg * DW_TB + tb) * 32 + id;
        const int o = t / 9;
        tr[tb] = (t - o * 9) / 3;
        tk[tb] = t - o * 9 - tr[tb] * 3;
        tvalid[tb] = t < rows && (o < O - 1 || gb != nullptr);
        const bool blur = tvalid[tb] && o == O - 1;
        tsrc[tb] = blur ? gb : gg + (size_t)(o < O - 1 ? o : 0) * HWo;
        tstep[tb] = blur ? HWo : (size_t)(O - 1) * HWo;
    }
    const us* xsrc[NB];
    bool xvalid[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { const int ch = c0 + nb * 32 + id; xvalid[nb] = ch < C; xsrc[nb] = x + (size_t)(ch < C ? ch : 0) * hw; }
    struct Tile { u4 a[DW_TB]; u4 bq[NB]; };
    auto load = [&](Tile& T, int tw, int i, int b) {       // tile tw of input row i of image b
        const int jb = tw * DW_TILE + 8 * half;               // this lane's first pixel
#pragma unroll
        for (int tb = 0; tb < DW_TB; ++tb) {
            if (tb >= ntb) continue;
            const int Y = 2 * i - 1 + tr[tb], Xb = 2 * jb - 1 + tk[tb];
            const bool rowok = tvalid[tb] && Y >= 0 && Y < H;
            const us* p = tsrc[tb] + (size_t)b * tstep[tb] + (size_t)(rowok ? Y : 0) * W;
            if (!rowok) {
                T.a[tb] = u4{0u, 0u, 0u, 0u};
            } else if (Xb >= 0 && Xb + 15 < W) {              // the common case: 16 consecutive DT, every other one is a pixel's
                uint32_t q[8];
                __builtin_memcpy(q, p + Xb, 32);
#pragma unroll
                for (int m = 0; m < 4; ++m) T.a[tb][m] = (q[2 * m] & 0xffffu) | (q[2 * m + 1] << 16);
            } else {                                          // the first / last tiles of a row: what lies outside is zero
                us v[8];
#pragma unroll
                for (int s_ = 0; s_ < 8; ++s_) {
                    const int X = Xb + 2 * s_;
                    const bool in = X >= 0 && X < W;
                    const us t = p[in ? X : 0];
                    v[s_] = in ? t : (us)0;
                }
                T.a[tb] = pack8(v);
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const us* p = xsrc[nb] + (size_t)b * C * hw + (size_t)i * w;
            if (!xvalid[nb]) {
                T.bq[nb] = u4{0u, 0u, 0u, 0u};
            } else if (jb + 7 < w && 2 * (jb + 7) < W) {
                __builtin_memcpy(&T.bq[nb], p + jb, 16);
            } else {
                us v[8];
#pragma unroll
                for (int s_ = 0; s_ < 8; ++s_) {
                    const int jx = jb + s_;
                    const bool in = jx < w && 2 * jx < W;      // (beyond the narrowed output: fed nothing)
                    const us t = p[in ? jx : 0];
                    v[s_] = in ? t : (us)0;
                }
                T.bq[nb] = pack8(v);
            }
        }
    };
    f16v acc[DW_TB][NB];
#pragma unroll
    for (int tb = 0; tb < DW_TB; ++tb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[tb][nb][q] = 0.f;
    Tile nxt;
#pragma unroll
    for (int tb = 0; tb < DW_TB; ++tb) nxt.a[tb] = u4{0u, 0u, 0u, 0u};
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) nxt.bq[nb] = u4{0u, 0u, 0u, 0u};
    int tw = 0, ti = 0, tb_ = 0;
    if (t0 < t1) {
        tw = (int)((unsigned)t0 % (unsigned)tiles_w);
        ti = (int)(((unsigned)t0 / (unsigned)tiles_w) % (unsigned)hfed);
        tb_ = (int)((unsigned)t0 / ((unsigned)tiles_w * (unsigned)hfed));
        load(nxt, tw, ti, tb_);
    }
    for (int t = t0; t < t1; ++t) {
        const Tile cur = nxt;
        if (++tw == tiles_w) { tw = 0; if (++ti == hfed) { ti = 0; ++tb_; } }      // the next tile (scalar)
        if (t + 1 < t1) load(nxt, tw, ti, tb_);
#pragma unroll
        for (int tb = 0; tb < DW_TB; ++tb) {
            if (tb >= ntb) continue;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[tb][nb] = mfma16<BF>(cur.a[tb], cur.bq[nb], acc[tb][nb]);
        }
    }
    // the workgroup's four blocks, added in wave order
    for (int turn = 0; turn < 4; ++turn) {
        if (wv == turn) {
#pragma unroll
            for (int tb = 0; tb < DW_TB; ++tb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        float* r = &red[((tb * NB + nb) * 16 + q) * 64 + lane];
                        *r = turn == 0 ? acc[tb][nb][q] : *r + acc[tb][nb][q];
                    }
        }
        __syncthreads();
    }
    float* dst = part + ((size_t)tg * gridDim.x + blockIdx.x) * DwSize<NB>::floats;
    for (int e = threadIdx.x; e < DwSize<NB>::floats; e += 256) dst[e] = red[e];
}

}  // namespace
}  // namespace cspn
