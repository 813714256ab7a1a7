// cspn_head_kxk_g16.hip -- the guidance heads for 5x5 and 7x7 propagation on fp16 / bf16 feature maps (what a backbone under autocast hands over), forward and
// backward: the three GEMMs of cspn_head_kxk.hip on v_mfma_f32_32x32x16_{f16,bf16}.  x, the guidance planes, their gradient and dL/dx are stored in the 16-bit
// type DT; the weights arrive as float32 masters and are rounded to DT once, in the per-call repack; the blur plane leaves as float32 (the accumulator) and its
// gradient arrives as float32 and is rounded to DT once as it enters the GEMMs.  Every product is of two DT values (exact in float32), the sums are float32.
//   The matrix instruction sums over 16 k per step: lane l (id = l % 32, half = l / 32) holds A[row id][k = 8 half + j] and B[k = 8 half + j][column id] in
//   element j = 0 .. 7 of a 4-register fragment; D as the fp32 form (lane: column id; register q: row (q / 4) * 8 + half * 4 + q % 4).
//   * forward:  k = the channel.  x is plane-major, so a lane gathers its pixel's 8 channels with 8 two-byte loads (a half-wave's 32 lanes read 64 contiguous
//     bytes of one channel's row per load) and packs them; the weights come as ready fragments [channel block of 8][tap][plane] (hk16_pack_kernel).
//   * dL/dx:    k = the output plane (the blur plane rides as plane O - 1, already rounded to DT in the workspace); the same gather over 8 planes.
//   * dL/dW:    k = the pixel: a tile is 16 consecutive pixels of an input row, a lane reads its row's window values (16 consecutive DT, every other one a
//     pixel's) and its channel's 8 pixels (16 bytes).  Partial blocks are added in wave order through LDS, then in workgroup order: no atomics, deterministic.
// Addresses are clamped and values selected: nothing is read outside a tensor, whatever lies outside feeds a zero.
#include "cspn_head_g16_common.h"

namespace cspn {
namespace {

// dL/dblur as it enters the GEMMs: rounded once to DT
template <bool BF>
__global__ __launch_bounds__(256) void hk16_round_kernel(const float* __restrict__ in, us* __restrict__ out, size_t n) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < n) out[idx] = narrow<BF>(in[idx]);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// One wave = PT input rows x 32 columns x all O planes (OB blocks of 32).  wp: hk16_pack_kernel k_channel, [2 * Cs][9][On] fragments (Cs = steps of 16 channels).
// fast: W % 4 == 0 and guidance 8-byte aligned -- neighbouring lanes trade a row, so that a lane stores four pixels of one output row (8 bytes).
template <bool BF, int OB, int PT>
__global__ __launch_bounds__(256, 2) void hk16_fwd_kernel(const us* __restrict__ x, const u4* __restrict__ wp, us* __restrict__ gout, float* __restrict__ bout,
                                                           int C, int h, int w, int H, int W, int B, int O, int fast) {
    constexpr int On = OB * 32;
    const int wq = (w + 31) / 32, hp = (h + PT - 1) / PT;
    const int unit = wave_unit();
    const int seg = unit % wq;
    const int i0 = PT * ((unit / wq) % hp), b = unit / (wq * hp);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, half = lane >> 5, id = lane & 31;
    const int j = seg * 32 + id;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    bool ok[PT + 1][2];
    unsigned off[PT + 1][2];
#pragma unroll
    for (int r = 0; r <= PT; ++r) {
        const int i = i0 + r;
        const bool rok = i < h && 2 * i < H;
        const unsigned ro = (unsigned)(i < h ? i : h - 1) * (unsigned)w;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            ok[r][e] = rok && j + e < w && 2 * (j + e) < W;
            off[r][e] = ro + (unsigned)(j + e < w ? j + e : w - 1);
        }
    }
    const us* xb = x + (size_t)b * C * hw;
    const int Cs = (C + 15) >> 4;
    struct Ops { u4 xv[PT + 1][2]; };
    auto load = [&](Ops& T, int s) {
        const int cb = s * 16 + half * 8;
#pragma unroll
        for (int r = 0; r <= PT; ++r)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                us v[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int ch = cb + jj;
                    const us t = xb[(size_t)(ch < C ? ch : C - 1) * hw + off[r][e]];
                    v[jj] = (ch < C && ok[r][e]) ? t : (us)0;
                }
                T.xv[r][e] = pack8(v);
            }
    };
    f16v P00[OB][PT], P01[OB][PT], P10[OB][PT], P11[OB][PT];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int pr = 0; pr < PT; ++pr)
#pragma unroll
            for (int q = 0; q < 16; ++q) P00[ob][pr][q] = P01[ob][pr][q] = P10[ob][pr][q] = P11[ob][pr][q] = 0.f;
    for (int s = 0; s < Cs; ++s) {       // (128 accumulator registers leave no room for a second set of operands: the SIMD's other wave covers the loads)
        Ops cur;
        load(cur, s);
        const u4* ws = wp + (size_t)(s * 2 + half) * 9 * On + id;
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            u4 k[9];
#pragma unroll
            for (int t = 0; t < 9; ++t) k[t] = ws[t * On + ob * 32];
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const u4 x00 = cur.xv[pr][0], x01 = cur.xv[pr][1], x10 = cur.xv[pr + 1][0], x11 = cur.xv[pr + 1][1];
                P00[ob][pr] = mfma16<BF>(k[4], x00, P00[ob][pr]);       // W11
                P01[ob][pr] = mfma16<BF>(k[3], x00, P01[ob][pr]);       // W10
                P10[ob][pr] = mfma16<BF>(k[1], x00, P10[ob][pr]);       // W01
                P11[ob][pr] = mfma16<BF>(k[0], x00, P11[ob][pr]);       // W00
                P01[ob][pr] = mfma16<BF>(k[5], x01, P01[ob][pr]);       // W12
                P10[ob][pr] = mfma16<BF>(k[7], x10, P10[ob][pr]);       // W21
                P11[ob][pr] = mfma16<BF>(k[2], x01, P11[ob][pr]);       // W02
                P11[ob][pr] = mfma16<BF>(k[6], x10, P11[ob][pr]);       // W20
                P11[ob][pr] = mfma16<BF>(k[8], x11, P11[ob][pr]);       // W22
            }
        }
    }
    // (no early return: the lanes of a pair trade rows below; a pair shares its half, so it shares every plane index and every branch on one)
    const bool mine = j < w && 2 * j < W;
    const int X0 = 2 * j;
    const bool two = X0 + 1 < W;
    const bool odd = id & 1;
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int o = ob * 32 + (q >> 2) * 8 + half * 4 + (q & 3);
            if (o >= O) continue;
            if (o == O - 1) {                                           // the blur plane: the float32 accumulator, a pixel's two outputs of a row in 8 bytes
                if (!bout || !mine) continue;
                float* dst = bout + (size_t)b * HWo;
#pragma unroll
                for (int pr = 0; pr < PT; ++pr) {
                    const int i = i0 + pr;
                    if (i >= h) continue;
                    auto put2 = [&](int Y, float va, float vb) {
                        if (Y >= H) return;
                        float* d = dst + (size_t)Y * W + X0;
                        if (two) { const float v[2] = {va, vb}; __builtin_memcpy(d, v, 8); }
                        else d[0] = va;
                    };
                    put2(2 * i, P00[ob][pr][q], P01[ob][pr][q]);
                    put2(2 * i + 1, P10[ob][pr][q], P11[ob][pr][q]);
                }
                continue;
            }
            us* dst = gout + ((size_t)b * (O - 1) + o) * HWo;
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const int i = i0 + pr;
                if (i >= h) continue;
                const uint32_t r0 = (uint32_t)narrow<BF>(P00[ob][pr][q]) | ((uint32_t)narrow<BF>(P01[ob][pr][q]) << 16);    // row 2i:     X0, X0 + 1
                const uint32_t r1 = (uint32_t)narrow<BF>(P10[ob][pr][q]) | ((uint32_t)narrow<BF>(P11[ob][pr][q]) << 16);    // row 2i + 1
                if (fast) {
                    // the even lane of a pair takes row 2i of both (X0 .. X0 + 3, X0 a multiple of 4), the odd lane row 2i + 1; W % 4 == 0: a pair is inside
                    // the output together or not at all
                    const uint32_t got = (uint32_t)__shfl_xor((int)(odd ? r0 : r1), 1);
                    const int Y = 2 * i + (odd ? 1 : 0);
                    if (mine && Y < H) {
                        const uint32_t v[2] = {odd ? got : r0, odd ? r1 : got};
                        __builtin_memcpy(dst + (size_t)Y * W + (X0 & ~3), v, 8);
                    }
                } else if (mine) {
                    if (2 * i < H) { us* d = dst + (size_t)(2 * i) * W + X0; d[0] = (us)r0; if (two) d[1] = (us)(r0 >> 16); }
                    if (2 * i + 1 < H) { us* d = dst + (size_t)(2 * i + 1) * W + X0; d[0] = (us)r1; if (two) d[1] = (us)(r1 >> 16); }
                }
            }
        }
}

// ---- dL/dx ----------------------------------------------------------------------------------------------------------------------------
// One wave = one input row x 32 columns x CB blocks of 32 channels (from c0).  wq: hk16_pack_kernel, [2 * Os][9][Cn] fragments (Os = steps of 16 planes).
// The window of pixel (i, j): g[o][2i - 1 + r][2j - 1 + k], whose weight is W[o][c][2 - r][2 - k].  gb: dL/dblur rounded to DT, or null.
template <bool BF, int CB>
__global__ __launch_bounds__(256, 2) void hk16_bwd_x_kernel(const us* __restrict__ gg, const us* __restrict__ gb, const u4* __restrict__ wq, us* __restrict__ dx,
                                                             int C, int c0, int Cn, int h, int w, int H, int W, int B, int O) {
    const int wq_ = (w + 31) / 32;
    const int unit = wave_unit();
    const int seg = unit % wq_;
    const int i = (unit / wq_) % h, b = unit / (wq_ * h);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, half = lane >> 5, id = lane & 31;
    const int j = seg * 32 + id;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    bool ok[3][3];
    unsigned off[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int Y = 2 * i - 1 + r;
        const bool yok = Y >= 0 && Y < H;
        const unsigned ro = (unsigned)(Y < 0 ? 0 : (Y >= H ? H - 1 : Y)) * (unsigned)W;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int X = 2 * j - 1 + k;
            ok[r][k] = yok && X >= 0 && X < W;
            off[r][k] = ro + (unsigned)(X < 0 ? 0 : (X >= W ? W - 1 : X));
        }
    }
    const int Os = (O + 15) >> 4;
    const us* gimg = gg + (size_t)b * (O - 1) * HWo;
    f16v acc[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[cb][q] = 0.f;
    for (int s = 0; s < Os; ++s) {
        const us* src[8];
        bool ook[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            const int o = s * 16 + half * 8 + jj;
            ook[jj] = o < O - 1 || (o == O - 1 && gb != nullptr);
            src[jj] = !ook[jj] ? gimg : (o < O - 1 ? gimg + (size_t)o * HWo : gb + (size_t)b * HWo);
        }
        u4 gv[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                us v[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const us t = src[jj][off[r][k]];
                    v[jj] = (ook[jj] && ok[r][k]) ? t : (us)0;
                }
                gv[r][k] = pack8(v);
            }
        const u4* ws = wq + (size_t)(s * 2 + half) * 9 * Cn + c0 + id;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int tap = (2 - r) * 3 + (2 - k);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) acc[cb] = mfma16<BF>(ws[tap * Cn + cb * 32], gv[r][k], acc[cb]);
            }
    }
    if (j >= w) return;
    const bool fed = 2 * i < H && 2 * j < W;       // (an input whose unpooled position lies beyond the narrowed output fed nothing: gradient 0)
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int c = c0 + cb * 32 + (q >> 2) * 8 + half * 4 + (q & 3);
            if (c >= C) continue;
            dx[((size_t)b * C + c) * hw + (size_t)i * w + j] = fed ? narrow<BF>(acc[cb][q]) : (us)0;
        }
}

size_t bwd_x_pack_bytes(int C, int O) { return round256((size_t)((O + 15) >> 4) * 2 * 9 * ((C + 31) & ~31) * 16); }
size_t blur16_bytes(int B, int h, int w) { return round256((size_t)B * (2 * h) * (2 * w) * 2); }

template <bool BF>
int forward_g16(const us* x, const float* wg, const float* wb, us* gout, float* bout, int B, int C, int h, int w, int H, int W, int K, void* ws, hipStream_t st) {
    const int O = K * K, On = (O + 31) & ~31, Cs = (C + 15) >> 4;
    // (one input row per wave at both K: a lane's 8 two-byte loads per operand sit in 8 registers until they are packed, and a second row's do not fit
    // beside K = 5's accumulators without scratch)
    const unsigned groups = groups_of((long long)B * h * ((w + 31) / 32));
    const long long halves = (long long)Cs * 2 * 9 * On * 8;
    if (!groups || halves >= (1ll << 31)) { set_error("cspn_guidance_head_kxk_g16: too many pixels or channels for one launch"); return CSPN_E_UNSUPPORTED; }
    hipLaunchKernelGGL(hk16_pack_kernel<BF>, dim3((unsigned)((halves + 255) / 256)), dim3(256), 0, st, wg, wb, (us*)ws, C, O, Cs * 2, On, 1);
    const int fast = (W % 4 == 0) && ((uintptr_t)gout % 8 == 0);
    if (K == 5) hipLaunchKernelGGL((hk16_fwd_kernel<BF, 1, 1>), dim3(groups), dim3(256), 0, st, x, (const u4*)ws, gout, bout, C, h, w, H, W, B, O, fast);
    else hipLaunchKernelGGL((hk16_fwd_kernel<BF, 2, 1>), dim3(groups), dim3(256), 0, st, x, (const u4*)ws, gout, bout, C, h, w, H, W, B, O, fast);
    return check_launch("hk16_fwd_kernel");
}

template <bool BF>
int backward_g16(const us* x, const float* wg, const float* wb, const us* gg, const float* gb, us* dx, float* dwg, float* dwb, int B, int C, int h, int w, int H,
                 int W, int K, void* ws, hipStream_t st) {
    static const char* what = "cspn_guidance_head_kxk_backward_g16";
    const int O = K * K;
    us* gb16 = nullptr;
    if (gb) {
        gb16 = (us*)((char*)ws + bwd_x_pack_bytes(C, O));
        const size_t n = (size_t)B * H * W;
        hipLaunchKernelGGL(hk16_round_kernel<BF>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, gb, gb16, n);
    }
    if (dx) {
        const int Os = (O + 15) >> 4, Cn = (C + 31) & ~31;
        const unsigned groups = groups_of((long long)B * h * ((w + 31) / 32));
        const long long halves = (long long)Os * 2 * 9 * Cn * 8;
        if (!groups || halves >= (1ll << 31)) { set_error("%s: too many pixels or channels for one launch", what); return CSPN_E_UNSUPPORTED; }
        hipLaunchKernelGGL(hk16_pack_kernel<BF>, dim3((unsigned)((halves + 255) / 256)), dim3(256), 0, st, wg, wb, (us*)ws, C, O, Os * 2, Cn, 0);
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time (two row blocks of the matrix core)
            if (C - c0 > 32) hipLaunchKernelGGL((hk16_bwd_x_kernel<BF, 2>), dim3(groups), dim3(256), 0, st, gg, gb16, (const u4*)ws, dx, C, c0, Cn, h, w, H, W, B, O);
            else hipLaunchKernelGGL((hk16_bwd_x_kernel<BF, 1>), dim3(groups), dim3(256), 0, st, gg, gb16, (const u4*)ws, dx, C, c0, Cn, h, w, H, W, B, O);
        }
        if (int e = check_launch("hk16_bwd_x_kernel")) return e;
    }
    if (dwg || dwb) {
        float* part = (float*)((char*)ws + bwd_x_pack_bytes(C, O) + blur16_bytes(B, h, w));
        const DwGeo G(B, h, w, H, W, O, DW_TILE);
        if (!G.fits) { set_error("%s: too many pixels", what); return CSPN_E_UNSUPPORTED; }
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time (two column blocks of the matrix core)
            const int NB = C - c0 > 32 ? 2 : 1;
            if (NB == 2) hipLaunchKernelGGL((hk16_bwd_w_kernel<BF, 2>), dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg, gb16, part, C, c0, h, w, H, W, O, G.tiles, G.tiles_w, G.hfed, G.nwave);
            else hipLaunchKernelGGL((hk16_bwd_w_kernel<BF, 1>), dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg, gb16, part, C, c0, h, w, H, W, O, G.tiles, G.tiles_w, G.hfed, G.nwave);
            head_kxk_dw_reduce(part, dwg, dwb, C, c0, NB, O, G.nwg, st);
        }
        if (int e = check_launch("hk16_bwd_w_kernel")) return e;
    }
    return 0;
}

}  // namespace

// the forward's weight fragments ([C rounded up to 16 / 8][9][32 or 64] x 16 bytes)
size_t head_kxk_g16_workspace(int C, int K) {
    const int On = (K * K + 31) & ~31;
    return round256((size_t)((C + 15) >> 4) * 2 * 9 * On * 16);
}

int head_kxk_g16_forward(const void* x, int dtype, const float* wg, const float* wb, void* gout, float* bout, int B, int C, int h, int w, int H, int W, int K,
                         void* ws, hipStream_t st) {
    return dtype == CSPN_DTYPE_F16 ? forward_g16<false>((const us*)x, wg, wb, (us*)gout, bout, B, C, h, w, H, W, K, ws, st)
                                   : forward_g16<true>((const us*)x, wg, wb, (us*)gout, bout, B, C, h, w, H, W, K, ws, st);
}

// dL/dx's weight fragments + dL/dblur rounded to DT + the workgroups' partial blocks of dL/dW (64 channels at a time)
size_t head_kxk_g16_backward_workspace(int B, int C, int h, int w, int K) {
    const int O = K * K;
    return bwd_x_pack_bytes(C, O) + blur16_bytes(B, h, w) + (size_t)row_groups(O) * DW_MAX_WG * DwSize<2>::floats * sizeof(float);
}

int head_kxk_g16_backward(const void* x, int dtype, const float* wg, const float* wb, const void* gg, const float* gb, void* dx, float* dwg, float* dwb, int B,
                          int C, int h, int w, int H, int W, int K, void* ws, hipStream_t st) {
    return dtype == CSPN_DTYPE_F16 ? backward_g16<false>((const us*)x, wg, wb, (const us*)gg, gb, (us*)dx, dwg, dwb, B, C, h, w, H, W, K, ws, st)
                                   : backward_g16<true>((const us*)x, wg, wb, (const us*)gg, gb, (us*)dx, dwg, dwb, B, C, h, w, H, W, K, ws, st);
}

}  // namespace cspn
