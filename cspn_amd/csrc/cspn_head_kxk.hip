// cspn_head_kxk.hip -- the guidance heads for 5x5 and 7x7 propagation: Simple_Gudi_UpConv_Block_Last_Layer(C, K*K-1, ...) (reference
// cspn_pytorch/models/torch_resnet_cspn_nyu.py:187-206: Unpool :41-54, narrowed to oheight x owidth, + bias-free 3x3 conv) with the 1-plane blur head riding
// along, forward and backward.  O = K*K-1 guidance planes + 1 blur plane = 25 or 49 output planes.
//     out[o][Y][X] = sum_{c,ky,kx} W[o][c][ky][kx] U[c][Y + ky - 1][X + kx - 1],   U[c][2i][2j] = x[c][i][j], zeros elsewhere / beyond the narrowed H x W
//     dL/dx[c][i][j]      = sum_{o,ky,kx} W[o][c][ky][kx] g[o][2i + 1 - ky][2j + 1 - kx]                        (g = dL/dout, zero outside the output)
//     dL/dW[o][c][ky][kx] = sum_{b,i,j}   x[b][c][i][j]   g[b][o][2i + 1 - ky][2j + 1 - kx]
// The structure is the 8-plane head's (cspn_head.hip): an input pixel (i, j) owns the 2 x 2 output block, with 1, 2, 2 and 4 non-zero taps for the four output
// parities -- 9 products per input pixel, channel and output plane, not 36:
//     out[2i  ][2j  ] = W11 x00                      out[2i  ][2j+1] = W10 x00 + W12 x01
//     out[2i+1][2j  ] = W01 x00 + W21 x10            out[2i+1][2j+1] = W00 x00 + W02 x01 + W20 x10 + W22 x11
// 25 or 49 planes x 4 parities do not fit the vector unit's registers the way 9 planes do: all three products are GEMMs on the matrix cores, exact fp32
// (v_mfma_f32_32x32x2_f32: A 32 x 2 -- lane l: row l % 32, k = l / 32 --, B 2 x 32 -- lane l: k = l / 32, column l % 32 --, D 32 x 32 in 16 registers -- lane l:
// column l % 32; register q: row (q / 4) * 8 + (l / 32) * 4 + q % 4).
//   * forward:  D_parity[o][pixel] += W[o][c][tap] x[c][pixel + shift(tap)]: rows = output planes (padded to 32 / 64), columns = 32 pixels of an input row,
//     k = a channel pair.  "lane = pixel, half-wave = channel" IS the B layout: a half-wave reads 128 contiguous bytes of its channel's row straight into the
//     operand register (the right neighbour: the same lines again, one float on), so the feature map comes from HBM once and needs no detour through LDS.
//     A wave keeps 4 parities x (planes x rows = 2 blocks) x 16 = 128 accumulator registers: K = 5 one plane block and two input rows, K = 7 two plane blocks and
//     one row.  The next channel pair's operands are requested before the current pair's 18 matrix instructions.
//   * dL/dx:    D[c][pixel] += W[o][c][tap] g[o][window(tap) of pixel]: rows = channels (blocks of 32, 64 per launch), columns = 32 pixels, k = a plane pair.
//   * dL/dW:    D[(o, tap)][c] += g[o][window(tap) of pixel] x[c][pixel]: the GEMM of head_bwd_w_kernel (cspn_head_backward.hip) with 9 * O = 225 / 441 rows
//     (8 / 14 blocks of 32) in place of 81; a launch's blockIdx.y takes 4 row blocks (128 accumulator registers with two channel blocks), a workgroup's four
//     waves add their blocks in wave order through LDS, hk_bwd_w_reduce_kernel adds the workgroups' blocks in workgroup order: no atomics, deterministic.
#include <cstdint>

#include "cspn_head_kxk_common.h"

namespace cspn {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int REC = 12;            // floats per (plane, channel) weight record: the 9 taps [ky][kx] + 3 of padding (three 16-byte loads)

// the weights of both heads as records: c_major (forward) [c < Cn][o < On][12], else (dL/dx) [o < On][c < Cn][12]; zeros beyond O planes / C channels and for
// the blur plane (o = O - 1) when there is no blur head
__global__ __launch_bounds__(256) void hk_pack_kernel(const float* __restrict__ wg, const float* __restrict__ wb, float* __restrict__ wp, int C, int O, int Cn,
                                                      int On, int c_major) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cn * On * REC) return;
    const int t = idx % REC, u = idx / REC;
    const int c = c_major ? u / On : u % Cn, o = c_major ? u % On : u / Cn;
    float v = 0.f;
    if (t < 9 && c < C) {
        if (o < O - 1) v = wg[((size_t)o * C + c) * 9 + t];
        else if (o == O - 1 && wb) v = wb[(size_t)c * 9 + t];
    }
    wp[idx] = v;
}

__device__ __forceinline__ f16v mfma(float a, float b, f16v c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// One wave = PT input rows (i0 .. i0 + PT - 1) x 32 columns x all O planes (OB blocks of 32).  wp: hk_pack_kernel c_major, [C rounded up to even][OB * 32][12].
template <int OB, int PT>
__global__ __launch_bounds__(256, 2) void hk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp, float* __restrict__ gout,
                                                         float* __restrict__ bout, int C, int h, int w, int H, int W, int B, int O) {
    constexpr int On = OB * 32;
    const int wq = (w + 31) / 32, hp = (h + PT - 1) / PT;
    const int unit = wave_unit();
    const int seg = unit % wq;
    const int i0 = PT * ((unit / wq) % hp), b = unit / (wq * hp);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, half = lane >> 5, id = lane & 31;
    const int j = seg * 32 + id;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    // every mask and every clamped offset is the same for all channels: feature rows i0 .. i0 + PT, columns j and j + 1; what lies beyond the image or beyond
    // the narrowed output fed nothing (zero)
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
    const float* xb = x + (size_t)b * C * hw;
    const int Ce = (C + 1) & ~1;
    struct Ops { float xv[PT + 1][2]; f4 k[OB][3]; };
    auto load = [&](Ops& T, int c0) {
        const int ch = c0 + half;
        const bool cok = ch < C;
        const float* xc = xb + (size_t)(cok ? ch : C - 1) * hw;
#pragma unroll
        for (int r = 0; r <= PT; ++r)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float v = xc[off[r][e]];
                T.xv[r][e] = (cok && ok[r][e]) ? v : 0.f;
            }
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            const f4* rec = reinterpret_cast<const f4*>(wp + ((size_t)ch * On + ob * 32 + id) * REC);
            T.k[ob][0] = rec[0]; T.k[ob][1] = rec[1]; T.k[ob][2] = rec[2];
        }
    };
    f16v P00[OB][PT], P01[OB][PT], P10[OB][PT], P11[OB][PT];
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int pr = 0; pr < PT; ++pr)
#pragma unroll
            for (int q = 0; q < 16; ++q) P00[ob][pr][q] = P01[ob][pr][q] = P10[ob][pr][q] = P11[ob][pr][q] = 0.f;
    Ops nxt;
    load(nxt, 0);
    for (int c0 = 0; c0 < Ce; c0 += 2) {
        const Ops cur = nxt;
        if (c0 + 2 < Ce) load(nxt, c0 + 2);
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
            const f4 k0 = cur.k[ob][0], k1 = cur.k[ob][1], k2 = cur.k[ob][2];   // taps 0-3, 4-7, 8
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const float x00 = cur.xv[pr][0], x01 = cur.xv[pr][1], x10 = cur.xv[pr + 1][0], x11 = cur.xv[pr + 1][1];
                P00[ob][pr] = mfma(k1[0], x00, P00[ob][pr]);       // W11
                P01[ob][pr] = mfma(k0[3], x00, P01[ob][pr]);       // W10
                P10[ob][pr] = mfma(k0[1], x00, P10[ob][pr]);       // W01
                P11[ob][pr] = mfma(k0[0], x00, P11[ob][pr]);       // W00
                P01[ob][pr] = mfma(k1[1], x01, P01[ob][pr]);       // W12
                P10[ob][pr] = mfma(k1[3], x10, P10[ob][pr]);       // W21
                P11[ob][pr] = mfma(k0[2], x01, P11[ob][pr]);       // W02
                P11[ob][pr] = mfma(k1[2], x10, P11[ob][pr]);       // W20
                P11[ob][pr] = mfma(k2[0], x11, P11[ob][pr]);       // W22
            }
        }
    }
    if (j >= w || 2 * j >= W) return;
    const int X0 = 2 * j;
    const bool two = X0 + 1 < W;
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int o = ob * 32 + (q >> 2) * 8 + half * 4 + (q & 3);
            if (o >= O) continue;
            float* dst = o < O - 1 ? gout + ((size_t)b * (O - 1) + o) * HWo : (bout ? bout + (size_t)b * HWo : nullptr);
            if (!dst) continue;
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const int i = i0 + pr;
                if (i >= h) continue;
                // a pixel's two outputs of a row are neighbours in memory: one 8-byte store where both exist; every element is written once
                auto put2 = [&](int Y, float va, float vb) {
                    if (Y >= H) return;                                  // (the narrowed output)
                    float* d = dst + (size_t)Y * W + X0;
                    if (two) { const float v[2] = {va, vb}; __builtin_memcpy(d, v, 8); }
                    else d[0] = va;
                };
                put2(2 * i, P00[ob][pr][q], P01[ob][pr][q]);
                put2(2 * i + 1, P10[ob][pr][q], P11[ob][pr][q]);
            }
        }
}

// ---- dL/dx ----------------------------------------------------------------------------------------------------------------------------
// One wave = PT input rows x 32 columns x CB blocks of 32 channels (from c0).  wq: hk_pack_kernel o_major, [O rounded up to even][Cn = C rounded up to 32][12].
// The window of pixel (i, j): g[o][2i - 1 + r][2j - 1 + k], whose weight is W[o][c][2 - r][2 - k].
template <int CB, int PT>
__global__ __launch_bounds__(256, 2) void hk_bwd_x_kernel(const float* __restrict__ gg, const float* __restrict__ gb, const float* __restrict__ wq,
                                                           float* __restrict__ dx, int C, int c0, int Cn, int h, int w, int H, int W, int B, int O) {
    const int wq_ = (w + 31) / 32, hp = (h + PT - 1) / PT;
    const int unit = wave_unit();
    const int seg = unit % wq_;
    const int i0 = PT * ((unit / wq_) % hp), b = unit / (wq_ * hp);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, half = lane >> 5, id = lane & 31;
    const int j = seg * 32 + id;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    bool ok[PT][3][3];
    unsigned off[PT][3][3];
#pragma unroll
    for (int pr = 0; pr < PT; ++pr)
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int Y = 2 * (i0 + pr) - 1 + r;
            const bool yok = Y >= 0 && Y < H;
            const unsigned ro = (unsigned)(Y < 0 ? 0 : (Y >= H ? H - 1 : Y)) * (unsigned)W;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int X = 2 * j - 1 + k;
                ok[pr][r][k] = yok && X >= 0 && X < W;
                off[pr][r][k] = ro + (unsigned)(X < 0 ? 0 : (X >= W ? W - 1 : X));
            }
        }
    const int Oe = (O + 1) & ~1;
    const float* gimg = gg + (size_t)b * (O - 1) * HWo;
    struct Ops { float gv[PT][3][3]; f4 k[CB][3]; };
    auto load = [&](Ops& T, int o0) {
        const int o = o0 + half;
        const bool ook = o < O - 1 || (o == O - 1 && gb != nullptr);
        const float* src = !ook ? gimg : (o < O - 1 ? gimg + (size_t)o * HWo : gb + (size_t)b * HWo);
#pragma unroll
        for (int pr = 0; pr < PT; ++pr)
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float v = src[off[pr][r][k]];
                    T.gv[pr][r][k] = (ook && ok[pr][r][k]) ? v : 0.f;
                }
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            const f4* rec = reinterpret_cast<const f4*>(wq + ((size_t)o * Cn + c0 + cb * 32 + id) * REC);
            T.k[cb][0] = rec[0]; T.k[cb][1] = rec[1]; T.k[cb][2] = rec[2];
        }
    };
    f16v acc[CB][PT];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int pr = 0; pr < PT; ++pr)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[cb][pr][q] = 0.f;
    Ops nxt;
    load(nxt, 0);
    for (int o0 = 0; o0 < Oe; o0 += 2) {
        const Ops cur = nxt;
        if (o0 + 2 < Oe) load(nxt, o0 + 2);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int tap = (2 - r) * 3 + (2 - k);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int pr = 0; pr < PT; ++pr) acc[cb][pr] = mfma(cur.k[cb][tap >> 2][tap & 3], cur.gv[pr][r][k], acc[cb][pr]);
            }
    }
    if (j >= w) return;
#pragma unroll
    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int c = c0 + cb * 32 + (q >> 2) * 8 + half * 4 + (q & 3);
            if (c >= C) continue;
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const int i = i0 + pr;
                if (i >= h) continue;
                const bool fed = 2 * i < H && 2 * j < W;       // (an input whose unpooled position lies beyond the narrowed output fed nothing: gradient 0)
                dx[((size_t)b * C + c) * hw + (size_t)i * w + j] = fed ? acc[cb][pr][q] : 0.f;
            }
        }
}

// ---- dL/dW ----------------------------------------------------------------------------------------------------------------------------
// D[row T = o * 9 + r * 3 + k][channel] += sum over pixels g[o][2i - 1 + r][2j - 1 + k] x[channel][i][j].  A tile = 8 consecutive pixels of an input row: lanes 0-31
// take pixels jb .. jb + 3, lanes 32-63 the next four, four matrix steps per (row block, channel block); a lane reads its row's four window values (8 consecutive
// floats, every other one a pixel's) and its channel's four pixels, the next tile's reads are issued before the current tile's matrix instructions.  blockIdx.y
// = the group of DW_TB row blocks; a wave takes a contiguous share of the tiles.
constexpr int DW_PX = 4, DW_TILE = 2 * DW_PX;

template <int NB>
__global__ __launch_bounds__(256, 2) void hk_bwd_w_kernel(const float* __restrict__ x, const float* __restrict__ gg, const float* __restrict__ gb,
                                                           float* __restrict__ part, const float* __restrict__ zero, int C, int c0, int h, int w, int H, int W,
                                                           int O, int tiles, int tiles_w, int hfed, int nwave) {
    __shared__ float red[DwSize<NB>::floats];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = blockIdx.x * 4 + wv, lane = threadIdx.x & 63;
    const int tg = blockIdx.y;
    // (a wave beyond nwave has no tiles; it still takes part in the workgroup's sum)
    const int t0 = wave < nwave ? (int)((long long)tiles * wave / nwave) : 0, t1 = wave < nwave ? (int)((long long)tiles * (wave + 1) / nwave) : 0;
    const int half = lane >> 5, id = lane & 31;
    const size_t HWo = (size_t)H * W, hw = (size_t)h * w;
    const int rows = 9 * O;
    const int ntb = (rows + 31) / 32 - tg * DW_TB;                 // row blocks of this group that hold rows at all (wave-uniform)
    int tr[DW_TB], tk[DW_TB];
    const float* tsrc[DW_TB];          // plane of image 0 (a padding row / no blur head: some valid plane, never used)
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
    const float* xsrc[NB];
    bool xvalid[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { const int ch = c0 + nb * 32 + id; xvalid[nb] = ch < C; xsrc[nb] = x + (size_t)(ch < C ? ch : 0) * hw; }
    struct Tile { float a[DW_TB][DW_PX]; float bq[NB][DW_PX]; };
    auto load = [&](Tile& T, int tw, int i, int b) {       // tile tw of input row i of image b
        const int jb = tw * DW_TILE + DW_PX * half;           // this lane's first pixel
#pragma unroll
        for (int tb = 0; tb < DW_TB; ++tb) {
            if (tb >= ntb) continue;
            const int Y = 2 * i - 1 + tr[tb], Xb = 2 * jb - 1 + tk[tb];
            const bool rowok = tvalid[tb] && Y >= 0 && Y < H;
            const float* p = tsrc[tb] + (size_t)b * tstep[tb] + (size_t)(rowok ? Y : 0) * W;
            if (!rowok || (Xb >= 0 && Xb + 2 * DW_PX - 1 < W)) {   // the common case: 2 DW_PX consecutive floats, every other one is a pixel's (a row outside: zeros)
                float q[2 * DW_PX];
                __builtin_memcpy(q, rowok ? p + Xb : zero, 8 * DW_PX);
#pragma unroll
                for (int s_ = 0; s_ < DW_PX; ++s_) T.a[tb][s_] = q[2 * s_];
            } else {                                             // the first / last tiles of a row: what lies outside reads a zero word
#pragma unroll
                for (int s_ = 0; s_ < DW_PX; ++s_) {
                    const int X = Xb + 2 * s_;
                    T.a[tb][s_] = *((X >= 0 && X < W) ? p + X : zero);
                }
            }
        }
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const float* p = xsrc[nb] + (size_t)b * C * hw + (size_t)i * w;
            if (!xvalid[nb] || (jb + DW_PX - 1 < w && 2 * (jb + DW_PX - 1) < W)) {
                __builtin_memcpy(T.bq[nb], xvalid[nb] ? p + jb : zero, 4 * DW_PX);
            } else {
#pragma unroll
                for (int s_ = 0; s_ < DW_PX; ++s_) {
                    const int j = jb + s_;
                    T.bq[nb][s_] = *((j < w && 2 * j < W) ? p + j : zero);      // (beyond the narrowed output: fed nothing)
                }
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
    for (int tb = 0; tb < DW_TB; ++tb)
#pragma unroll
        for (int s_ = 0; s_ < DW_PX; ++s_) nxt.a[tb][s_] = 0.f;
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
        for (int s_ = 0; s_ < DW_PX; ++s_)
#pragma unroll
            for (int tb = 0; tb < DW_TB; ++tb) {
                if (tb >= ntb) continue;
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[tb][nb] = mfma(cur.a[tb][s_], cur.bq[nb][s_], acc[tb][nb]);
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

__global__ void hk_zero_line_kernel(float* __restrict__ z) { z[threadIdx.x] = 0.f; }

// dW[o][c][ky][kx] = sum over the workgroups' blocks, in workgroup order (deterministic)
__global__ __launch_bounds__(256) void hk_bwd_w_reduce_kernel(const float* __restrict__ part, float* __restrict__ dwg, float* __restrict__ dwb, int C, int c0,
                                                               int NB, int O, int nwg) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nch = NB * 32;
    if (idx >= 9 * O * nch) return;
    const int t = idx / nch, cl = idx - t * nch, ch = c0 + cl;
    if (ch >= C) return;
    const int tbg = t >> 5, tg = tbg / DW_TB, tb = tbg - tg * DW_TB, i = t & 31, nb = cl >> 5, jc = cl & 31;
    const int q = (i >> 3) * 4 + (i & 3), l = ((i & 7) >> 2) * 32 + jc;
    const size_t stride = (size_t)DW_TB * NB * 16 * 64;
    const float* p = part + (size_t)tg * nwg * stride + ((size_t)(tb * NB + nb) * 16 + q) * 64 + l;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int g = 0;
    for (; g + 3 < nwg; g += 4) { s0 += p[(size_t)g * stride]; s1 += p[(size_t)(g + 1) * stride]; s2 += p[(size_t)(g + 2) * stride]; s3 += p[(size_t)(g + 3) * stride]; }
    for (; g < nwg; ++g) s0 += p[(size_t)g * stride];
    const float v = (s0 + s1) + (s2 + s3);
    const int o = t / 9, r = (t - o * 9) / 3, k = t - o * 9 - r * 3;
    const int tap = (2 - r) * 3 + (2 - k);
    if (o < O - 1) { if (dwg) dwg[((size_t)o * C + ch) * 9 + tap] = v; }
    else if (dwb) dwb[(size_t)ch * 9 + tap] = v;
}

size_t bwd_x_pack_bytes(int C, int O) { return round256((size_t)((O + 1) & ~1) * ((C + 31) & ~31) * REC * sizeof(float)); }

}  // namespace

void head_kxk_dw_reduce(const float* part, float* dwg, float* dwb, int C, int c0, int NB, int O, int nwg, hipStream_t st) {
    hipLaunchKernelGGL(hk_bwd_w_reduce_kernel, dim3((9 * O * NB * 32 + 255) / 256), dim3(256), 0, st, part, dwg, dwb, C, c0, NB, O, nwg);
}

// the forward's weight records ([C rounded up to even][32 or 64][12] floats)
size_t head_kxk_workspace(int C, int K) {
    const int On = (K * K + 31) & ~31;
    return round256((size_t)((C + 1) & ~1) * On * REC * sizeof(float));
}

int head_kxk_forward(const float* x, const float* wg, const float* wb, float* gout, float* bout, int B, int C, int h, int w, int H, int W, int K, void* ws,
                     hipStream_t st) {
    const int O = K * K, On = (O + 31) & ~31, Ce = (C + 1) & ~1;
    const int PT = K == 5 ? 2 : 1;
    const unsigned groups = groups_of((long long)B * ((h + PT - 1) / PT) * ((w + 31) / 32));
    if (!groups || (long long)Ce * On * REC >= (1ll << 31)) { set_error("cspn_guidance_head_kxk_f32: too many pixels or channels for one launch"); return CSPN_E_UNSUPPORTED; }
    float* wp = (float*)ws;
    hipLaunchKernelGGL(hk_pack_kernel, dim3((Ce * On * REC + 255) / 256), dim3(256), 0, st, wg, wb, wp, C, O, Ce, On, 1);
    if (K == 5) hipLaunchKernelGGL((hk_fwd_kernel<1, 2>), dim3(groups), dim3(256), 0, st, x, wp, gout, bout, C, h, w, H, W, B, O);
    else hipLaunchKernelGGL((hk_fwd_kernel<2, 1>), dim3(groups), dim3(256), 0, st, x, wp, gout, bout, C, h, w, H, W, B, O);
    return check_launch("hk_fwd_kernel");
}

// dL/dx's weight records + a line of zeros + the workgroups' partial blocks of dL/dW (64 channels at a time)
size_t head_kxk_backward_workspace(int B, int C, int h, int w, int K) {
    (void)B; (void)h; (void)w;
    const int O = K * K;
    return bwd_x_pack_bytes(C, O) + 256 + (size_t)row_groups(O) * DW_MAX_WG * DwSize<2>::floats * sizeof(float);
}

int head_kxk_backward(const float* x, const float* wg, const float* wb, const float* gg, const float* gb, float* dx, float* dwg, float* dwb, int B, int C,
                      int h, int w, int H, int W, int K, void* ws, hipStream_t st) {
    static const char* what = "cspn_guidance_head_kxk_backward_f32";
    const int O = K * K;
    if (dx) {
        constexpr int PT = 2;
        const int Oe = (O + 1) & ~1, Cn = (C + 31) & ~31;
        const unsigned groups = groups_of((long long)B * ((h + PT - 1) / PT) * ((w + 31) / 32));
        if (!groups || (long long)Oe * Cn * REC >= (1ll << 31)) { set_error("%s: too many pixels or channels for one launch", what); return CSPN_E_UNSUPPORTED; }
        float* wq = (float*)ws;
        hipLaunchKernelGGL(hk_pack_kernel, dim3((Oe * Cn * REC + 255) / 256), dim3(256), 0, st, wg, wb, wq, C, O, Cn, Oe, 0);
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time (two row blocks of the matrix core)
            if (C - c0 > 32) hipLaunchKernelGGL((hk_bwd_x_kernel<2, PT>), dim3(groups), dim3(256), 0, st, gg, gb, wq, dx, C, c0, Cn, h, w, H, W, B, O);
            else hipLaunchKernelGGL((hk_bwd_x_kernel<1, PT>), dim3(groups), dim3(256), 0, st, gg, gb, wq, dx, C, c0, Cn, h, w, H, W, B, O);
        }
        if (int e = check_launch("hk_bwd_x_kernel")) return e;
    }
    if (dwg || dwb) {
        float* zero = (float*)((char*)ws + bwd_x_pack_bytes(C, O));        // what a tile reads for positions outside the tensors
        float* part = zero + 64;
        hipLaunchKernelGGL(hk_zero_line_kernel, dim3(1), dim3(64), 0, st, zero);
        const DwGeo G(B, h, w, H, W, O, DW_TILE);
        if (!G.fits) { set_error("%s: too many pixels", what); return CSPN_E_UNSUPPORTED; }
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time (two column blocks of the matrix core)
            const int NB = C - c0 > 32 ? 2 : 1;
            if (NB == 2) hipLaunchKernelGGL(hk_bwd_w_kernel<2>, dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg, gb, part, zero, C, c0, h, w, H, W, O, G.tiles, G.tiles_w, G.hfed, G.nwave);
            else hipLaunchKernelGGL(hk_bwd_w_kernel<1>, dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg, gb, part, zero, C, c0, h, w, H, W, O, G.tiles, G.tiles_w, G.hfed, G.nwave);
            head_kxk_dw_reduce(part, dwg, dwb, C, c0, NB, O, G.nwg, st);
        }
        if (int e = check_launch("hk_bwd_w_kernel")) return e;
    }
    return 0;
}

}  // namespace cspn
