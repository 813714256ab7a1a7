// cspn_head_g16.hip -- the 3 x 3 model's guidance heads (8 guidance planes + the blur plane) on an fp16 / bf16 feature map, feeding the float32 rings:
// x and dL/dx are stored in the 16-bit type DT; the weights arrive as float32 masters and are rounded to DT once, in the per-call repack; guidance AND blur
// leave as float32, the matrix cores' unrounded accumulators, which is what Affinity_Propagate consumes; their gradients arrive as float32 (what the ring's
// backward returns) and are rounded to DT once as they enter the GEMMs (h16_round_kernel writes the rounded planes into the workspace).  Every product is of
// two DT values (exact in float32), the sums are float32.  dL/dx is the float32 accumulator rounded once at its single store; the weight gradients are the
// float32 accumulators.  No loss scaling happens in here: fp16 underflow of small gradients is the caller's GradScaler, as for any 16-bit convolution.
//   * forward: v_mfma_f32_16x16x32_{f16,bf16}, k = the channel (32 per instruction), rows = the 9 planes (9 of 16 rows used), columns = 16 pixels.  Lane l
//     (id = l % 16, qd = l / 16) holds A[row id][k = 8 qd + j] and B[k = 8 qd + j][column id] in element j = 0 .. 7 of a 4-register fragment, and
//     D[row 4 qd + q][column id] in register q.  An input pixel owns its 2 x 2 output block: 1 + 2 + 2 + 4 taps per parity, every output element written once.
//     x is plane-major, so a lane gathers its pixel's 8 channels with 8 loads -- of 4 bytes, which bring the right neighbour's (the taps at j + 1) along --
//     and packs them; the 36 accumulators of a block leave room for a second operand set: the loads of the next 32 channels are in flight while the matrix
//     cores work on this step's.
//   * dL/dx: the same instruction, one step per window column with k = (window row, plane) = 27 of 32, rows = 16 channels; the gather as the forward's.
//   * dL/dW: the GEMM of cspn_head_g16_common.h with O = 9 on the rounded planes (v_mfma_f32_32x32x16, k = the pixel; the partial blocks are added in wave
//     order through LDS, then in workgroup order: no atomics, deterministic).
// Addresses are clamped and values selected: nothing is read outside a tensor, whatever lies outside feeds a zero.  No kernel waits on another workgroup.
#include "cspn_head_g16_common.h"

namespace cspn {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
constexpr int O9 = 9;         // 8 guidance planes + the blur plane (plane 8)

template <bool BF>
__device__ __forceinline__ f4v mfma32(u4 a, u4 b, f4v c) {
    if constexpr (BF) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8, a), __builtin_bit_cast(b8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// One wave = PT input rows x 32 columns (two blocks of 16) x 9 planes.  wp: hk16_pack_kernel k_channel with 16 rows, [4 * Cs][9][16] fragments (Cs = steps of
// 32 channels).  WIDE (w >= 2): a 4-byte load fetches a pixel and its right neighbour, the operands of the taps at j and j + 1 in one (the lanes on a row's
// last pixel load the pair that ends there); else 2-byte loads (a one-column x has no right neighbours).
// fast: W % 4 == 0 and both outputs 16-byte aligned -- neighbouring lanes trade a row, so that a lane stores four pixels of one output row.
template <bool BF, int PT, bool WIDE>
__global__ __launch_bounds__(256, 2) void h16_fwd_kernel(const us* __restrict__ x, const u4* __restrict__ wp, float* __restrict__ gout, float* __restrict__ bout,
                                                          int C, int h, int w, int H, int W, int B, int fast) {
    const int wq = (w + 31) / 32, hp = (h + PT - 1) / PT;
    const int unit = wave_unit();
    const int seg = unit % wq;
    const int i0 = PT * ((unit / wq) % hp), b = unit / (wq * hp);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, qd = lane >> 4, id = lane & 15;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    // block n's pixel of this lane is column j = seg * 32 + n * 16 + id: ok0 / ok1 = that pixel / its right neighbour feeds the output
    bool ok0[PT + 1][2], ok1[PT + 1][2], last[2];
    unsigned off[PT + 1][2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int j = seg * 32 + n * 16 + id, jc = j < w ? j : w - 1;
        last[n] = WIDE && jc == w - 1;                    // the pair (w - 2, w - 1): the pixel in the high half, no right neighbour
#pragma unroll
        for (int r = 0; r <= PT; ++r) {
            const int i = i0 + r;
            const bool rok = i < h && 2 * i < H;
            ok0[r][n] = rok && j < w && 2 * j < W;
            ok1[r][n] = rok && j + 1 < w && 2 * (j + 1) < W;
            off[r][n] = (unsigned)(i < h ? i : h - 1) * (unsigned)w + (unsigned)(jc - (last[n] ? 1 : 0));
        }
    }
    const us* xb = x + (size_t)b * C * hw;
    const int Cs = (C + 31) >> 5;
    struct Raw { uint32_t v[PT + 1][2][8]; };             // as loaded: the lane's 8 channels of a pixel (low half) and its right neighbour (high half)
    struct Ops { u4 xv[PT + 1][4]; };                     // [.][2 n]: the pixel, [.][2 n + 1]: its right neighbour
    auto fetch = [&](Raw& R, int s) {
        const int cb = s * 32 + qd * 8;
#pragma unroll
        for (int r = 0; r <= PT; ++r)
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const int ch = cb + jj;
                    const us* p = xb + (size_t)(ch < C ? ch : C - 1) * hw + off[r][n];
                    uint32_t t;
                    if constexpr (WIDE) __builtin_memcpy(&t, p, 4);
                    else t = *p;
                    R.v[r][n][jj] = ch < C ? t : 0u;
                }
    };
    auto operands = [&](Ops& T, const Raw& R) {
#pragma unroll
        for (int r = 0; r <= PT; ++r)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                u4 lo, hi;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t a = R.v[r][n][2 * m], c = R.v[r][n][2 * m + 1];
                    lo[m] = (a & 0xffffu) | (c << 16);
                    hi[m] = (a >> 16) | (c & 0xffff0000u);
                }
                const u4 zero = {0u, 0u, 0u, 0u};
                T.xv[r][2 * n] = ok0[r][n] ? (last[n] ? hi : lo) : zero;
                T.xv[r][2 * n + 1] = ok1[r][n] ? hi : zero;
            }
    };
    f4v P00[2][PT], P01[2][PT], P10[2][PT], P11[2][PT];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int pr = 0; pr < PT; ++pr)
#pragma unroll
            for (int q = 0; q < 4; ++q) P00[n][pr][q] = P01[n][pr][q] = P10[n][pr][q] = P11[n][pr][q] = 0.f;
    Raw nxt;
    fetch(nxt, 0);
    for (int s = 0; s < Cs; ++s) {
        Ops cur;
        operands(cur, nxt);
        if (s + 1 < Cs) fetch(nxt, s + 1);         // in flight during this step's matrix work
        const u4* ws = wp + (size_t)(s * 4 + qd) * 9 * 16 + id;
        u4 k[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) k[t] = ws[t * 16];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const u4 x00 = cur.xv[pr][2 * n], x01 = cur.xv[pr][2 * n + 1], x10 = cur.xv[pr + 1][2 * n], x11 = cur.xv[pr + 1][2 * n + 1];
                P00[n][pr] = mfma32<BF>(k[4], x00, P00[n][pr]);       // W11
                P01[n][pr] = mfma32<BF>(k[3], x00, P01[n][pr]);       // W10
                P10[n][pr] = mfma32<BF>(k[1], x00, P10[n][pr]);       // W01
                P11[n][pr] = mfma32<BF>(k[0], x00, P11[n][pr]);       // W00
                P01[n][pr] = mfma32<BF>(k[5], x01, P01[n][pr]);       // W12
                P10[n][pr] = mfma32<BF>(k[7], x10, P10[n][pr]);       // W21
                P11[n][pr] = mfma32<BF>(k[2], x01, P11[n][pr]);       // W02
                P11[n][pr] = mfma32<BF>(k[6], x10, P11[n][pr]);       // W20
                P11[n][pr] = mfma32<BF>(k[8], x11, P11[n][pr]);       // W22
            }
    }
    // (no early return: the lanes of a pair trade rows below; a pair shares its qd, so it shares every plane index and every branch on one)
    const bool odd = id & 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int o = qd * 4 + q;
        if (o >= O9) continue;
        if (o == O9 - 1 && !bout) continue;
        float* dst = (o == O9 - 1 ? bout + (size_t)b * HWo : gout + ((size_t)b * (O9 - 1) + o) * HWo);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int j = seg * 32 + n * 16 + id;
            const bool mine = j < w && 2 * j < W;
            const int X0 = 2 * j;
            const bool two = X0 + 1 < W;
#pragma unroll
            for (int pr = 0; pr < PT; ++pr) {
                const int i = i0 + pr;
                if (i >= h) continue;
                const float r0[2] = {P00[n][pr][q], P01[n][pr][q]};    // row 2i:     X0, X0 + 1
                const float r1[2] = {P10[n][pr][q], P11[n][pr][q]};    // row 2i + 1
                if (fast) {
                    // the even lane of a pair takes row 2i of both (X0 .. X0 + 3, X0 a multiple of 4), the odd lane row 2i + 1; W % 4 == 0: a pair is inside
                    // the output together or not at all
                    const float g0 = __shfl_xor(odd ? r0[0] : r1[0], 1), g1 = __shfl_xor(odd ? r0[1] : r1[1], 1);
                    const int Y = 2 * i + (odd ? 1 : 0);
                    if (mine && Y < H) {
                        const float v[4] = {odd ? g0 : r0[0], odd ? g1 : r0[1], odd ? r1[0] : g0, odd ? r1[1] : g1};
                        __builtin_memcpy(dst + (size_t)Y * W + (X0 & ~3), v, 16);
                    }
                } else if (mine) {
                    if (2 * i < H) { float* d = dst + (size_t)(2 * i) * W + X0; d[0] = r0[0]; if (two) d[1] = r0[1]; }
                    if (2 * i + 1 < H) { float* d = dst + (size_t)(2 * i + 1) * W + X0; d[0] = r1[0]; if (two) d[1] = r1[1]; }
                }
            }
        }
    }
}

// ---- dL/dx ----------------------------------------------------------------------------------------------------------------------------
// dx[c][i][j] = sum over planes o, window rows r, window columns kx of g[o][2i - 1 + r][2j - 1 + kx] W[o][c][2 - r][2 - kx].  One matrix step per window
// column: k = 9 r + o (27 of 32 used), rows = 16 channels, columns = 16 pixels.  One wave = one input row x 32 columns (two blocks of 16) x 64 channels from
// c0 (four row blocks).  A lane gathers its 8 (r, o) at a pixel with 8 + 8 loads: 4 bytes at column 2j (the window's columns 1 and 2; WIDE, W >= 2 -- the
// lanes on an odd W's last column load the pair that ends there) and 2 bytes at column 2j - 1.  gg, gb: the gradients rounded to DT (gb null: no blur head).
// wq: h16_pack_dx_kernel's fragments [kx][block of 16 channels][lane].
template <bool BF>
__global__ __launch_bounds__(256) void h16_pack_dx_kernel(const float* __restrict__ wg, const float* __restrict__ wb, us* __restrict__ wp, int C, int ncb) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 3 * ncb * 64 * 8) return;
    const int jj = idx & 7, lane = (idx >> 3) & 63, u = idx >> 9;
    const int cblk = u % ncb, kx = u / ncb;
    const int k = (lane >> 4) * 8 + jj, r = k / 9, o = k - 9 * r, c = cblk * 16 + (lane & 15);
    float v = 0.f;
    if (k < 27 && c < C) {
        const int tap = (2 - r) * 3 + (2 - kx);
        if (o < O9 - 1) v = wg[((size_t)o * C + c) * 9 + tap];
        else if (wb) v = wb[(size_t)c * 9 + tap];
    }
    wp[idx] = narrow<BF>(v);
}

template <bool BF, bool WIDE>
__global__ __launch_bounds__(256, 2) void h16_bwd_x_kernel(const us* __restrict__ gg, const us* __restrict__ gb, const u4* __restrict__ wq, us* __restrict__ dx,
                                                            int C, int c0, int ncb, int h, int w, int H, int W, int B) {
    const int wq_ = (w + 31) / 32;
    const int unit = wave_unit();
    const int seg = unit % wq_;
    const int i = (unit / wq_) % h, b = unit / (wq_ * h);
    if (b >= B) return;
    const int lane = threadIdx.x & 63, qd = lane >> 4, id = lane & 15;
    const size_t hw = (size_t)h * w, HWo = (size_t)H * W;
    const us* src[8];              // the row of this lane's k = 8 qd + jj: plane o of image b at row 2i - 1 + r (clamped; what lies outside feeds a zero)
    bool rok[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int k = qd * 8 + jj, r = k / 9, o = k - 9 * r, Y = 2 * i - 1 + r;
        const bool blur = k < 27 && o == O9 - 1 && gb != nullptr;
        rok[jj] = k < 27 && (o < O9 - 1 || blur) && Y >= 0 && Y < H;
        const us* plane = blur ? gb + (size_t)b * HWo : gg + ((size_t)b * (O9 - 1) + (k < 27 && o < O9 - 1 ? o : 0)) * HWo;
        src[jj] = plane + (size_t)(Y < 0 ? 0 : (Y >= H ? H - 1 : Y)) * W;
    }
    const u4 zero = {0u, 0u, 0u, 0u};
    u4 Bf[2][3];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int j = seg * 32 + n * 16 + id, jc = j < w ? j : w - 1;
        const bool shift = WIDE && 2 * jc > W - 2;                       // the pair (W - 2, W - 1): column 2j in the high half, no column 2j + 1
        const int Xp = WIDE ? (shift ? W - 2 : 2 * jc) : 0;                // (not WIDE: W = 1)
        const int Xs = 2 * jc - 1 < 0 ? 0 : (2 * jc - 1 < W ? 2 * jc - 1 : W - 1);
        uint32_t P[8];
        us S[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
            uint32_t t;
            if constexpr (WIDE) __builtin_memcpy(&t, src[jj] + Xp, 4);
            else t = src[jj][Xp];
            const us sv = src[jj][Xs];
            P[jj] = rok[jj] ? t : 0u;
            S[jj] = (rok[jj] && j >= 1) ? sv : (us)0;
        }
        u4 lo, hi;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            lo[m] = (P[2 * m] & 0xffffu) | (P[2 * m + 1] << 16);
            hi[m] = (P[2 * m] >> 16) | (P[2 * m + 1] & 0xffff0000u);
        }
        Bf[n][0] = pack8(S);
        Bf[n][1] = shift ? hi : lo;
        Bf[n][2] = shift ? zero : hi;
    }
    f4v acc[4][2];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[cb][n][q] = 0.f;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const u4 a = wq[(size_t)(kx * ncb + (c0 >> 4) + cb) * 64 + lane];
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[cb][n] = mfma32<BF>(a, Bf[n][kx], acc[cb][n]);
        }
#pragma unroll
    for (int n = 0; n < 2; ++n) {
        const int j = seg * 32 + n * 16 + id;
        if (j >= w) continue;
        const bool fed = 2 * i < H && 2 * j < W;       // (an input whose unpooled position lies beyond the narrowed output fed nothing: gradient 0)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + cb * 16 + qd * 4 + q;
                if (c >= C) continue;
                dx[((size_t)b * C + c) * hw + (size_t)i * w + j] = fed ? narrow<BF>(acc[cb][n][q]) : (us)0;
            }
    }
}

constexpr int FWD_PT = 2;

// dL/dguidance [n8 floats] and dL/dblur [n1 floats, or null] as they enter the GEMMs: rounded once to DT, into one run of n8 + n1 DT.  Four elements per thread
// (16 bytes in, 8 out); the quad that straddles the two sources or the end goes element by element.
template <bool BF>
__global__ __launch_bounds__(256) void h16_round_kernel(const float* __restrict__ gg, const float* __restrict__ gb, us* __restrict__ out, size_t n8, size_t n1) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4, n = n8 + (gb ? n1 : 0);
    if (i0 >= n) return;
    const bool first = i0 + 3 < n8, second = i0 >= n8 && i0 + 3 < n;
    if (first || second) {
        float v[4];
        __builtin_memcpy(v, first ? gg + i0 : gb + (i0 - n8), 16);
        const uint32_t r[2] = {(uint32_t)narrow<BF>(v[0]) | ((uint32_t)narrow<BF>(v[1]) << 16), (uint32_t)narrow<BF>(v[2]) | ((uint32_t)narrow<BF>(v[3]) << 16)};
        __builtin_memcpy(out + i0, r, 8);
    } else {
        for (size_t i = i0; i < i0 + 4 && i < n; ++i) out[i] = narrow<BF>(i < n8 ? gg[i] : gb[i - n8]);
    }
}

size_t dx_pack_bytes(int C) { return round256((size_t)3 * ((C + 63) / 64 * 4) * 64 * 16); }       // dL/dx's weight fragments
size_t grads16_bytes(int B, int h, int w) { return round256((size_t)B * O9 * (2 * h) * (2 * w) * 2); }

template <bool BF>
int forward16(const us* x, const float* wg, const float* wb, float* gout, float* bout, int B, int C, int h, int w, int H, int W, void* ws, hipStream_t st) {
    const int Cs = (C + 31) >> 5;
    const unsigned groups = groups_of((long long)B * ((h + FWD_PT - 1) / FWD_PT) * ((w + 31) / 32));
    const long long halves = (long long)Cs * 4 * 9 * 16 * 8;
    if (!groups || halves >= (1ll << 31)) { set_error("cspn_guidance_head_g16: too many pixels or channels for one launch"); return CSPN_E_UNSUPPORTED; }
    hipLaunchKernelGGL(hk16_pack_kernel<BF>, dim3((unsigned)((halves + 255) / 256)), dim3(256), 0, st, wg, wb, (us*)ws, C, O9, Cs * 4, 16, 1);
    const int fast = (W % 4 == 0) && ((uintptr_t)gout % 16 == 0) && ((uintptr_t)bout % 16 == 0);
    if (w >= 2) hipLaunchKernelGGL((h16_fwd_kernel<BF, FWD_PT, true>), dim3(groups), dim3(256), 0, st, x, (const u4*)ws, gout, bout, C, h, w, H, W, B, fast);
    else hipLaunchKernelGGL((h16_fwd_kernel<BF, FWD_PT, false>), dim3(groups), dim3(256), 0, st, x, (const u4*)ws, gout, bout, C, h, w, H, W, B, fast);
    return check_launch("h16_fwd_kernel");
}

template <bool BF>
int backward16(const us* x, const float* wg, const float* wb, const float* gg, const float* gb, us* dx, float* dwg, float* dwb, int B, int C, int h, int w, int H,
               int W, void* ws, hipStream_t st) {
    static const char* what = "cspn_guidance_head_backward_g16";
    // the gradients as they enter the GEMMs: rounded once to DT, [B, 8, H, W] then [B, 1, H, W]
    const size_t n = (size_t)B * H * W;
    if ((O9 - 1) * n >= ((size_t)1 << 39)) { set_error("%s: too many pixels for one launch", what); return CSPN_E_UNSUPPORTED; }
    us* gg16 = (us*)((char*)ws + dx_pack_bytes(C));
    us* gb16 = gb ? gg16 + (O9 - 1) * n : nullptr;
    hipLaunchKernelGGL(h16_round_kernel<BF>, dim3((unsigned)((O9 * n + 1023) / 1024)), dim3(256), 0, st, gg, gb, gg16, (O9 - 1) * n, n);
    if (dx) {
        const int ncb = (C + 63) / 64 * 4;
        const unsigned groups = groups_of((long long)B * h * ((w + 31) / 32));
        const long long halves = (long long)3 * ncb * 64 * 8;
        if (!groups || halves >= (1ll << 31)) { set_error("%s: too many pixels or channels for one launch", what); return CSPN_E_UNSUPPORTED; }
        hipLaunchKernelGGL(h16_pack_dx_kernel<BF>, dim3((unsigned)((halves + 255) / 256)), dim3(256), 0, st, wg, wb, (us*)ws, C, ncb);
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time
            if (W >= 2) hipLaunchKernelGGL((h16_bwd_x_kernel<BF, true>), dim3(groups), dim3(256), 0, st, gg16, gb16, (const u4*)ws, dx, C, c0, ncb, h, w, H, W, B);
            else hipLaunchKernelGGL((h16_bwd_x_kernel<BF, false>), dim3(groups), dim3(256), 0, st, gg16, gb16, (const u4*)ws, dx, C, c0, ncb, h, w, H, W, B);
        }
        if (int e = check_launch("h16_bwd_x_kernel")) return e;
    }
    if (dwg || dwb) {
        float* part = (float*)((char*)ws + dx_pack_bytes(C) + grads16_bytes(B, h, w));
        const DwGeo G(B, h, w, H, W, O9, DW_TILE);
        if (!G.fits) { set_error("%s: too many pixels", what); return CSPN_E_UNSUPPORTED; }
        for (int c0 = 0; c0 < C; c0 += 64) {                     // 64 channels at a time (two column blocks of the matrix core)
            const int NB = C - c0 > 32 ? 2 : 1;
            if (NB == 2) hipLaunchKernelGGL((hk16_bwd_w_kernel<BF, 2>), dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg16, gb16, part, C, c0, h, w, H, W, O9, G.tiles, G.tiles_w, G.hfed, G.nwave);
            else hipLaunchKernelGGL((hk16_bwd_w_kernel<BF, 1>), dim3(G.nwg, G.ng), dim3(256), 0, st, x, gg16, gb16, part, C, c0, h, w, H, W, O9, G.tiles, G.tiles_w, G.hfed, G.nwave);
            head_kxk_dw_reduce(part, dwg, dwb, C, c0, NB, O9, G.nwg, st);
        }
        if (int e = check_launch("hk16_bwd_w_kernel")) return e;
    }
    return 0;
}

}  // namespace

// the forward's weight fragments ([C rounded up to 32 / 8][9][16] x 16 bytes)
size_t head_g16_workspace(int C) { return round256((size_t)((C + 31) >> 5) * 4 * 9 * 16 * 16); }

int head_g16_forward(const void* x, int dtype, const float* wg, const float* wb, float* gout, float* bout, int B, int C, int h, int w, int H, int W, void* ws,
                     hipStream_t st) {
    return dtype == CSPN_DTYPE_F16 ? forward16<false>((const us*)x, wg, wb, gout, bout, B, C, h, w, H, W, ws, st)
                                   : forward16<true>((const us*)x, wg, wb, gout, bout, B, C, h, w, H, W, ws, st);
}

// dL/dx's weight fragments + both gradients rounded to DT + the workgroups' partial blocks of dL/dW (64 channels at a time)
size_t head_g16_backward_workspace(int B, int C, int h, int w) {
    return dx_pack_bytes(C) + grads16_bytes(B, h, w) + (size_t)row_groups(O9) * DW_MAX_WG * DwSize<2>::floats * sizeof(float);
}

int head_g16_backward(const void* x, int dtype, const float* wg, const float* wb, const float* gg, const float* gb, void* dx, float* dwg, float* dwb, int B, int C,
                      int h, int w, int H, int W, void* ws, hipStream_t st) {
    return dtype == CSPN_DTYPE_F16 ? backward16<false>((const us*)x, wg, wb, gg, gb, (us*)dx, dwg, dwb, B, C, h, w, H, W, ws, st)
                                   : backward16<true>((const us*)x, wg, wb, gg, gb, (us*)dx, dwg, dwb, B, C, h, w, H, W, ws, st);
}

}  // namespace cspn
