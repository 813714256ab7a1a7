// cspn2d_scan.hip -- line-scan propagation, the three-way linear recurrence of SPN (the "line scan, three-way" contract),
// float32, forward and backward.  Written from the published description of the method, not from a source.
//   x     [B][C][H][W]
//   dirs  a non-empty subset of {0 left->right, 1 right->left, 2 top->bottom, 3 bottom->top} as a 4-bit mask; D = its size, the directions are
//         numbered d = 0 .. D-1 in ascending order of their code
//   gates [B][D Cg 3][H][W]    channel (d Cg + j) 3 + k, used as given; Cg divides C, channel c uses group j = c / (C / Cg)
//   lam   [B][D C][H][W] or NULL        out [B][D C][H][W], channel d C + c
// Directions 0 / 1: a line is a column, t the column index (ascending for 0, descending for 1), i the row.  Directions 2 / 3: a line is a
// row, t the row index, i the column.  L the line length, t- the line visited just before t, k in {0,1,2} the connection to h(i + k - 1, t-):
//   g^_k(i,t) = g_k(i,t)  if t is not the first line and 0 <= i + k - 1 < L,   else 0
//   b(i,t)    = lam(i,t)  if lam is given,   else 1 - sum_k g^_k(i,t)
//   h(i,t)    = b(i,t) x(i,t) + sum_k g^_k(i,t) h(i + k - 1, t-)                       (first line: h = b x)
//   A(i,t)    = grad_out(i,t) + sum_k g^_k(i - (k-1), t+) A(i - (k-1), t+)             (t+: the line visited after t; last line: A = grad_out)
//   grad_x    = sum_d b A        grad_lam = A x (lam given)
//   grad_g_k  = sum_{c in group} A (h(i + k - 1, t-) - x(i,t)) without lam,  sum_{c in group} A h(i + k - 1, t-) with lam; exactly 0 wherever
//               g^_k is the dropped 0
// Nothing is guarded: gates with sum |g| > 1 diverge as the formulas do.
//
// One launch runs every (image, direction, channel): a workgroup of 256 threads owns the lines of one of them and walks the whole scan.  Pixel
// i = k 256 + thread of the line (k < 8: lines of up to 2048 pixels) stays with its thread for all steps, so the previous line (forward: h;
// backward: the three products g^_k A) lives in registers.  i - 1 and i + 1 are the neighbouring lanes: a wave shift (DPP) inside a wave; the
// first and the last lane of every wave leave their values in a double-buffered LDS slot, which is the one barrier of a step.
// Memory goes through LDS in blocks of tb lines (tb a power of two <= 16, the largest that fits): rows x tb columns for the horizontal
// directions, read and written back along the rows (tb consecutive floats a row) into a tile padded to an odd pitch, so that the step's
// reads down a column meet no bank conflict; tb rows for the vertical ones.  No tensor is transposed in memory.  Results replace their inputs
// in the tile (out over x; grad_x over grad_out, grad_gates over the gates, grad_lam over lam).  The global loads and stores of a block are
// outside the barriered loop: no step waits for memory.
// The backward reads x, gates, lam, out and grad_out.  grad_x of direction d > 0 and grad_gates of a group's channels r > 0 go to the workspace;
// one reduction launch adds them in ascending order onto what d = 0 / r = 0 wrote.  No atomics: every result is run-to-run bitwise.
#include "cspn_common.h"

namespace cspn {

namespace {

constexpr int SNT = 256, SNW = SNT / 64, SPPT = SCAN_MAX_LINE / SNT, SEDGE = SPPT * SNW;
// floats of one staged array: the forward stages 5 (x, 3 gates, lam), the backward 7 (grad_out, 3 gates, x, lam, out); with the edge slots
// (2 buffers x 2 sides x SEDGE floats) each is at most 64 KiB
constexpr int FCAP = 3072, BCAP = 2304;
static_assert(FCAP >= SCAN_MAX_LINE && BCAP >= SCAN_MAX_LINE, "a block of one line must fit");
static_assert((5 * FCAP + 4 * SEDGE) * 4 <= 65536 && (7 * BCAP + 4 * SEDGE) * 4 <= 65536, "LDS of a workgroup");

// lines of a staged block: the largest power of two <= 16 whose tile fits cap floats (horizontal tiles of more than one column carry a
// padding column)
int scan_tb(int L, bool horiz, int cap) {
    int tb = 16;
    while (tb > 1 && (size_t)L * (horiz ? tb + 1 : tb) > (size_t)cap) tb >>= 1;
    return tb;
}

// the value of lane - 1 (lane 0: 0) and of lane + 1 (lane 63: 0) of the wave; every lane of the wave must be active
__device__ __forceinline__ float lane_below(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_above(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

// the code of the slot-th direction of the mask
__device__ __forceinline__ int scan_dir(int dirs, int slot) {
    int d = 0;
    for (;; ++d)
        if ((dirs >> d) & 1)
            if (slot-- == 0) break;
    return d;
}

// a block of a plane [H][W] <-> its LDS tile.  HORIZ: rows 0 .. L-1, columns t0 .. t0 + n - 1, tile[r pitch + c], tb = 1 << tbs columns wide;
// else rows t0 .. t0 + n - 1, columns 0 .. L-1 (L = W), tile[l pitch + i].  Lines outside 0 .. T-1 are skipped.
template <bool HORIZ>
__device__ __forceinline__ void tile_load(float* __restrict__ tile, const float* __restrict__ plane, int L, int T, int W, int t0, int n, int tbs, int pitch) {
    if (HORIZ) {
        for (int e = threadIdx.x; e < (L << tbs); e += SNT) {
            const int r = e >> tbs, c = e & ((1 << tbs) - 1);
            if (c < n && (unsigned)(t0 + c) < (unsigned)T) tile[r * pitch + c] = plane[(size_t)r * W + t0 + c];
        }
    } else {
        for (int l = 0; l < n; ++l) {
            if ((unsigned)(t0 + l) >= (unsigned)T) continue;
            for (int i = threadIdx.x; i < L; i += SNT) tile[l * pitch + i] = plane[(size_t)(t0 + l) * W + i];
        }
    }
}

template <bool HORIZ>
__device__ __forceinline__ void tile_store(float* __restrict__ plane, const float* __restrict__ tile, int L, int W, int t0, int n, int tbs, int pitch) {
    if (HORIZ) {
        for (int e = threadIdx.x; e < (L << tbs); e += SNT) {
            const int r = e >> tbs, c = e & ((1 << tbs) - 1);
            if (c < n) plane[(size_t)r * W + t0 + c] = tile[r * pitch + c];
        }
    } else {
        for (int l = 0; l < n; ++l)
            for (int i = threadIdx.x; i < L; i += SNT) plane[(size_t)(t0 + l) * W + i] = tile[l * pitch + i];
    }
}

// the scan of one (image, direction, channel): L pixels a line, T lines, rev: descending t
template <bool HORIZ>
__device__ __forceinline__ void scan_forward_lines(float* __restrict__ lds, const float* __restrict__ xp, const float* __restrict__ gp,
                                                   const float* __restrict__ lp, float* __restrict__ op, int L, int T, int W, size_t HW, bool rev, int tbs) {
    float* sx = lds;                 // x, then h
    float* sg = lds + FCAP;          // three arrays
    float* sl = lds + 4 * FCAP;
    float* edge = lds + 5 * FCAP;    // [2 buffers][below | above][SEDGE]
    const int tb = 1 << tbs, pitch = HORIZ ? tb + (tb > 1 ? 1 : 0) : L;
    const int npx = (L + SNT - 1) / SNT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float h[SPPT];
#pragma unroll
    for (int k = 0; k < SPPT; ++k) h[k] = 0.f;
    for (int s0 = 0; s0 < T; s0 += tb) {
        const int n = min(tb, T - s0), t0 = rev ? T - s0 - n : s0;
        __syncthreads();   // the previous block is stored (and, the first time, the edge slots are cleared)
        tile_load<HORIZ>(sx, xp, L, T, W, t0, n, tbs, pitch);
#pragma unroll
        for (int k = 0; k < 3; ++k) tile_load<HORIZ>(sg + k * FCAP, gp + k * HW, L, T, W, t0, n, tbs, pitch);
        if (lp) tile_load<HORIZ>(sl, lp, L, T, W, t0, n, tbs, pitch);
        __syncthreads();
        for (int q = 0; q < n; ++q) {
            const int s = s0 + q, l = rev ? n - 1 - q : q;
            const float* rb = edge + ((s + 1) & 1) * 2 * SEDGE;   // what step s - 1 left
            float* wb = edge + (s & 1) * 2 * SEDGE;
#pragma unroll
            for (int k = 0; k < SPPT; ++k) {
                if (k >= npx) break;
                const int i = k * SNT + threadIdx.x, e = k * SNW + wave;
                const float hc = h[k];
                float hm = lane_below(hc), hp = lane_above(hc);
                if (lane == 0) hm = e > 0 ? rb[SEDGE + e - 1] : 0.f;
                if (lane == 63) hp = e + 1 < SEDGE ? rb[e + 1] : 0.f;
                float v = 0.f;
                if (i < L) {
                    const int a = HORIZ ? i * pitch + l : l * pitch + i;
                    const float g0 = (s > 0 && i > 0) ? sg[a] : 0.f, g1 = s > 0 ? sg[FCAP + a] : 0.f, g2 = (s > 0 && i + 1 < L) ? sg[2 * FCAP + a] : 0.f;
                    const float b = lp ? sl[a] : 1.f - ((g0 + g1) + g2);
                    v = fmaf(g2, hp, fmaf(g1, hc, fmaf(g0, hm, b * sx[a])));
                    sx[a] = v;
                }
                h[k] = v;
                if (lane == 0) wb[e] = v;             // read by the lane below it: the last lane of the wave before
                if (lane == 63) wb[SEDGE + e] = v;    // read by the first lane of the wave behind
            }
            __syncthreads();
        }
        tile_store<HORIZ>(op, sx, L, W, t0, n, tbs, pitch);
    }
}

__global__ __launch_bounds__(SNT) void scan_forward_kernel(const float* __restrict__ x, const float* __restrict__ gates, const float* __restrict__ lam,
                                                           float* __restrict__ out, int C, int Cg, int D, int dirs, int H, int W, int tbs_v, int tbs_h) {
    __shared__ float lds[5 * FCAP + 4 * SEDGE];
    unsigned blk = blockIdx.x;
    const int c = blk % C;
    blk /= C;
    const int slot = blk % D, b = blk / D, dir = scan_dir(dirs, slot);
    const size_t HW = (size_t)H * W, oc = ((size_t)b * D + slot) * C + c;
    const float* xp = x + ((size_t)b * C + c) * HW;
    const float* gp = gates + (((size_t)b * D + slot) * Cg + c / (C / Cg)) * 3 * HW;
    const float* lp = lam ? lam + oc * HW : nullptr;
    if (threadIdx.x < 4 * SEDGE) lds[5 * FCAP + threadIdx.x] = 0.f;
    if (dir < 2) scan_forward_lines<true>(lds, xp, gp, lp, out + oc * HW, H, W, W, HW, dir == 1, tbs_h);
    else scan_forward_lines<false>(lds, xp, gp, lp, out + oc * HW, W, H, W, HW, dir == 3, tbs_v);
}

// the adjoint scan of one (image, direction, channel), last line first.  hp: out of the forward; gxp, ggp (three planes), glp: where this
// workgroup's gradients go, each may be NULL
template <bool HORIZ>
__device__ __forceinline__ void scan_backward_lines(float* __restrict__ lds, const float* __restrict__ xp, const float* __restrict__ gp,
                                                    const float* __restrict__ lp, const float* __restrict__ hp, const float* __restrict__ gop,
                                                    float* __restrict__ gxp, float* __restrict__ ggp, float* __restrict__ glp, int L, int T, int W, size_t HW,
                                                    bool rev, int tbs) {
    float* sa = lds;                 // grad_out, then b A
    float* sg = lds + BCAP;          // the gates, then their gradients
    float* sx = lds + 4 * BCAP;
    float* sl = lds + 5 * BCAP;      // lam, then A x
    float* sh = lds + 6 * BCAP;      // h of the line visited before: the block of out shifted by one line
    float* edge = lds + 7 * BCAP;
    const int tb = 1 << tbs, pitch = HORIZ ? tb + (tb > 1 ? 1 : 0) : L;
    const int npx = (L + SNT - 1) / SNT, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float p0[SPPT], p1[SPPT], p2[SPPT];   // g^_k A of the line visited after this one
#pragma unroll
    for (int k = 0; k < SPPT; ++k) p0[k] = p1[k] = p2[k] = 0.f;
    for (int s0 = (T - 1) / tb * tb; s0 >= 0; s0 -= tb) {
        const int n = min(tb, T - s0), t0 = rev ? T - s0 - n : s0;
        __syncthreads();
        tile_load<HORIZ>(sa, gop, L, T, W, t0, n, tbs, pitch);
#pragma unroll
        for (int k = 0; k < 3; ++k) tile_load<HORIZ>(sg + k * BCAP, gp + k * HW, L, T, W, t0, n, tbs, pitch);
        tile_load<HORIZ>(sx, xp, L, T, W, t0, n, tbs, pitch);
        if (lp) tile_load<HORIZ>(sl, lp, L, T, W, t0, n, tbs, pitch);
        tile_load<HORIZ>(sh, hp, L, T, W, t0 + (rev ? 1 : -1), n, tbs, pitch);   // (the line before the first does not exist and is not read)
        __syncthreads();
        for (int q = n - 1; q >= 0; --q) {
            const int s = s0 + q, l = rev ? n - 1 - q : q;
            const float* rb = edge + ((s + 1) & 1) * 2 * SEDGE;   // what step s + 1 left
            float* wb = edge + (s & 1) * 2 * SEDGE;
#pragma unroll
            for (int k = 0; k < SPPT; ++k) {
                if (k >= npx) break;
                const int i = k * SNT + threadIdx.x, e = k * SNW + wave;
                float a0 = lane_above(p0[k]), a2 = lane_below(p2[k]);   // g^_0 A of pixel i + 1, g^_2 A of pixel i - 1
                if (lane == 63) a0 = e + 1 < SEDGE ? rb[e + 1] : 0.f;
                if (lane == 0) a2 = e > 0 ? rb[SEDGE + e - 1] : 0.f;
                float n0 = 0.f, n1 = 0.f, n2 = 0.f;
                if (i < L) {
                    const int a = HORIZ ? i * pitch + l : l * pitch + i, di = HORIZ ? pitch : 1;
                    const float A = ((sa[a] + a0) + p1[k]) + a2;
                    const bool k0 = s > 0 && i > 0, k1 = s > 0, k2 = s > 0 && i + 1 < L;
                    const float g0 = k0 ? sg[a] : 0.f, g1 = k1 ? sg[BCAP + a] : 0.f, g2 = k2 ? sg[2 * BCAP + a] : 0.f;
                    const float xv = sx[a], sub = lp ? 0.f : xv;
                    const float b = lp ? sl[a] : 1.f - ((g0 + g1) + g2);
                    sa[a] = b * A;
                    if (lp) sl[a] = A * xv;
                    sg[a] = k0 ? A * (sh[a - di] - sub) : 0.f;
                    sg[BCAP + a] = k1 ? A * (sh[a] - sub) : 0.f;
                    sg[2 * BCAP + a] = k2 ? A * (sh[a + di] - sub) : 0.f;
                    n0 = g0 * A;
                    n1 = g1 * A;
                    n2 = g2 * A;
                }
                p0[k] = n0;
                p1[k] = n1;
                p2[k] = n2;
                if (lane == 0) wb[e] = n0;             // read by the lane below it
                if (lane == 63) wb[SEDGE + e] = n2;    // read by the lane above it
            }
            __syncthreads();
        }
        if (gxp) tile_store<HORIZ>(gxp, sa, L, W, t0, n, tbs, pitch);
        if (ggp) {
#pragma unroll
            for (int k = 0; k < 3; ++k) tile_store<HORIZ>(ggp + k * HW, sg + k * BCAP, L, W, t0, n, tbs, pitch);
        }
        if (glp) tile_store<HORIZ>(glp, sl, L, W, t0, n, tbs, pitch);
    }
}

// gx / gg / gl: the gradient tensors (each may be NULL).  Direction slot 0 writes grad_x itself, slot d > 0 the part d - 1 of xpart
// ([D-1][B][C][H][W]); the first channel of a group writes grad_gates itself, its channel r > 0 the part r - 1 of gpart ([C/Cg - 1][B][D Cg 3][H][W])
__global__ __launch_bounds__(SNT) void scan_backward_kernel(const float* __restrict__ x, const float* __restrict__ gates, const float* __restrict__ lam,
                                                            const float* __restrict__ out, const float* __restrict__ gout, float* __restrict__ gx,
                                                            float* __restrict__ gg, float* __restrict__ gl, float* __restrict__ xpart,
                                                            float* __restrict__ gpart, int B, int C, int Cg, int D, int dirs, int H, int W, int tbs_v,
                                                            int tbs_h) {
    __shared__ float lds[7 * BCAP + 4 * SEDGE];
    unsigned blk = blockIdx.x;
    const int c = blk % C;
    blk /= C;
    const int slot = blk % D, b = blk / D, dir = scan_dir(dirs, slot), cpg = C / Cg, j = c / cpg, r = c - j * cpg;
    const size_t HW = (size_t)H * W, oc = ((size_t)b * D + slot) * C + c, xc = (size_t)b * C + c, gc = (((size_t)b * D + slot) * Cg + j) * 3;
    float* gxp = gx ? (slot == 0 ? gx + xc * HW : xpart + ((size_t)(slot - 1) * B * C + xc) * HW) : nullptr;
    float* ggp = gg ? (r == 0 ? gg + gc * HW : gpart + ((size_t)(r - 1) * B * D * Cg * 3 + gc) * HW) : nullptr;
    float* glp = gl ? gl + oc * HW : nullptr;
    const float* lp = lam ? lam + oc * HW : nullptr;
    if (threadIdx.x < 4 * SEDGE) lds[7 * BCAP + threadIdx.x] = 0.f;
    if (dir < 2)
        scan_backward_lines<true>(lds, x + xc * HW, gates + gc * HW, lp, out + oc * HW, gout + oc * HW, gxp, ggp, glp, H, W, W, HW, dir == 1, tbs_h);
    else
        scan_backward_lines<false>(lds, x + xc * HW, gates + gc * HW, lp, out + oc * HW, gout + oc * HW, gxp, ggp, glp, W, H, W, HW, dir == 3, tbs_v);
}

// dst[e] += part[0][e] + part[1][e] + ..., added in ascending order, for the nx elements of grad_x (px parts) and the ng of grad_gates (pg parts)
__global__ __launch_bounds__(SNT) void scan_reduce_kernel(float* __restrict__ gx, const float* __restrict__ xpart, size_t nx, int px, float* __restrict__ gg,
                                                          const float* __restrict__ gpart, size_t ng, int pg) {
    const size_t stride = (size_t)gridDim.x * SNT;
    for (size_t e = (size_t)blockIdx.x * SNT + threadIdx.x; e < nx + ng; e += stride) {
        const bool first = e < nx;
        const size_t at = first ? e : e - nx, len = first ? nx : ng;
        float* dst = first ? gx : gg;
        const float* part = first ? xpart : gpart;
        const int parts = first ? px : pg;
        float v = dst[at];
        for (int p = 0; p < parts; ++p) v += part[(size_t)p * len + at];
        dst[at] = v;
    }
}

int log2i(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return s;
}

}  // namespace

int scan_forward(const float* x, const float* gates, const float* lam, float* out, int B, int C, int Cg, int H, int W, int dirs, hipStream_t st) {
    const int D = __builtin_popcount(dirs);
    const unsigned blocks = (unsigned)((size_t)B * D * C);
    hipLaunchKernelGGL(scan_forward_kernel, dim3(blocks), dim3(SNT), 0, st, x, gates, lam, out, C, Cg, D, dirs, H, W, log2i(scan_tb(W, false, FCAP)),
                       log2i(scan_tb(H, true, FCAP)));
    return check_launch("scan_forward_kernel");
}

int scan_backward(const float* x, const float* gates, const float* lam, const float* out, const float* gout, float* gx, float* gg, float* gl, int B, int C,
                  int Cg, int H, int W, int dirs, void* ws, hipStream_t st) {
    const int D = __builtin_popcount(dirs);
    const ScanBackwardWs lay(B, C, Cg, H, W, D);
    float* xpart = (float*)((char*)ws + lay.xpart);
    float* gpart = (float*)((char*)ws + lay.gpart);
    const unsigned blocks = (unsigned)((size_t)B * D * C);
    hipLaunchKernelGGL(scan_backward_kernel, dim3(blocks), dim3(SNT), 0, st, x, gates, lam, out, gout, gx, gg, gl, xpart, gpart, B, C, Cg, D, dirs, H, W,
                       log2i(scan_tb(W, false, BCAP)), log2i(scan_tb(H, true, BCAP)));
    if (int e = check_launch("scan_backward_kernel")) return e;
    const size_t HW = (size_t)H * W, nx = (gx && D > 1) ? (size_t)B * C * HW : 0, ng = (gg && C / Cg > 1) ? (size_t)B * D * Cg * 3 * HW : 0;
    if (nx + ng == 0) return 0;
    const size_t want = (nx + ng + SNT - 1) / SNT;
    const unsigned rblocks = (unsigned)(want < (size_t)(8 * num_cus()) ? want : (size_t)(8 * num_cus()));
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(rblocks), dim3(SNT), 0, st, gx, xpart, nx, D - 1, gg, gpart, ng, C / Cg - 1);
    return check_launch("scan_reduce_kernel");
}

}  // namespace cspn
