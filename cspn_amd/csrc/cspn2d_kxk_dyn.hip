// cspn2d_kxk_dyn.hip -- K x K propagation with per-step attention (the "dynamic, centre-sited" contract), K = 3, 5 or 7,
// float32, forward and backward.  The kernels are siblings of those in cspn2d_kxk_impl.h (whose bodies stay the text they are) and share
// their helpers: the 64 x 16 tile of 256 threads, tile_of, stage, Quad, load4 / store4, chan, the VEC / guarded-scalar pair.
//   guid [N][KK][H][W]         raw, any sign, read at p; channel order and off_k = (R - t, R - l) of the K x K engine
//   att  [N][n (R+1)][H][W]    used as given; channel s (R+1) + r: r = 0 the pixel's own term (in the divisor only), r >= 1 ring r of step s,
//                              ring(k) = max(|dy|, |dx|)
//   values [N][C][H][W] on the shared guid / att; sparse [N][H][W] or NULL, pinned where > 0 before every step (the result is not pinned)
//   w^_k = att_ring(k) g_k    D = att_0 + sum_k |w^_k|    c = (att_0 + sum_k (|w^_k| - w^_k)) / D  ( = 1 - sum_k w^_k / D )
//   H_{s+1}(p) = c H~_s(p) + (sum_k w^_k H~_s(p + off_k)) / D          zero outside the image; the sum is scaled once, after it
// No modulated or normalised gate and no gradient of one is ever stored: the forward step forms w^ in the gate registers; the adjoint step holds
// the raw gates of shifted pixels and reads att_r A / D from one staged tile per ring; the gradient pass keeps g and its KK sums in registers over
// all steps and channels and writes every element of dL/dguid and dL/datt once.  No atomics: every result is run-to-run bitwise.
// D = 0 gives the non-finite pattern of the statement; nothing is guarded.
#include "cspn2d_kxk_impl.h"

namespace cspn {

namespace {

// ring(k) - 1 of the gate channel of the pair (t, l)
template <int K>
__host__ __device__ constexpr int ring0(int t, int l) {
    const int a = t > K / 2 ? t - K / 2 : K / 2 - t, b = l > K / 2 ? l - K / 2 : K / 2 - l;
    return (a > b ? a : b) - 1;
}

// one forward step for all C channels: dst = pin(step(src)), or step(src) where sparse is NULL (the last step; a call without a mask).
// att: the step's R + 1 planes of image 0, astride floats from an image's planes to the next one's.
// VEC: W % 4 == 0 and guid, att, dst and sparse 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_dyn_forward_step(const float* __restrict__ guid, const float* __restrict__ att, size_t astride,
                                                           const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ sparse, int C,
                                                           int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, SW = TW + 2 * R;
    __shared__ float lds[(TH + 2 * R) * SW];
    // 1 / D, c and the measured depth of the thread's four pixels wait here while the stencil runs, as the ABS instance parks 1 / S
    __shared__ float4 park[3 * NT];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    Quad<float> g[KK];
    const float* gp = guid + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) load_quad<VEC, float>(g[k], gp + (size_t)k * HW, row_in, T.x0, W, guid);
    {
        const float* ap = att + (size_t)T.n * astride + pix;
        float a[R + 1][4], Dn[4], Cn[4];
#pragma unroll
        for (int r = 0; r <= R; ++r) load4<VEC>(a[r], ap + (size_t)r * HW, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) Dn[j] = Cn[j] = a[0][j];
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l), r = ring0<K>(t, l) + 1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float w = a[r][j] * g[k].v[j];
                    g[k].v[j] = w;
                    Dn[j] += fabsf(w);
                    Cn[j] += fabsf(w) - w;
                }
            }
        float rd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rd[j] = 1.f / Dn[j];
        park[threadIdx.x] = make_float4(rd[0], rd[1], rd[2], rd[3]);   // read back by this thread alone
        park[NT + threadIdx.x] = make_float4(Cn[0] * rd[0], Cn[1] * rd[1], Cn[2] * rd[2], Cn[3] * rd[3]);
        if (sparse) {
            float s[4];
            load4<VEC>(s, sparse + (size_t)T.n * HW + pix, row_in, T.x0, W);
            park[2 * NT + threadIdx.x] = make_float4(s[0], s[1], s[2], s[3]);
        }
    }
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)T.n * C + c) * HW;
        __syncthreads();   // the previous channel's reads of lds are done
        stage<R>(lds, src + plane, T.y0, T.xt0, H, W);
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            float row[4 + 2 * R];   // row y + R - t, columns x0 - R .. x0 + 3 + R
#pragma unroll
            for (int i = 0; i < 4 + 2 * R; ++i) row[i] = lds[(T.ly + 2 * R - t) * SW + 4 * T.lq + i];
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(g[k].get(j), row[j + 2 * R - l], acc[j]);
            }
        }
        const float4 q = park[threadIdx.x], cq = park[NT + threadIdx.x];
        const float rd[4] = {q.x, q.y, q.z, q.w}, cc[4] = {cq.x, cq.y, cq.z, cq.w};
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(acc[j], rd[j], cc[j] * lds[(T.ly + R) * SW + 4 * T.lq + R + j]);
        if (sparse) {
            const float4 sq = park[2 * NT + threadIdx.x];
            const float s[4] = {sq.x, sq.y, sq.z, sq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = s[j] > 0.f ? s[j] : v[j];
        }
        store4<VEC>(dst + plane + pix, v, row_in, T.x0, W);
    }
}

// one adjoint step for all C channels: dst(q) = (1 - m)(c(q) src(q) + sum_k g_k(q') (att_ring(k) src / D)(q')), q' = q - off_k, m = [sparse > 0].
// The thread holds the raw gates of its shifted pixels, as kxk_adjoint_step does; att_r / D of the tile and its halo is formed once (fac, one tile
// per ring, from att and the ring sums of kxk_dyn_rings) and multiplied by src per channel (prod).  c of the thread's own pixels comes from the
// same planes.  VEC: W % 4 == 0 and att, rings, src, dst and sparse 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_dyn_adjoint_step(const float* __restrict__ guid, const float* __restrict__ att, size_t astride,
                                                           const float* __restrict__ rings, const float* __restrict__ src, float* __restrict__ dst,
                                                           const float* __restrict__ sparse, int C, int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, SW = TW + 2 * R, SH = TH + 2 * R, SZ = SW * SH;
    __shared__ float fac[R * SZ];
    __shared__ float prod[R * SZ];
    __shared__ float4 park[2 * NT];   // c and the measured depth of the thread's four pixels
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const float* ab = att + (size_t)T.n * astride;
    const float* rb = rings + (size_t)T.n * 2 * R * HW;
    for (int i = threadIdx.x; i < SZ; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = T.y0 - R + r, gx = T.xt0 - R + c;
        float f[R];
#pragma unroll
        for (int q = 0; q < R; ++q) f[q] = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const int o = gy * W + gx;
            float D = ab[o];
#pragma unroll
            for (int q = 0; q < R; ++q) {
                f[q] = ab[(size_t)(q + 1) * HW + o];
                D += fabsf(f[q]) * rb[(size_t)q * HW + o];
            }
            D = 1.f / D;
#pragma unroll
            for (int q = 0; q < R; ++q) f[q] *= D;
        }
#pragma unroll
        for (int q = 0; q < R; ++q) fac[q * SZ + i] = f[q];
    }
    {
        float a[4], Dn[4], Cn[4];
        load4<VEC>(a, ab + pix, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) Dn[j] = Cn[j] = a[j];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            float G[4], Gs[4];
            load4<VEC>(a, ab + (size_t)(q + 1) * HW + pix, row_in, T.x0, W);
            load4<VEC>(G, rb + (size_t)q * HW + pix, row_in, T.x0, W);
            load4<VEC>(Gs, rb + (size_t)(R + q) * HW + pix, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                Dn[j] = fmaf(fabsf(a[j]), G[j], Dn[j]);
                Cn[j] += fabsf(a[j]) * G[j] - a[j] * Gs[j];
            }
        }
        park[threadIdx.x] = make_float4(Cn[0] / Dn[0], Cn[1] / Dn[1], Cn[2] / Dn[2], Cn[3] / Dn[3]);
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (sparse) load4<VEC>(s, sparse + (size_t)T.n * HW + pix, row_in, T.x0, W);
        park[NT + threadIdx.x] = make_float4(s[0], s[1], s[2], s[3]);
    }
    // the gates last: what the tiles and c needed is dead by now, and K = 7 has no register to spare for it
    Quad<float> g[KK];
    const float* gb = guid + (size_t)T.n * KK * HW;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int py = T.y - R + t;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l);
            g[k].clear();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = T.x0 + j - R + l;
                if (yin && T.x0 + j < W && px >= 0 && px < W) g[k].put(j, gb[(size_t)k * HW + py * W + px]);
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)T.n * C + c) * HW;
        const float* sp = src + plane;
        __syncthreads();   // fac is written; the previous channel's reads of prod are done
        for (int i = threadIdx.x; i < SZ; i += NT) {
            const int r = i / SW, cc = i - r * SW;
            const int gy = T.y0 - R + r, gx = T.xt0 - R + cc;
            const float a = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? sp[gy * W + gx] : 0.f;
#pragma unroll
            for (int q = 0; q < R; ++q) prod[q * SZ + i] = fac[q * SZ + i] * a;
        }
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            // a row's reads of prod start when the row above is summed: gathered in front of the stencil they take registers K = 7 does not have
            asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]) : : "memory");
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l), q = ring0<K>(t, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(g[k].get(j), prod[q * SZ + (T.ly + t) * SW + 4 * T.lq + j + l], acc[j]);
            }
        }
        float a[4];
        load4<VEC>(a, sp + pix, row_in, T.x0, W);
        const float4 cq = park[threadIdx.x], sq = park[NT + threadIdx.x];
        const float cc[4] = {cq.x, cq.y, cq.z, cq.w}, s[4] = {sq.x, sq.y, sq.z, sq.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = s[j] > 0.f ? 0.f : fmaf(cc[j], a[j], acc[j]);
        store4<VEC>(dst + plane + pix, acc, row_in, T.x0, W);
    }
}

// PX pixels x0 .. x0 + PX - 1 of a row, PX = 4 (load4 / store4) or 2; VEC: W % 4 == 0 and the plane 16-byte aligned
template <int PX, bool VEC>
__device__ __forceinline__ void loadn(float (&v)[PX], const float* __restrict__ p, bool row_in, int x0, int W) {
    if constexpr (PX == 4) {
        load4<VEC>(v, p, row_in, x0, W);
    } else if (VEC) {
        const float2 q = (row_in && x0 < W) ? *reinterpret_cast<const float2*>(p) : make_float2(0.f, 0.f);
        v[0] = q.x; v[1] = q.y;
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] = (row_in && x0 + j < W) ? p[j] : 0.f;
    }
}

template <int PX, bool VEC>
__device__ __forceinline__ void storen(float* __restrict__ p, const float (&v)[PX], bool row_in, int x0, int W) {
    if constexpr (PX == 4) {
        store4<VEC>(p, v, row_in, x0, W);
    } else {
        if (!row_in) return;
        if (VEC) {
            if (x0 < W) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (x0 + j < W) p[j] = v[j];
        }
    }
}

// pixels a thread of the gradient pass owns: the raw gates and their KK sums are both held in registers, which K = 7 has for two pixels
template <int K>
constexpr int dyn_grad_px() { return K == 7 ? 2 : 4; }

// dL/dguid [N][KK][H][W] and dL/datt [N][n (R+1)][H][W] (each may be NULL), every element written once.  A tile is 64 x 4 PX pixels:
// 64 / PX threads a row, PX pixels of the row each.  Levels: H~_0 = h0, H~_s = hist + (s - 1) L; A_{s+1} = alev + s L (the adjoint steps' outputs,
// (1 - m) applied), A_n = gout.  Over s, then c, with d_k = H~_s(p + off_k) - H~_s(p):
//   acc_k += (att_r / D_s) A_{s+1}(p) d_k         P_r += sum_{k in ring r} g_k A_{s+1}(p) d_k
// after the channels of step s:  T = (sum_r att_r P_r) / D_s,  dL/datt_{s,0} = -T / D_s,  dL/datt_{s,r} = (P_r - T sign(att_r) G_r) / D_s,
// U_r += |att_r| T / D_s (kept in LDS, a word a thread, ring and pixel); after the last step dL/dg_k = acc_k - sign(g_k) U_ring(k).
// G_r = sum_{k in ring r} |g_k| is re-formed from the gate registers where it is used.  VEC: W % 4 == 0 and guid, att, gg and ga 16-byte aligned
template <int K, int PX, bool VEC>
__global__ __launch_bounds__(NT) void kxk_dyn_grad(const float* __restrict__ guid, const float* __restrict__ att, size_t astride,
                                                   const float* __restrict__ h0, const float* __restrict__ hist, const float* __restrict__ alev,
                                                   const float* __restrict__ gout, float* __restrict__ gg, float* __restrict__ ga, int n_iter, size_t L, int C,
                                                   int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, QXG = TW / PX, THG = NT / QXG, SW = TW + 2 * R, SH = THG + 2 * R;
    __shared__ float lds[SH * SW];
    __shared__ float upark[R * PX * NT];   // U_r of the thread's pixels, read and written by this thread alone
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int ly = threadIdx.x / QXG, lq = threadIdx.x % QXG, y0 = ty * THG, xt0 = tx * TW, y = y0 + ly, x0 = xt0 + PX * lq;
    const int HW = H * W;
    const bool row_in = y < H;
    const int pix = y * W + x0;
    float g[KK][PX], acc[KK][PX];
    const float* gp = guid + (size_t)n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        loadn<PX, VEC>(g[k], gp + (size_t)k * HW, row_in, x0, W);
#pragma unroll
        for (int j = 0; j < PX; ++j) acc[k][j] = 0.f;
    }
    // G_r of the thread's pixels, summed in channel order
    auto ring_sums = [&](float (&G)[R][PX]) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < PX; ++j) G[r][j] = 0.f;
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
#pragma unroll
                for (int j = 0; j < PX; ++j) G[ring0<K>(t, l)][j] += fabsf(g[chan<K>(t, l)][j]);
            }
    };
    const float* ab = att + (size_t)n * astride + pix;
    float* gab = ga ? ga + (size_t)n * astride + pix : nullptr;
    for (int it = 0; it < n_iter; ++it) {
        const float* hl = it == 0 ? h0 : hist + (size_t)(it - 1) * L;
        const float* al = it + 1 == n_iter ? gout : alev + (size_t)it * L;
        const float* ap = ab + (size_t)it * (R + 1) * HW;
        float f[R][PX], P[R][PX];
        {
            float G[R][PX], D[PX];
            ring_sums(G);
            loadn<PX, VEC>(D, ap, row_in, x0, W);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                loadn<PX, VEC>(f[r], ap + (size_t)(r + 1) * HW, row_in, x0, W);
#pragma unroll
                for (int j = 0; j < PX; ++j) D[j] = fmaf(fabsf(f[r][j]), G[r][j], D[j]);
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    f[r][j] /= D[j];
                    P[r][j] = 0.f;
                }
        }
        for (int c = 0; c < C; ++c) {
            const size_t plane = ((size_t)n * C + c) * HW;
            __syncthreads();
            for (int i = threadIdx.x; i < SW * SH; i += NT) {   // stage, for a tile of THG rows
                const int r = i / SW, cc = i - r * SW;
                const int gy = y0 - R + r, gx = xt0 - R + cc;
                lds[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? hl[plane + gy * W + gx] : 0.f;
            }
            float a[PX];
            loadn<PX, false>(a, al + plane + pix, row_in, x0, W);
            __syncthreads();
            float cen[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) cen[j] = lds[(ly + R) * SW + PX * lq + R + j];
#pragma unroll
            for (int t = 0; t < K; ++t) {
                float row[PX + 2 * R];   // row y + R - t, columns x0 - R .. x0 + PX - 1 + R
                asm volatile("" : : : "memory");   // one row's reads at a time: the gates and their sums leave no register for more
#pragma unroll
                for (int i = 0; i < PX + 2 * R; ++i) row[i] = lds[(ly + 2 * R - t) * SW + PX * lq + i];
#pragma unroll
                for (int l = 0; l < K; ++l) {
                    if (t == R && l == R) continue;
                    const int k = chan<K>(t, l), r = ring0<K>(t, l);
#pragma unroll
                    for (int j = 0; j < PX; ++j) {
                        const float d = a[j] * (row[j + 2 * R - l] - cen[j]);   // the difference first: it is exact where the level is smooth
                        acc[k][j] = fmaf(f[r][j], d, acc[k][j]);
                        P[r][j] = fmaf(g[k][j], d, P[r][j]);
                    }
                }
            }
        }
        // the step's epilogue: f_r = att_r / D, so T = sum_r f_r P_r; att and D are read and formed again rather than kept over the channels
        float G[R][PX], a0[PX], D[PX], T[PX];
        ring_sums(G);
        loadn<PX, VEC>(a0, ap, row_in, x0, W);
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            D[j] = a0[j];
            T[j] = 0.f;
        }
        float ar[R][PX];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            loadn<PX, VEC>(ar[r], ap + (size_t)(r + 1) * HW, row_in, x0, W);
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                D[j] = fmaf(fabsf(ar[r][j]), G[r][j], D[j]);
                T[j] = fmaf(f[r][j], P[r][j], T[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            D[j] = 1.f / D[j];
            a0[j] = -T[j] * D[j];
        }
        if (gab) storen<PX, VEC>(gab + (size_t)it * (R + 1) * HW, a0, row_in, x0, W);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float d[PX];
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                d[j] = (P[r][j] - T[j] * signf(ar[r][j]) * G[r][j]) * D[j];
                float& u = upark[(r * PX + j) * NT + threadIdx.x];
                u = fmaf(fabsf(ar[r][j]), T[j] * D[j], it ? u : 0.f);
            }
            if (gab) storen<PX, VEC>(gab + ((size_t)it * (R + 1) + r + 1) * HW, d, row_in, x0, W);
        }
    }
    if (!gg) return;
    float* gq = gg + (size_t)n * KK * HW + pix;
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l), r = ring0<K>(t, l);
#pragma unroll
            for (int j = 0; j < PX; ++j) acc[k][j] -= signf(g[k][j]) * upark[(r * PX + j) * NT + threadIdx.x];
            storen<PX, VEC>(gq + (size_t)k * HW, acc[k], row_in, x0, W);
        }
}

// the ring sums of the raw gates for the adjoint steps, step-independent: rings [N][2 R][H][W], plane r - 1 = G_r = sum_{k in ring r} |g_k|,
// plane R + r - 1 = sum_{k in ring r} g_k, each summed in channel order.  VEC: W % 4 == 0, guid and rings 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_dyn_rings(const float* __restrict__ guid, float* __restrict__ rings, int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1;
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    const float* gp = guid + (size_t)T.n * KK * HW + pix;
    float G[2 * R][4];
#pragma unroll
    for (int r = 0; r < 2 * R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) G[r][j] = 0.f;
#pragma unroll
    for (int t = 0; t < K; ++t)
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int r = ring0<K>(t, l);
            float g[4];
            load4<VEC>(g, gp + (size_t)chan<K>(t, l) * HW, row_in, T.x0, W);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                G[r][j] += fabsf(g[j]);
                G[R + r][j] += g[j];
            }
        }
    float* rp = rings + (size_t)T.n * 2 * R * HW + pix;
#pragma unroll
    for (int r = 0; r < 2 * R; ++r) store4<VEC>(rp + (size_t)r * HW, G[r], row_in, T.x0, W);
}

// H~_0: dst = sparse where sparse > 0, else x, for the C channels of an image.  VEC: W % 4 == 0 and x, sparse and dst 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(NT) void kxk_dyn_pin(const float* __restrict__ x, const float* __restrict__ sparse, float* __restrict__ dst, int C, int H, int W,
                                                  int tiles_x, int tiles_y) {
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float s[4];
    load4<VEC>(s, sparse + (size_t)T.n * HW + pix, row_in, T.x0, W);
    for (int c = 0; c < C; ++c) {
        const size_t at = ((size_t)T.n * C + c) * HW + pix;
        float v[4];
        load4<VEC>(v, x + at, row_in, T.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s[j] > 0.f ? s[j] : v[j];
        store4<VEC>(dst + at, v, row_in, T.x0, W);
    }
}

int pin_level(const float* x, const float* sparse, float* dst, const Grid& G, int C, int H, int W, hipStream_t st) {
    with_bool(W % 4 == 0 && aligned16(x) && aligned16(sparse) && aligned16(dst), [&](auto vec) {
        hipLaunchKernelGGL((kxk_dyn_pin<decltype(vec)::value>), dim3(G.blocks), dim3(NT), 0, st, x, sparse, dst, C, H, W, G.tx, G.ty);
    });
    return check_launch("kxk_dyn_pin");
}

template <int K>
int dyn_forward(const float* guid, const float* att, const float* x, const float* sparse, float* out, float* hist, int N, int C, int H, int W, int n_iter,
                void* ws, hipStream_t st) {
    constexpr int R = K / 2;
    const Grid G = grid_of(N, H, W);
    const size_t HW = (size_t)H * W, L = (size_t)N * C * HW, astride = (size_t)n_iter * (R + 1) * HW;
    float* level = (float*)ws;
    const float* src = x;
    if (sparse) {
        if (int e = pin_level(x, sparse, level, G, C, H, W, st)) return e;
        src = level;
        level += kxk_level_floats(L);
    }
    float *ping = level, *pong = level + kxk_level_floats(L);
    for (int it = 1; it <= n_iter; ++it) {
        float* dst = it == n_iter ? out : (hist ? hist + (size_t)(it - 1) * L : ((it & 1) ? ping : pong));
        const float* as = att + (size_t)(it - 1) * (R + 1) * HW;
        const float* sp = it == n_iter ? nullptr : sparse;   // the result is not pinned
        with_bool(W % 4 == 0 && aligned16(guid) && aligned16(att) && aligned16(dst) && aligned16(sparse), [&](auto vec) {
            hipLaunchKernelGGL((kxk_dyn_forward_step<K, decltype(vec)::value>), dim3(G.blocks), dim3(NT), 0, st, guid, as, astride, src, dst, sp, C, H, W, G.tx,
                               G.ty);
        });
        if (int e = check_launch("kxk_dyn_forward_step")) return e;
        src = dst;
    }
    return 0;
}

template <int K>
int dyn_backward(const float* guid, const float* att, const float* x, const float* sparse, const float* hist, const float* gout, float* gg, float* ga,
                 float* gx, int N, int C, int H, int W, int n_iter, void* ws, hipStream_t st) {
    constexpr int R = K / 2, PX = dyn_grad_px<K>();
    const Grid G = grid_of(N, H, W);
    const size_t HW = (size_t)H * W, L = (size_t)N * C * HW, astride = (size_t)n_iter * (R + 1) * HW;
    const KxkDynBackwardWs lay(N, C, H, W, K, n_iter, sparse != nullptr);
    float* alev = (float*)ws;   // A_1 .. A_{n-1}, level t at alev + (t - 1) L
    float* rings = (float*)((char*)ws + lay.rings);
    float* h0 = (float*)((char*)ws + lay.h0);
    const bool grads = gg || ga;
    const int last = gx ? 0 : (grads ? 1 : n_iter);
    if (last < n_iter) {
        with_bool(W % 4 == 0 && aligned16(guid), [&](auto vec) {
            hipLaunchKernelGGL((kxk_dyn_rings<K, decltype(vec)::value>), dim3(G.blocks), dim3(NT), 0, st, guid, rings, H, W, G.tx, G.ty);
        });
        if (int e = check_launch("kxk_dyn_rings")) return e;
    }
    for (int t = n_iter - 1; t >= last; --t) {
        const float* src = t + 1 == n_iter ? gout : alev + (size_t)t * L;
        float* dst = t == 0 ? gx : alev + (size_t)(t - 1) * L;
        const float* as = att + (size_t)t * (R + 1) * HW;
        with_bool(W % 4 == 0 && aligned16(att) && aligned16(src) && aligned16(dst) && aligned16(sparse), [&](auto vec) {
            hipLaunchKernelGGL((kxk_dyn_adjoint_step<K, decltype(vec)::value>), dim3(G.blocks), dim3(NT), 0, st, guid, as, astride, rings, src, dst, sparse, C,
                               H, W, G.tx, G.ty);
        });
        if (int e = check_launch("kxk_dyn_adjoint_step")) return e;
    }
    if (!grads) return 0;
    if (sparse)
        if (int e = pin_level(x, sparse, h0, G, C, H, W, st)) return e;
    constexpr int THG = NT / (TW / PX);
    const int tys = (H + THG - 1) / THG;
    const unsigned blocks = (unsigned)((size_t)N * G.tx * tys);
    with_bool(W % 4 == 0 && aligned16(guid) && aligned16(att) && aligned16(gg) && aligned16(ga), [&](auto vec) {
        hipLaunchKernelGGL((kxk_dyn_grad<K, PX, decltype(vec)::value>), dim3(blocks), dim3(NT), 0, st, guid, att, astride, sparse ? h0 : x, hist, alev, gout, gg, ga,
                           n_iter, L, C, H, W, G.tx, tys);
    });
    return check_launch("kxk_dyn_grad");
}

}  // namespace

int kxk_dyn_forward(const float* guid, const float* att, const float* x, const float* sparse, float* out, float* hist, int N, int C, int H, int W, int K,
                    int n_iter, void* ws, hipStream_t st) {
    return with_k<3, 5, 7>(K, [&](auto k) { return dyn_forward<decltype(k)::value>(guid, att, x, sparse, out, hist, N, C, H, W, n_iter, ws, st); });
}

int kxk_dyn_backward(const float* guid, const float* att, const float* x, const float* sparse, const float* hist, const float* gout, float* gg, float* ga,
                     float* gx, int N, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st) {
    return with_k<3, 5, 7>(K, [&](auto k) {
        return dyn_backward<decltype(k)::value>(guid, att, x, sparse, hist, gout, gg, ga, gx, N, C, H, W, n_iter, ws, st);
    });
}

}  // namespace cspn
