// cspn2d_kxk.hip -- the 2D NONE op (Paddle contract: gates used as given, centre-sited, no centre term, any sign) over a K x K
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
#include "cspn_common.h"

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

// the plane s [H][W] of the tile's rows y0 - R .. y0 + TH + R - 1 and columns xt0 - R .. xt0 + TW + R - 1 into lds, zeros outside the image
template <int R>
__device__ __forceinline__ void stage(float* lds, const float* __restrict__ s, int y0, int xt0, int H, int W) {
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    for (int i = threadIdx.x; i < SW * SH; i += NT) {
        const int r = i / SW, c = i - r * SW;
        const int gy = y0 - R + r, gx = xt0 - R + c;
        lds[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? s[gy * W + gx] : 0.f;
    }
}

// four pixels x0 .. x0+3 of row y (p = row offset of x0); VEC: W % 4 == 0 and the plane 16-byte aligned (a quad is then all in or all out)
template <bool VEC>
__device__ __forceinline__ void load4(float (&v)[4], const float* __restrict__ p, bool row_in, int x0, int W) {
    if (VEC) {
        const float4 q = (row_in && x0 < W) ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (row_in && x0 + j < W) ? p[j] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ p, const float (&v)[4], bool row_in, int x0, int W) {
    if (!row_in) return;
    if (VEC) {
        if (x0 < W) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x0 + j < W) p[j] = v[j];
    }
}

// gate channel of the pair (t, l), l != R or t != R
template <int K>
__host__ __device__ constexpr int chan(int t, int l) { return t * K + l - (t * K + l > (K / 2) * (K + 1) ? 1 : 0); }

// one forward step for all C channels: dst = step(src).  VEC: W % 4 == 0, gate and dst 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_forward_step(const float* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst,
                                                       int C, int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, SW = TW + 2 * R;
    __shared__ float lds[(TH + 2 * R) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float g[KK][4];
    const float* gp = gate + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) load4<VEC>(g[k], gp + (size_t)k * HW, row_in, T.x0, W);
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
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(g[k][j], row[j + 2 * R - l], acc[j]);
            }
        }
        store4<VEC>(dst + plane + pix, acc, row_in, T.x0, W);
    }
}

// one adjoint step for all C channels: dst = step^T(src).  The gate of pixel q and channel k is read at q - off_k (zero outside the
// image); VEC: W % 4 == 0 and dst 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_adjoint_step(const float* __restrict__ gate, const float* __restrict__ src, float* __restrict__ dst,
                                                       int C, int H, int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, SW = TW + 2 * R;
    __shared__ float lds[(TH + 2 * R) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    float g[KK][4];
    const float* gb = gate + (size_t)T.n * KK * HW;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const int py = T.y - R + t;
        const bool yin = row_in && py >= 0 && py < H;
#pragma unroll
        for (int l = 0; l < K; ++l) {
            if (t == R && l == R) continue;
            const int k = chan<K>(t, l);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int px = T.x0 + j - R + l;
                g[k][j] = (yin && T.x0 + j < W && px >= 0 && px < W) ? gb[(size_t)k * HW + py * W + px] : 0.f;
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)T.n * C + c) * HW;
        __syncthreads();
        stage<R>(lds, src + plane, T.y0, T.xt0, H, W);
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < K; ++t) {
            float row[4 + 2 * R];   // row y - R + t, columns x0 - R .. x0 + 3 + R
#pragma unroll
            for (int i = 0; i < 4 + 2 * R; ++i) row[i] = lds[(T.ly + t) * SW + 4 * T.lq + i];
#pragma unroll
            for (int l = 0; l < K; ++l) {
                if (t == R && l == R) continue;
                const int k = chan<K>(t, l);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = fmaf(g[k][j], row[j + l], acc[j]);
            }
        }
        store4<VEC>(dst + plane + T.y * W + T.x0, acc, row_in, T.x0, W);
    }
}

// dL/dg for all KK channels of the tile: the levels H_0 = x, H_t = hist + (t - 1) L (t >= 1) and A_t = alev + (t - 1) L (t < n),
// A_n = gout, L = N C H W.  Accumulated over t = 0 .. n-1, then c = 0 .. C-1, written once.  VEC: W % 4 == 0 and gg 16-byte aligned
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void kxk_gate_grad(const float* __restrict__ x, const float* __restrict__ hist, const float* __restrict__ alev,
                                                    const float* __restrict__ gout, float* __restrict__ gg, int n_iter, size_t L, int C, int H,
                                                    int W, int tiles_x, int tiles_y) {
    constexpr int R = K / 2, KK = K * K - 1, SW = TW + 2 * R;
    __shared__ float lds[(TH + 2 * R) * SW];
    const Tile T = tile_of(tiles_x, tiles_y);
    const int HW = H * W;
    const bool row_in = T.y < H;
    const int pix = T.y * W + T.x0;
    float acc[KK][4];
#pragma unroll
    for (int k = 0; k < KK; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
    for (int it = 0; it < n_iter; ++it) {
        const float* hl = it == 0 ? x : hist + (size_t)(it - 1) * L;
        const float* al = it + 1 == n_iter ? gout : alev + (size_t)it * L;
        for (int c = 0; c < C; ++c) {
            const size_t plane = ((size_t)T.n * C + c) * HW;
            __syncthreads();
            stage<R>(lds, hl + plane, T.y0, T.xt0, H, W);
            float a[4];
            load4<false>(a, al + plane + pix, row_in, T.x0, W);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < K; ++t) {
                float row[4 + 2 * R];
#pragma unroll
                for (int i = 0; i < 4 + 2 * R; ++i) row[i] = lds[(T.ly + 2 * R - t) * SW + 4 * T.lq + i];
#pragma unroll
                for (int l = 0; l < K; ++l) {
                    if (t == R && l == R) continue;
                    const int k = chan<K>(t, l);
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[k][j] = fmaf(a[j], row[j + 2 * R - l], acc[k][j]);
                }
            }
        }
    }
    float* gp = gg + (size_t)T.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) store4<VEC>(gp + (size_t)k * HW, acc[k], row_in, T.x0, W);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

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

template <int K>
int forward_steps(const float* gate, const float* x, float* out, float* hist, int N, int C, int H, int W, int n_iter, void* ws, hipStream_t st) {
    const Grid G = grid_of(N, H, W);
    const size_t L = (size_t)N * C * H * W;
    float* ping = (float*)ws;
    float* pong = ping + kxk_level_floats(L);
    const float* src = x;
    for (int it = 1; it <= n_iter; ++it) {
        float* dst = it == n_iter ? out : (hist ? hist + (size_t)(it - 1) * L : ((it & 1) ? ping : pong));
        if (W % 4 == 0 && aligned16(gate) && aligned16(dst))
            hipLaunchKernelGGL((kxk_forward_step<K, true>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty);
        else
            hipLaunchKernelGGL((kxk_forward_step<K, false>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty);
        if (int e = check_launch("kxk_forward_step")) return e;
        src = dst;
    }
    return 0;
}

template <int K>
int backward_run(const float* gate, const float* x, const float* hist, const float* gout, float* gg, float* gx, int N, int C, int H, int W,
                 int n_iter, void* ws, hipStream_t st) {
    const Grid G = grid_of(N, H, W);
    const size_t L = (size_t)N * C * H * W;
    float* alev = (float*)ws;   // A_1 .. A_{n-1}, level t at alev + (t - 1) L
    // the adjoint steps: A_{n-1} .. A_1 always (the gate gradient reads them), A_0 = dL/dx where asked for
    const int last = gx ? 0 : (gg ? 1 : n_iter);
    for (int t = n_iter - 1; t >= last; --t) {
        const float* src = t + 1 == n_iter ? gout : alev + (size_t)t * L;
        float* dst = t == 0 ? gx : alev + (size_t)(t - 1) * L;
        if (W % 4 == 0 && aligned16(dst))
            hipLaunchKernelGGL((kxk_adjoint_step<K, true>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty);
        else
            hipLaunchKernelGGL((kxk_adjoint_step<K, false>), dim3(G.blocks), dim3(NT), 0, st, gate, src, dst, C, H, W, G.tx, G.ty);
        if (int e = check_launch("kxk_adjoint_step")) return e;
    }
    if (!gg) return 0;
    if (W % 4 == 0 && aligned16(gg))
        hipLaunchKernelGGL((kxk_gate_grad<K, true>), dim3(G.blocks), dim3(NT), 0, st, x, hist, alev, gout, gg, n_iter, L, C, H, W, G.tx, G.ty);
    else
        hipLaunchKernelGGL((kxk_gate_grad<K, false>), dim3(G.blocks), dim3(NT), 0, st, x, hist, alev, gout, gg, n_iter, L, C, H, W, G.tx, G.ty);
    return check_launch("kxk_gate_grad");
}

}  // namespace

// arguments checked by the caller (cspn_abi.cpp): K in {5, 7}, n_iter >= 1, N C H W and N KK H W below 2^31, no aliasing, the
// workspace as kxk_workspace_floats / kxk_backward_workspace_floats
int kxk_forward(const float* gate, const float* x, float* out, float* hist, int N, int C, int H, int W, int K, int n_iter, void* ws,
                hipStream_t st) {
    return K == 5 ? forward_steps<5>(gate, x, out, hist, N, C, H, W, n_iter, ws, st) : forward_steps<7>(gate, x, out, hist, N, C, H, W, n_iter, ws, st);
}

int kxk_backward(const float* gate, const float* x, const float* hist, const float* gout, float* gg, float* gx, int N, int C, int H, int W, int K,
                 int n_iter, void* ws, hipStream_t st) {
    return K == 5 ? backward_run<5>(gate, x, hist, gout, gg, gx, N, C, H, W, n_iter, ws, st)
                  : backward_run<7>(gate, x, hist, gout, gg, gx, N, C, H, W, n_iter, ws, st);
}

}  // namespace cspn
