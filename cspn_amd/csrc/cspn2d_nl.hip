// cspn2d_nl.hip -- non-local propagation with learned offsets (the refinement step of NLSPN and of the models built on it), K = 3, forward
// and backward.  aff [B][KK][H][W] used as given (any sign, normalised by the caller), offset [B][2 KK][H][W] (channel 2k is dy_k, 2k + 1
// is dx_k), values [B][C][H][W], the C channels share aff and offset; sparse NULL or [B][H][W], pinned where > 0.
//   neighbour k    the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre, base_k = (t - R, l - R), R = K / 2: the sign of
//                  the deformable convolution, THE OPPOSITE of the K x K engine's off_k = (R - t, R - l) (cspn2d_kxk_impl.h)
//   bil(F, p + base + d)   fy = dy - floor(dy), fx = dx - floor(dx) (the fraction of the OFFSET, exact in float32), (y0, x0) = p + base +
//                  floor(d) in integers, the four corners weighted (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx; a corner outside contributes 0
//   forward        Ht_t = sparse where sparse > 0, else H_t;  H_{t+1}(p) = c(p) Ht_t(p) + sum_k aff_k(p) bil(Ht_t, p + base_k + d_k(p)),
//                  c = 1 - sum_k aff_k, H_0 = x, out = H_n (not pinned)
//   adjoint        At_t(q) = c(q) A_{t+1}(q) + sum_{p,k} aff_k(p) w_{p,k->q} A_{t+1}(p)  (a scatter),  A_t = (1 - m) At_t,  A_n = grad_out
//   gradients      grad_aff_k = sum_t sum_c A_{t+1} (bil_k(Ht_t) - Ht_t),  grad_dy_k = aff_k sum_t sum_c A_{t+1} d bil_k / d fy, likewise dx;
//                  floor has no derivative, d fy / d dy = 1
// Every finite offset is valid: floor(d) is clamped to +-2^29 before it becomes an integer (everything out there is outside the image for
// every shape the entry points take, so the function is unchanged), each corner coordinate is then clamped into the image for its address
// and its weight zeroed where it was outside, tested as !(y0 >= 0 && y0 < H).  A NaN or infinite offset gives an unspecified value, never
// an access outside the tensors: fmaxf / fminf send a NaN floor to the clamp's bound.
// Kernels: nl_forward_step (four adjacent pixels of a row per thread, 16-byte loads of the 24 aff / offset planes where VEC; corner indices and
// weights once, then the channel loop; the level is stored already pinned, so no step gathers sparse at its corners), nl_pin (the pre-pass
// Ht_0, and (1 - m) on grad_x), nl_adjoint_step (one pixel per lane; the adds are summed in an LDS window around the workgroup's tile, then
// added row by row, as 64 adjacent addresses a wave instruction, with atomicAdd(float*) into a level a memset has zeroed first in stream
// order), nl_gate_grad (one pixel per lane, the 8 + 16
// sums in registers over t, then c; every element written once), nl_sample / nl_sample_backward (the sampling operator on the same helpers).
// THE ADJOINT IS NOT RUN-TO-RUN BITWISE: the float atomics add in arrival order, so At_t, and through it every gradient, can differ in its
// last bits between two calls.  The forward (and nl_sample) is bitwise reproducible.  cspn2d_nl_det.hip holds a second backward that is: the same
// levels through a gathering adjoint, then this unit's nl_gate_grad (nl_gate_gradients).
// Storage types: aff is stored as AT and offset as OT, each float, __half or __hip_bfloat16 (the pairs (float, float), (float, T), (T, T); the
// *_g16 entry points).  A 16-bit value is widened exactly where it is read (cspn_gate16.h: widen, ld4g), after which tap_of and every sum are the
// float32 code: the results are bitwise those on the widened tensors.  grad_aff is stored as AT and grad_offset as OT: the float32 sum, rounded
// once to nearest even at its single store (narrow_value).  x, sparse, out, the history and every workspace level are float32 for every pair.
#include "cspn2d_nl_taps.h"

namespace cspn {

namespace {

using namespace nl;   // NT, the bases, Tap / tap_of, Pixel / pixel_of, Grid / pixel_grid: cspn2d_nl_taps.h

constexpr int QX = 16, TW = 4 * QX, TH = NT / QX;   // forward: a 64 x 16 pixel tile, four pixels of a row per thread

// F[i] through a 32-bit byte offset from the plane's (wave-uniform) base: one address register a load instead of two (i < H W <= 2^27)
__device__ __forceinline__ float at32(const float* __restrict__ F, int i) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(F) + ((unsigned)i << 2));
}

// the four corner VALUES of a sample, outside ones 0 (the offset gradient differences them)
__device__ __forceinline__ void corners_of(const Tap& t, const float* __restrict__ F, float (&f)[4]) {
    const float v0 = at32(F, t.i00), v1 = at32(F, t.i00 + t.sx), v2 = at32(F, t.i00 + t.sy), v3 = at32(F, t.i00 + t.sy + t.sx);
    f[0] = (t.ok & 1u) ? v0 : 0.f;
    f[1] = (t.ok & 2u) ? v1 : 0.f;
    f[2] = (t.ok & 4u) ? v2 : 0.f;
    f[3] = (t.ok & 8u) ? v3 : 0.f;
}

// four pixels x0 .. x0+3 of a row; VEC: W % 4 == 0 and the plane 16-byte aligned (a quad is then all in or all out)
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

// four aff / offset values of a row as float32; VEC: W % 4 == 0 and the plane aligned to four of its elements (16 bytes, or 8 for a 16-bit type)
template <class GT, bool VEC>
__device__ __forceinline__ void load4g(float (&v)[4], const store_t<GT>* __restrict__ p, bool row_in, int x0, int W) {
    if constexpr (std::is_same<GT, float>::value) {
        load4<VEC>(v, p, row_in, x0, W);
    } else if (VEC) {
        const float4 q = (row_in && x0 < W) ? ld4g<GT>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (row_in && x0 + j < W) ? widen<GT>(p[j]) : 0.f;
    }
}

struct Quad {
    int n, y, x0;
    bool row_in;
};

__device__ __forceinline__ Quad quad_of(int tiles_x, int tiles_y, int H) {
    int b = blockIdx.x;
    Quad q;
    const int tx = b % tiles_x;
    b /= tiles_x;
    q.y = (b % tiles_y) * TH + threadIdx.x / QX;
    q.n = b / tiles_y;
    q.x0 = tx * TW + 4 * (threadIdx.x % QX);
    q.row_in = q.y < H;
    return q;
}

// dst = sparse where sparse > 0, else src (ZERO: else-branch kept, the pinned pixels set to 0: A_0 = (1 - m) At_0), all C channels; in place
// where dst == src.  VEC: W % 4 == 0, the three 16-byte aligned
template <bool VEC, bool ZERO>
__global__ __launch_bounds__(NT) void nl_pin(const float* src, const float* __restrict__ sparse, float* dst, int C, int H, int W, int tiles_x,
                                             int tiles_y) {
    const Quad q = quad_of(tiles_x, tiles_y, H);
    const int HW = H * W, pix = q.y * W + q.x0;
    float s[4];
    load4<VEC>(s, sparse + (size_t)q.n * HW + pix, q.row_in, q.x0, W);
    for (int c = 0; c < C; ++c) {
        const size_t at = ((size_t)q.n * C + c) * HW + pix;
        float v[4];
        load4<VEC>(v, src + at, q.row_in, q.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = s[j] > 0.f ? (ZERO ? 0.f : s[j]) : v[j];
        store4<VEC>(dst + at, v, q.row_in, q.x0, W);
    }
}

// one forward step for all C channels: dst = step(src), src already pinned; pin != NULL: dst is stored pinned (the level the next step
// reads), NULL: raw (the last step).  VEC: W % 4 == 0, src, dst, pin 16-byte aligned and aff, off to four of their elements.  Per pixel and neighbour the thread keeps
// the corner index, the two fractions, the affinity and six bits (the two corner steps, the four inside flags) over the channel loop: the
// four weights as products would be 128 more registers for four pixels
template <int K, bool VEC, class AT, class OT>
__global__ __launch_bounds__(NT) void nl_forward_step(const store_t<AT>* __restrict__ aff, const store_t<OT>* __restrict__ off, const float* __restrict__ src,
                                                      float* __restrict__ dst, const float* __restrict__ pin, int C, int H, int W, int tiles_x,
                                                      int tiles_y) {
    constexpr int KK = K * K - 1;
    const Quad q = quad_of(tiles_x, tiles_y, H);
    const int HW = H * W, pix = q.y * W + q.x0;
    const store_t<AT>* ap = aff + (size_t)q.n * KK * HW + pix;
    const store_t<OT>* op = off + (size_t)q.n * 2 * KK * HW + pix;
    int i00[KK][4];
    unsigned bits[(KK + 3) / 4][4];   // a byte per neighbour: sx, sy != 0, ok
    float fy[KK][4], fx[KK][4], a[KK][4], cc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < (KK + 3) / 4; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) bits[k][j] = 0u;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        float dy[4], dx[4];
        load4g<AT, VEC>(a[k], ap + (size_t)k * HW, q.row_in, q.x0, W);
        load4g<OT, VEC>(dy, op + (size_t)(2 * k) * HW, q.row_in, q.x0, W);
        load4g<OT, VEC>(dx, op + (size_t)(2 * k + 1) * HW, q.row_in, q.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Tap t = tap_of(dy[j], dx[j], q.y, q.x0 + j, base_y<K>(k), base_x<K>(k), H, W);
            i00[k][j] = t.i00;
            fy[k][j] = t.fy;
            fx[k][j] = t.fx;
            bits[k / 4][j] |= ((t.sx ? 1u : 0u) | (t.sy ? 2u : 0u) | (t.ok << 2)) << (8 * (k % 4));
            cc[j] += a[k][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cc[j] = 1.f - cc[j];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (pin) load4<VEC>(s, pin + (size_t)q.n * HW + pix, q.row_in, q.x0, W);
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)q.n * C + c) * HW;
        const float* F = src + plane;
        float acc[4];
        load4<VEC>(acc, F + pix, q.row_in, q.x0, W);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] *= cc[j];
        // the corner indices are re-derived per channel: left loop-invariant, the compiler keeps all 128 corner addresses in registers
#pragma unroll
        for (int k = 0; k < KK; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(i00[k][j]));
#pragma unroll
        for (int k = 0; k < KK; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned b = bits[k / 4][j] >> (8 * (k % 4));
                const int at = i00[k][j], sx = b & 1u, sy = (b & 2u) ? W : 0;
                const float r0 = at32(F, at), r1 = at32(F, at + sx), r2 = at32(F, at + sy), r3 = at32(F, at + sy + sx);
                const float v0 = (b & 4u) ? r0 : 0.f, v1 = (b & 8u) ? r1 : 0.f, v2 = (b & 16u) ? r2 : 0.f, v3 = (b & 32u) ? r3 : 0.f;
                const float top = fmaf(fx[k][j], v1 - v0, v0), bot = fmaf(fx[k][j], v3 - v2, v2);
                acc[j] = fmaf(a[k][j], fmaf(fy[k][j], bot - top, top), acc[j]);
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = s[j] > 0.f ? s[j] : acc[j];
        store4<VEC>(dst + plane + pix, acc, q.row_in, q.x0, W);
    }
}

// one adjoint step for all C channels, scattered: dst += step^T(A), A = src with (1 - m) applied where mask != NULL (src is then a stored
// At level; NULL: src = grad_out).  dst has been zeroed in stream order.  A workgroup owns a 64 x 16 pixel tile, a wave 64 adjacent pixels of a
// row, four rows in turn.  The adds that land in the tile or within AR pixels of it (nearly all of them: an offset is a few pixels) are summed in
// LDS first (ds_add_f32), everything farther goes to dst as a global float atomic at once; then the LDS window is added to dst row by row, so
// that one wave instruction's global atomics are 64 adjacent addresses whatever the offsets look like, and there are about two of them a
// pixel instead of 4 KK + 1.  Scattered straight from the lanes, the 33 adds a pixel run at a small fraction of the float-atomic rate as soon
// as neighbouring pixels' offsets differ (profiles/nl.md).  Per channel the taps are formed again: the tile's 1024 pixels x 8 taps do not fit
constexpr int AW = 64, AH = 16, AR = 6, LW = AW + 2 * AR, LH = AH + 2 * AR;

__device__ __forceinline__ void scatter_add(float* lds, float* D, int cy, int cx, int wy0, int wx0, int W, float v) {
    const int ly = cy - wy0, lx = cx - wx0;
    // (the LDS add at workgroup scope: LDS has no other, and two adds of one scope are merged into one flat atomic on a selected address)
    if ((unsigned)ly < (unsigned)LH && (unsigned)lx < (unsigned)LW) __hip_atomic_fetch_add(lds + ly * LW + lx, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(D + cy * W + cx, v);
}

template <int K, class AT, class OT>
__global__ __launch_bounds__(NT) void nl_adjoint_step(const store_t<AT>* __restrict__ aff, const store_t<OT>* __restrict__ off, const float* __restrict__ src,
                                                      const float* __restrict__ mask, float* dst, int C, int H, int W, int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    __shared__ float lds[LH * LW];
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y, n = b / tiles_y;
    const int HW = H * W, wy0 = ty * AH - AR, wx0 = tx * AW - AR;   // the window's first row and column (may be outside the image)
    const int x = tx * AW + threadIdx.x % AW;
    for (int c = 0; c < C; ++c) {
        const size_t plane = ((size_t)n * C + c) * HW;
        float* D = dst + plane;
        __syncthreads();   // the previous channel's window has been added to dst
        for (int i = threadIdx.x; i < LH * LW; i += NT) lds[i] = 0.f;
        __syncthreads();
        for (int r = threadIdx.x / AW; r < AH; r += NT / AW) {
            const int y = ty * AH + r, pix = y * W + x;
            if (!(y < H && x < W)) continue;
            if (mask && mask[(size_t)n * HW + pix] > 0.f) continue;   // A(p) = 0: nothing to add
            const float a = src[plane + pix];
            const store_t<AT>* ap = aff + (size_t)n * KK * HW + pix;
            const store_t<OT>* op = off + (size_t)n * 2 * KK * HW + pix;
            float cc = 0.f;
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                const float g = widen<AT>(ap[(size_t)k * HW]);
                const Tap t = tap_of(widen<OT>(op[(size_t)(2 * k) * HW]), widen<OT>(op[(size_t)(2 * k + 1) * HW]), y, x, base_y<K>(k), base_x<K>(k), H, W);
                cc += g;
                const float ga = g * a;
                const int cy1 = t.cy0 + (t.sy ? 1 : 0), cx1 = t.cx0 + t.sx;
                // a weight is zero where its corner is outside the image: what is added lies inside, at the clamped coordinates
                if (t.w[0] != 0.f) scatter_add(lds, D, t.cy0, t.cx0, wy0, wx0, W, t.w[0] * ga);
                if (t.w[1] != 0.f) scatter_add(lds, D, t.cy0, cx1, wy0, wx0, W, t.w[1] * ga);
                if (t.w[2] != 0.f) scatter_add(lds, D, cy1, t.cx0, wy0, wx0, W, t.w[2] * ga);
                if (t.w[3] != 0.f) scatter_add(lds, D, cy1, cx1, wy0, wx0, W, t.w[3] * ga);
            }
            atomicAdd(lds + (y - wy0) * LW + (x - wx0), (1.f - cc) * a);   // the centre term: the pixel itself, inside the window
        }
        __syncthreads();
        for (int i = threadIdx.x; i < LH * LW; i += NT) {
            const float v = lds[i];
            const int gy = wy0 + i / LW, gx = wx0 + i % LW;
            if (v != 0.f && gy >= 0 && gy < H && gx >= 0 && gx < W) atomicAdd(D + gy * W + gx, v);
        }
    }
}

// grad_aff [B][KK][H][W] and grad_offset [B][2 KK][H][W] (either may be NULL), one pixel per lane.  Levels: Ht_0 = h0, Ht_t = hist + (t - 1) L;
// A_{t+1} = gout (t + 1 = n) or (1 - m) alev[t LA] (mask NULL: no m).  The sums run over t, then c, in registers; each element is written once,
// gaff in the type of aff and goff in the type of off (the float32 value rounded at that store)
template <int K, class AT, class OT>
__global__ __launch_bounds__(NT, 4) void nl_gate_grad(const store_t<AT>* __restrict__ aff, const store_t<OT>* __restrict__ off, const float* __restrict__ h0,
                                                   const float* __restrict__ hist, const float* __restrict__ alev, const float* __restrict__ gout,
                                                   const float* __restrict__ mask, store_t<AT>* __restrict__ gaff, store_t<OT>* __restrict__ goff, int n_iter,
                                                   size_t L, size_t LA, int C, int H, int W, int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    const Pixel p = pixel_of(tiles_x, tiles_y, H, W);
    if (!p.in) return;
    const int HW = H * W, pix = p.y * W + p.x;
    const store_t<OT>* op = off + (size_t)p.n * 2 * KK * HW + pix;
    const bool masked = mask && mask[(size_t)p.n * HW + pix] > 0.f;
    Tap tap[KK];
    float ga[KK], gy[KK], gx[KK];
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        tap[k] = tap_of(widen<OT>(op[(size_t)(2 * k) * HW]), widen<OT>(op[(size_t)(2 * k + 1) * HW]), p.y, p.x, base_y<K>(k), base_x<K>(k), H, W);
        ga[k] = gy[k] = gx[k] = 0.f;
    }
    for (int it = 0; it < n_iter; ++it) {
        const bool top = it + 1 == n_iter;
        if (!top && masked) continue;   // A_{t+1}(p) = 0
        const float* hl = it == 0 ? h0 : hist + (size_t)(it - 1) * L;
        const float* al = top ? gout : alev + (size_t)it * LA;
        for (int c = 0; c < C; ++c) {
            const size_t plane = ((size_t)p.n * C + c) * HW;
            const float* F = hl + plane;
            const float a = al[plane + pix], hc = F[pix];
#pragma unroll
            for (int k = 0; k < KK; ++k) {
                asm volatile("" : "+v"(tap[k].i00));   // as in nl_forward_step: no corner address is kept across the loops
                const Tap& t = tap[k];
                float f[4];
                corners_of(t, F, f);
                const float gy1 = 1.f - t.fy, gx1 = 1.f - t.fx;
                const float bil = gy1 * gx1 * f[0] + gy1 * t.fx * f[1] + t.fy * gx1 * f[2] + t.fy * t.fx * f[3];
                ga[k] = fmaf(a, bil - hc, ga[k]);
                gy[k] = fmaf(a, gx1 * (f[2] - f[0]) + t.fx * (f[3] - f[1]), gy[k]);
                gx[k] = fmaf(a, gy1 * (f[1] - f[0]) + t.fy * (f[3] - f[2]), gx[k]);
            }
        }
    }
    if (gaff) {
        store_t<AT>* g = gaff + (size_t)p.n * KK * HW + pix;
#pragma unroll
        for (int k = 0; k < KK; ++k) g[(size_t)k * HW] = narrow_value<AT>(ga[k]);
    }
    if (goff) {
        const store_t<AT>* ap = aff + (size_t)p.n * KK * HW + pix;
        store_t<OT>* g = goff + (size_t)p.n * 2 * KK * HW + pix;
#pragma unroll
        for (int k = 0; k < KK; ++k) {
            const float a = widen<AT>(ap[(size_t)k * HW]);
            g[(size_t)(2 * k) * HW] = narrow_value<OT>(a * gy[k]);
            g[(size_t)(2 * k + 1) * HW] = narrow_value<OT>(a * gx[k]);
        }
    }
}

// the sampling operator: out_k(p) = bil(f, p + base_k + d_k(p)), f [B][H][W] -> out [B][KK][H][W]
template <int K, class OT>
__global__ __launch_bounds__(NT) void nl_sample_kernel(const store_t<OT>* __restrict__ off, const float* __restrict__ f, float* __restrict__ out, int H, int W,
                                                       int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    const Pixel p = pixel_of(tiles_x, tiles_y, H, W);
    if (!p.in) return;
    const int HW = H * W, pix = p.y * W + p.x;
    const store_t<OT>* op = off + (size_t)p.n * 2 * KK * HW + pix;
    const float* F = f + (size_t)p.n * HW;
    float* o = out + (size_t)p.n * KK * HW + pix;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const Tap t = tap_of(widen<OT>(op[(size_t)(2 * k) * HW]), widen<OT>(op[(size_t)(2 * k + 1) * HW]), p.y, p.x, base_y<K>(k), base_x<K>(k), H, W);
        float v = t.w[0] * F[t.i00];
        v = fmaf(t.w[1], F[t.i00 + t.sx], v);
        v = fmaf(t.w[2], F[t.i00 + t.sy], v);
        v = fmaf(t.w[3], F[t.i00 + t.sy + t.sx], v);
        o[(size_t)k * HW] = v;
    }
}

// its backward: gf [B][H][W] (zeroed in stream order) += the scattered gout, goff [B][2 KK][H][W] written once, in the type of off; either may be NULL
template <int K, class OT>
__global__ __launch_bounds__(NT) void nl_sample_backward_kernel(const store_t<OT>* __restrict__ off, const float* __restrict__ f, const float* __restrict__ gout,
                                                                float* gf, store_t<OT>* __restrict__ goff, int H, int W, int tiles_x, int tiles_y) {
    constexpr int KK = K * K - 1;
    const Pixel p = pixel_of(tiles_x, tiles_y, H, W);
    if (!p.in) return;
    const int HW = H * W, pix = p.y * W + p.x;
    const store_t<OT>* op = off + (size_t)p.n * 2 * KK * HW + pix;
    const float* gp = gout + (size_t)p.n * KK * HW + pix;
    const float* F = f + (size_t)p.n * HW;
    float* D = gf ? gf + (size_t)p.n * HW : nullptr;
    store_t<OT>* g = goff ? goff + (size_t)p.n * 2 * KK * HW + pix : nullptr;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const Tap t = tap_of(widen<OT>(op[(size_t)(2 * k) * HW]), widen<OT>(op[(size_t)(2 * k + 1) * HW]), p.y, p.x, base_y<K>(k), base_x<K>(k), H, W);
        const float a = gp[(size_t)k * HW];
        if (D) {
            if (t.w[0] != 0.f) atomicAdd(D + t.i00, t.w[0] * a);
            if (t.w[1] != 0.f) atomicAdd(D + t.i00 + t.sx, t.w[1] * a);
            if (t.w[2] != 0.f) atomicAdd(D + t.i00 + t.sy, t.w[2] * a);
            if (t.w[3] != 0.f) atomicAdd(D + t.i00 + t.sy + t.sx, t.w[3] * a);
        }
        if (g) {
            float c[4];
            corners_of(t, F, c);
            g[(size_t)(2 * k) * HW] = narrow_value<OT>(a * ((1.f - t.fx) * (c[2] - c[0]) + t.fx * (c[3] - c[1])));
            g[(size_t)(2 * k + 1) * HW] = narrow_value<OT>(a * ((1.f - t.fy) * (c[1] - c[0]) + t.fy * (c[3] - c[2])));
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

Grid quad_grid(int N, int H, int W) {
    Grid g;
    g.tx = (W + TW - 1) / TW;
    g.ty = (H + TH - 1) / TH;
    g.blocks = (unsigned)((size_t)N * g.tx * g.ty);
    return g;
}

template <bool ZERO>
int pin_levels(const float* src, const float* sparse, float* dst, int B, int C, int H, int W, hipStream_t st) {
    const Grid g = quad_grid(B, H, W);
    if (W % 4 == 0 && aligned16(src) && aligned16(sparse) && aligned16(dst))
        hipLaunchKernelGGL((nl_pin<true, ZERO>), dim3(g.blocks), dim3(NT), 0, st, src, sparse, dst, C, H, W, g.tx, g.ty);
    else
        hipLaunchKernelGGL((nl_pin<false, ZERO>), dim3(g.blocks), dim3(NT), 0, st, src, sparse, dst, C, H, W, g.tx, g.ty);
    return check_launch("nl_pin");
}

template <int K, class AT, class OT>
int forward(const store_t<AT>* aff, const store_t<OT>* off, const float* x, const float* sparse, float* out, float* hist, int B, int C, int H, int W,
            int n_iter, void* ws, hipStream_t st) {
    constexpr int adt = std::is_same<AT, float>::value ? 0 : CSPN_DTYPE_F16, odt = std::is_same<OT, float>::value ? 0 : CSPN_DTYPE_F16;   // (the width alone)
    const size_t L = (size_t)B * C * H * W, LS = kxk_level_floats(L);
    float* lv[2] = {(float*)ws, (float*)ws + LS};
    const Grid g = quad_grid(B, H, W);
    const bool vec0 = quads_ok(W, adt, {aff}, {sparse}) && quads_ok(W, odt, {off}, {});
    const float* src = x;
    int slot = 0;
    if (sparse) {
        if (int e = pin_levels<false>(x, sparse, lv[0], B, C, H, W, st)) return e;
        src = lv[0];
        slot = 1;
    }
    for (int t = 0; t < n_iter; ++t) {
        const bool last = t + 1 == n_iter;
        float* dst = last ? out : (hist ? hist + (size_t)t * L : lv[slot]);
        const float* pin = last ? nullptr : sparse;
        if (vec0 && aligned16(src) && aligned16(dst))
            hipLaunchKernelGGL((nl_forward_step<K, true, AT, OT>), dim3(g.blocks), dim3(NT), 0, st, aff, off, src, dst, pin, C, H, W, g.tx, g.ty);
        else
            hipLaunchKernelGGL((nl_forward_step<K, false, AT, OT>), dim3(g.blocks), dim3(NT), 0, st, aff, off, src, dst, pin, C, H, W, g.tx, g.ty);
        if (int e = check_launch("nl_forward_step")) return e;
        src = dst;
        if (!hist && !last) slot ^= 1;
    }
    return 0;
}

// the gate gradients from the adjoint levels at the start of ws (the scatter's, or the gather's of cspn2d_nl_det.hip: nl_gate_grad reads both)
template <int K, class AT, class OT>
int gate_gradients(const store_t<AT>* aff, const store_t<OT>* off, const float* x, const float* sparse, const float* hist, const float* gout,
                   store_t<AT>* gaff, store_t<OT>* goff, int B, int C, int H, int W, int n_iter, void* ws, hipStream_t st) {
    if (!gaff && !goff) return 0;
    const size_t L = (size_t)B * C * H * W, LS = kxk_level_floats(L);
    float* alev = (float*)ws;
    const Grid g = pixel_grid(B, H, W);
    const float* h0 = x;
    if (sparse) {
        float* p = alev + (size_t)(n_iter - 1) * LS;
        if (int e = pin_levels<false>(x, sparse, p, B, C, H, W, st)) return e;
        h0 = p;
    }
    hipLaunchKernelGGL((nl_gate_grad<K, AT, OT>), dim3(g.blocks), dim3(NT), 0, st, aff, off, h0, hist, alev, gout, sparse, gaff, goff, n_iter, L, LS, C, H, W,
                       g.tx, g.ty);
    return check_launch("nl_gate_grad");
}

template <int K, class AT, class OT>
int backward(const store_t<AT>* aff, const store_t<OT>* off, const float* x, const float* sparse, const float* hist, const float* gout, store_t<AT>* gaff,
             store_t<OT>* goff, float* gx, int B, int C, int H, int W, int n_iter, void* ws, hipStream_t st) {
    const size_t L = (size_t)B * C * H * W, LS = kxk_level_floats(L);
    float* alev = (float*)ws;   // At_1 .. At_{n-1}
    Grid ga;   // the adjoint step's 64 x 16 tiles
    ga.tx = (W + AW - 1) / AW;
    ga.ty = (H + AH - 1) / AH;
    ga.blocks = (unsigned)((size_t)B * ga.tx * ga.ty);
    for (int t = n_iter - 1; t >= (gx ? 0 : 1); --t) {
        const bool top = t + 1 == n_iter;
        const float* src = top ? gout : alev + (size_t)t * LS;
        float* dst = t == 0 ? gx : alev + (size_t)(t - 1) * LS;
        hipError_t e = hipMemsetAsync(dst, 0, sizeof(float) * L, st);
        if (e != hipSuccess) { set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
        hipLaunchKernelGGL((nl_adjoint_step<K, AT, OT>), dim3(ga.blocks), dim3(NT), 0, st, aff, off, src, top ? nullptr : sparse, dst, C, H, W, ga.tx,
                           ga.ty);
        if (int err = check_launch("nl_adjoint_step")) return err;
    }
    if (gx && sparse)
        if (int e = pin_levels<true>(gx, sparse, gx, B, C, H, W, st)) return e;
    return gate_gradients<K, AT, OT>(aff, off, x, sparse, hist, gout, gaff, goff, B, C, H, W, n_iter, ws, st);
}

}  // namespace

// K is 3: checked by the caller; 5 and 7 are further instances of the templates.  adt / odt: one of the pairs of with_nl_types, checked by the caller
int nl_forward(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, float* out, float* hist, int B, int C, int H, int W,
               int K, int n_iter, void* ws, hipStream_t st) {
    (void)K;
    return with_nl_types(adt, odt, [&](auto ta, auto to) {
        using AT = typename decltype(ta)::type;
        using OT = typename decltype(to)::type;
        return forward<3, AT, OT>((const store_t<AT>*)aff, (const store_t<OT>*)off, x, sparse, out, hist, B, C, H, W, n_iter, ws, st);
    });
}

int nl_backward(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout, void* gaff,
                void* goff, float* gx, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st) {
    (void)K;
    return with_nl_types(adt, odt, [&](auto ta, auto to) {
        using AT = typename decltype(ta)::type;
        using OT = typename decltype(to)::type;
        return backward<3, AT, OT>((const store_t<AT>*)aff, (const store_t<OT>*)off, x, sparse, hist, gout, (store_t<AT>*)gaff, (store_t<OT>*)goff, gx, B, C, H,
                                   W, n_iter, ws, st);
    });
}

int nl_gate_gradients(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout,
                      void* gaff, void* goff, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st) {
    (void)K;
    return with_nl_types(adt, odt, [&](auto ta, auto to) {
        using AT = typename decltype(ta)::type;
        using OT = typename decltype(to)::type;
        return gate_gradients<3, AT, OT>((const store_t<AT>*)aff, (const store_t<OT>*)off, x, sparse, hist, gout, (store_t<AT>*)gaff, (store_t<OT>*)goff, B, C,
                                         H, W, n_iter, ws, st);
    });
}

int nl_sample(const void* off, int odt, const float* f, float* out, int B, int H, int W, int K, hipStream_t st) {
    (void)K;
    const Grid g = pixel_grid(B, H, W);
    with_gate_type(odt, [&](auto to) {
        using OT = typename decltype(to)::type;
        hipLaunchKernelGGL((nl_sample_kernel<3, OT>), dim3(g.blocks), dim3(NT), 0, st, (const store_t<OT>*)off, f, out, H, W, g.tx, g.ty);
    });
    return check_launch("nl_sample");
}

int nl_sample_backward(const void* off, int odt, const float* f, const float* gout, float* gf, void* goff, int B, int H, int W, int K, hipStream_t st) {
    (void)K;
    if (gf) {
        hipError_t e = hipMemsetAsync(gf, 0, sizeof(float) * (size_t)B * H * W, st);
        if (e != hipSuccess) { set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    }
    const Grid g = pixel_grid(B, H, W);
    with_gate_type(odt, [&](auto to) {
        using OT = typename decltype(to)::type;
        hipLaunchKernelGGL((nl_sample_backward_kernel<3, OT>), dim3(g.blocks), dim3(NT), 0, st, (const store_t<OT>*)off, f, gout, gf, (store_t<OT>*)goff, H, W,
                           g.tx, g.ty);
    });
    return check_launch("nl_sample_backward");
}

}  // namespace cspn
