// cspn2d_nl_det.hip -- the run-to-run bitwise backward of non-local propagation (cspn2d_backward_nl_det_f32) and of the sampling operator
// (cspn2d_nl_sample_backward_det_f32).  The contract, the neighbour order and tap_of are cspn2d_nl.hip's (cspn2d_nl_taps.h); what differs is
// how the adjoint of the bilinear gather is formed: not as a scatter with float atomics, but as a GATHER through an inverted index of the
// operator, whose sums do not depend on the order of their terms.  This unit holds no float atomic, on global memory or on LDS.
//
//   the index      per call (it is the same for all n steps), in CSR form over the P = B H W destinations q: start[q] .. start[q + 1] (uint32:
//                  at most 32 P <= 2^32 - 2 entries, by the entry points' guard B 16 H W <= 2^31 - 1) delimit q's list of 8-byte entries
//                      code = p 32 + k 4 + corner   (uint32; p the source pixel within the image, H W <= 2^27)
//                      coef = fl32(aff_k(p) w_corner(p, k))     (the sampling operator: w alone)
//                  one for every tap with a non-zero weight that lands on q (a corner outside the image has weight 0, as in the scatter).
//                  Built in three steps: nl_index_taps<false> counts the taps per destination with integer atomics, three plain passes scan
//                  the counts exclusively (nl_scan_tiles: 2048 counts a workgroup and the tile's sum; nl_scan_sums: one workgroup scans the
//                  sums; nl_scan_add), nl_index_taps<true> fills the lists through an integer atomic cursor per destination.  The order of the
//                  entries within a list is whatever the fill gives.  The propagation index also keeps the plane c(q) = 1 - sum_k aff_k(q),
//                  summed in k order.  Lists of more than NL_DET_LONG = 128 entries are put on a worklist (nl_scan_tiles, through an integer
//                  atomic counter).  Counts, cursors and the worklist counter are zeroed by the call, in stream order.
//   the sum        for destination q, level t and channel c the terms are tau_0 = fl32(c(q) A_{t+1}(q)) and tau_i = fl32(coef_i A_{t+1}(p_i));
//                  m of them.  With e = ilogb(max |tau_i|), L = ceil(log2 m) and s = 61 - e - L, each term is quantised as
//                  q_i = llrint(ldexp((double)tau_i, s)) (the scaling exact, the rounding to nearest even, |q_i| <= 2^(62 - L)), the q_i are added
//                  in int64 (associative: any order and any split give the same S, |S| <= 2^62), and ldexpf(__ll2float_rn(S), -s) is stored.
//                  All terms zero: +0.  A NaN term, or infinities of both signs: the quiet NaN 0x7fc00000; else an infinite term: that
//                  infinity.  The result is a function of the multiset of terms alone.  Error against the exact sum of the tau_i: one float32
//                  rounding plus at most m 2^(-s-1) <= 2^(2L - 62) max |tau_i| (terms of 2^(38 - L) times less than the largest are the first
//                  to lose bits: none does for L <= 15).
//   the kernels    nl_gather_step: one lane per destination, coalesced over q; per channel two passes over the list, the maximum and the
//                  sum (over the wave's terms staged in LDS, see there); it stores A_t = (1 - m(q)) At_t(q) directly, so the stored levels are the ones nl_gate_grad
//                  reads, grad_x needs no pinning pass and no level is zeroed first.  nl_gather_long: one WAVE per worklist entry, a strided
//                  loop over the list, a wave reduction of the maximum and one of the int64 sum (a list holds up to 32 H W entries when every
//                  offset points at one pixel).  The sampling operator: the same index with aff = NULL, the gather reads grad_out[n][k][p]
//                  with k from the code; grad_offset is written once by cspn2d_nl.hip's kernel.
//   storage types  aff stored as AT, offset as OT (cspn2d_nl.hip): nl_index_taps widens them where it reads them, so the coefficients
//                  fl32(aff w) and the plane c are formed from the widened values, and the index, the gathers and every level are what they are for
//                  float32 tensors.
#include "cspn2d_nl_taps.h"

namespace cspn {

namespace {

using namespace nl;

constexpr int SCAN_PER = (int)(NL_DET_SCAN_TILE / NT);   // counts a thread
static_assert(SCAN_PER * NT == (int)NL_DET_SCAN_TILE, "a scan tile is a whole number of counts a thread");

// count (FILL false: start[q] += 1, and the plane c) or fill (FILL true: the entry at start[q] + cursor[q]++) the taps of one source pixel
template <int K, bool FILL, class AT, class OT>
__global__ __launch_bounds__(NT) void nl_index_taps(const store_t<AT>* __restrict__ aff, const store_t<OT>* __restrict__ off, unsigned* start, unsigned* cursor,
                                                    uint2* __restrict__ ent, size_t cap, float* __restrict__ cpl, int H, int W, int tiles_x,
                                                    int tiles_y) {
    constexpr int KK = K * K - 1;
    const Pixel p = pixel_of(tiles_x, tiles_y, H, W);
    if (!p.in) return;
    const int HW = H * W, pix = p.y * W + p.x;
    const store_t<OT>* op = off + (size_t)p.n * 2 * KK * HW + pix;
    const store_t<AT>* ap = aff ? aff + (size_t)p.n * KK * HW + pix : nullptr;
    unsigned* st = start + (size_t)p.n * HW;
    unsigned* cu = cursor + (size_t)p.n * HW;
    float cc = 0.f;
#pragma unroll
    for (int k = 0; k < KK; ++k) {
        const float g = ap ? widen<AT>(ap[(size_t)k * HW]) : 1.f;
        const Tap t = tap_of(widen<OT>(op[(size_t)(2 * k) * HW]), widen<OT>(op[(size_t)(2 * k + 1) * HW]), p.y, p.x, base_y<K>(k), base_x<K>(k), H, W);
        cc += g;
        // a weight is zero where its corner is outside the image: every destination lies inside, at the clamped coordinates
        const int d[4] = {t.i00, t.i00 + t.sx, t.i00 + t.sy, t.i00 + t.sy + t.sx};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (t.w[j] == 0.f) continue;
            if (FILL) {
                const size_t at = (size_t)st[d[j]] + atomicAdd(cu + d[j], 1u);
                if (at < cap) ent[at] = make_uint2((unsigned)pix * 32u + (unsigned)(k * 4 + j), __float_as_uint(ap ? g * t.w[j] : t.w[j]));
            } else {
                atomicAdd(st + d[j], 1u);
            }
        }
    }
    if (!FILL && cpl) cpl[(size_t)p.n * HW + pix] = 1.f - cc;
}

// the exclusive scan of v over the workgroup (s: NT words of LDS); total: the workgroup's sum
__device__ __forceinline__ unsigned block_scan(unsigned* s, unsigned v, unsigned& total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const unsigned a = tid >= d ? s[tid - d] : 0u;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    total = s[NT - 1];
    const unsigned incl = s[tid];
    __syncthreads();
    return incl - v;
}

// pass 1: each tile of 2048 counts scanned in place, its sum to sums[tile]; the destinations with a long list go on the worklist
__global__ __launch_bounds__(NT) void nl_scan_tiles(unsigned* start, unsigned* __restrict__ sums, unsigned* __restrict__ work, unsigned* nwork,
                                                    unsigned work_cap, size_t P) {
    __shared__ unsigned s[NT];
    const size_t base = (size_t)blockIdx.x * NL_DET_SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    unsigned v[SCAN_PER], sum = 0u;
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
        v[j] = base + j < P ? start[base + j] : 0u;
        if (v[j] > NL_DET_LONG) {
            const unsigned slot = atomicAdd(nwork, 1u);
            if (slot < work_cap) work[slot] = (unsigned)(base + j);
        }
        sum += v[j];
    }
    unsigned total;
    unsigned run = block_scan(s, sum, total);
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j) {
        if (base + j < P) start[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// pass 2, one workgroup: the tiles' sums scanned in place, NT at a time with a carry; the grand total to *total (start[P])
__global__ __launch_bounds__(NT) void nl_scan_sums(unsigned* sums, unsigned tiles, unsigned* total) {
    __shared__ unsigned s[NT];
    unsigned carry = 0u;
    for (unsigned base = 0; base < tiles; base += NT) {
        const unsigned i = base + threadIdx.x;
        const unsigned v = i < tiles ? sums[i] : 0u;
        unsigned tot;
        const unsigned ex = block_scan(s, v, tot);
        if (i < tiles) sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// pass 3: every start of a tile moved up by the sum of the tiles before it
__global__ __launch_bounds__(NT) void nl_scan_add(unsigned* start, const unsigned* __restrict__ sums, size_t P) {
    const size_t base = (size_t)blockIdx.x * NL_DET_SCAN_TILE + (size_t)threadIdx.x * SCAN_PER;
    const unsigned add = sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SCAN_PER; ++j)
        if (base + j < P) start[base + j] += add;
}

// ---- the order-independent sum ----
// pass 1 over a term: the largest finite magnitude; infinities and NaNs are added up on their own (inf + inf = inf, inf - inf = NaN, NaN stays)
__device__ __forceinline__ void see(float t, float& mx, float& sp) {
    const float a = fabsf(t);
    if (a < INFINITY) mx = fmaxf(mx, a);
    else sp += t;
}

// s = 61 - e - L for m >= 1 terms of magnitude <= mx (finite, > 0)
__device__ __forceinline__ int scale_of(float mx, unsigned m) { return 61 - ilogbf(mx) - (m <= 1u ? 0 : 32 - __clz((int)(m - 1u))); }

__device__ __forceinline__ long long quantise(float t, int s) { return llrint(ldexp((double)t, s)); }

__device__ __forceinline__ float special(float sp) { return sp == sp ? sp : __uint_as_float(0x7fc00000u); }

// the value an entry multiplies: A_{t+1}(p) of the channel's plane, or (SAMPLE) grad_out[k][p] of the image
template <bool SAMPLE>
__device__ __forceinline__ float term(const uint2 e, const float* __restrict__ A, int HW) {
    const int p = min((int)(e.x >> 5), HW - 1);   // (a filled entry's p is inside the plane: the clamp keeps any other word's read inside too)
    const int at = SAMPLE ? (int)((e.x >> 2) & 7u) * HW + p : p;
    return __fmul_rn(__uint_as_float(e.y), A[at]);
}

// one adjoint step for all C channels, gathered: dst(q) = (1 - m(q)) (c(q) src(q) + sum_i coef_i src(p_i)), one lane per destination.  src is
// grad_out or a stored level A_{t+1} (already (1 - m) A~).  SAMPLE: C = 1, no centre term, no mask, src = grad_out [B][KK][H][W].  A destination
// on the worklist is left to nl_gather_long (a pinned one is written here: its zeros).
// A wave's 64 destinations are adjacent pixels of a row, so their lists are ONE contiguous range of the entries.  Walked by each lane from
// global memory, the 64 loads of a wave instruction fall into 64 cache lines; so per channel the wave first forms the terms of its whole range
// with coalesced loads of the entries (lane j takes entries j, j + 64, ..), keeps them in STAGE floats of LDS, and each lane then makes its
// two passes over its own piece there.  A range of more than STAGE entries (a long list among the 64) is walked from global memory as before
constexpr int STAGE = 3072;   // terms a wave: 64 lists of up to 32 taps are 2048, the rest is for strays

template <bool SAMPLE>
__global__ __launch_bounds__(NT) void nl_gather_step(const unsigned* __restrict__ start, const uint2* __restrict__ ent, const float* __restrict__ cpl,
                                                     const float* __restrict__ src, const float* __restrict__ mask, float* __restrict__ dst, size_t cap,
                                                     int C, int KK, int H, int W, int tiles_x, int tiles_y) {
    __shared__ float lds[(NT / 64) * STAGE];
    const Pixel p = pixel_of(tiles_x, tiles_y, H, W);   // (no lane leaves before the last barrier)
    const int HW = H * W, pix = p.in ? p.y * W + p.x : 0;
    const size_t q = p.in ? (size_t)p.n * HW + pix : 0;
    const bool pinned = p.in && !SAMPLE && mask && mask[q] > 0.f;
    unsigned b = 0u, cnt = 0u;
    if (p.in) {
        b = start[q];
        cnt = start[q + 1] - b;
    }
    const bool valid = p.in && (size_t)b + cnt <= cap;   // (always, for the starts the scan made)
    // the wave's range [b0, b1) of the entries
    unsigned b0 = valid ? b : 0xffffffffu, b1 = valid ? b + cnt : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        b0 = min(b0, (unsigned)__shfl_xor((int)b0, d, 64));
        b1 = max(b1, (unsigned)__shfl_xor((int)b1, d, 64));
    }
    const unsigned len = b1 > b0 ? b1 - b0 : 0u, lane = threadIdx.x & 63u;
    const bool staged = len <= (unsigned)STAGE;   // wave-uniform
    float* T = lds + (threadIdx.x / 64) * STAGE;
    const bool walk = valid && !pinned && cnt <= NL_DET_LONG;
    const uint2* E = ent + (size_t)b;
    const unsigned at = staged && valid ? b - b0 : 0u;   // the lane's piece of T: at + cnt <= len
    const float cq = (SAMPLE || !walk) ? 0.f : cpl[q];
    for (int c = 0; c < C; ++c) {
        const float* A = src + (SAMPLE ? (size_t)p.n * KK : (size_t)p.n * C + c) * HW;
        if (staged)
            for (unsigned i = lane; i < len; i += 64u) T[i] = term<SAMPLE>(ent[(size_t)b0 + i], A, HW);
        __syncthreads();
        if (pinned) {
            dst[((size_t)p.n * C + c) * HW + pix] = 0.f;
        } else if (walk) {
            float mx = 0.f, sp = 0.f;
            const float t0 = SAMPLE ? 0.f : __fmul_rn(cq, A[pix]);
            see(t0, mx, sp);
            for (unsigned i = 0; i < cnt; ++i) see(staged ? T[at + i] : term<SAMPLE>(E[i], A, HW), mx, sp);
            float r = 0.f;
            if (sp != 0.f) {
                r = special(sp);
            } else if (mx != 0.f) {
                const int s = scale_of(mx, cnt + (SAMPLE ? 0u : 1u));
                long long S = quantise(t0, s);
                for (unsigned i = 0; i < cnt; ++i) S += quantise(staged ? T[at + i] : term<SAMPLE>(E[i], A, HW), s);
                r = ldexpf(__ll2float_rn(S), -s);
            }
            dst[((size_t)p.n * C + c) * HW + pix] = r;
        }
        __syncthreads();   // T is formed again for the next channel
    }
}

// the same sum for the destinations on the worklist, one wave each: the lanes stride over the list, the maximum and the int64 sum are reduced
// over the wave (an integer sum: any split gives the same S)
template <bool SAMPLE>
__global__ __launch_bounds__(NT) void nl_gather_long(const unsigned* __restrict__ start, const uint2* __restrict__ ent, const float* __restrict__ cpl,
                                                     const float* __restrict__ src, const float* __restrict__ mask, float* __restrict__ dst,
                                                     const unsigned* __restrict__ work, const unsigned* __restrict__ nwork, unsigned work_cap, size_t P,
                                                     size_t cap, int C, int KK, int HW) {
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (NT / 64);
    const unsigned nw = min(*nwork, work_cap);
    for (unsigned w = blockIdx.x * (NT / 64) + threadIdx.x / 64; w < nw; w += waves) {
        const unsigned q = work[w];
        if (q >= P) continue;   // (never: the worklist holds destinations)
        const int n = (int)(q / (unsigned)HW), pix = (int)(q % (unsigned)HW);
        if (!SAMPLE && mask && mask[q] > 0.f) continue;   // pinned: nl_gather_step stored its zeros
        const unsigned b = start[q], cnt = start[q + 1] - b;
        if ((size_t)b + cnt > cap) continue;
        const uint2* E = ent + (size_t)b;
        const float cq = SAMPLE ? 0.f : cpl[q];
        for (int c = 0; c < C; ++c) {
            const float* A = src + (SAMPLE ? (size_t)n * KK : (size_t)n * C + c) * HW;
            float mx = 0.f, sp = 0.f;
            const float t0 = (SAMPLE || lane != 0u) ? 0.f : __fmul_rn(cq, A[pix]);   // the centre term: lane 0's
            see(t0, mx, sp);
            for (unsigned i = lane; i < cnt; i += 64u) see(term<SAMPLE>(E[i], A, HW), mx, sp);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                mx = fmaxf(mx, __shfl_xor(mx, d, 64));
                sp += __shfl_xor(sp, d, 64);   // zeros, infinities and NaNs only: the class of the sum does not depend on the order
            }
            float r = 0.f;
            if (sp != 0.f) {
                r = special(sp);
            } else if (mx != 0.f) {
                const int s = scale_of(mx, cnt + (SAMPLE ? 0u : 1u));
                long long S = quantise(t0, s);
                for (unsigned i = lane; i < cnt; i += 64u) S += quantise(term<SAMPLE>(E[i], A, HW), s);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) S += __shfl_xor(S, d, 64);
                r = ldexpf(__ll2float_rn(S), -s);
            }
            if (lane == 0u) dst[((size_t)n * C + c) * HW + pix] = r;
        }
    }
}

struct Index {
    unsigned *nwork, *start, *cursor, *work, *sums;
    float* cpl;
    uint2* ent;
    NlDetIndex lay;
    Index(void* base, size_t P, bool has_c) : lay(P, has_c) {
        char* b = (char*)base;
        nwork = (unsigned*)(b + lay.counter);
        start = (unsigned*)(b + lay.start);
        cursor = (unsigned*)(b + lay.cursor);
        cpl = has_c ? (float*)(b + lay.cplane) : nullptr;
        work = (unsigned*)(b + lay.work);
        sums = (unsigned*)(b + lay.sums);
        ent = (uint2*)(b + lay.entries);
    }
};

template <int K, class AT, class OT>
int build_index(const Index& ix, const store_t<AT>* aff, const store_t<OT>* off, int B, int H, int W, hipStream_t st) {
    const size_t P = (size_t)B * H * W;
    // the worklist counter, the counts and the cursors lie in a row: zeroed here, in stream order
    hipError_t e = hipMemsetAsync(ix.nwork, 0, ix.lay.zeroed, st);
    if (e != hipSuccess) { set_error("hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    const Grid g = pixel_grid(B, H, W);
    hipLaunchKernelGGL((nl_index_taps<K, false, AT, OT>), dim3(g.blocks), dim3(NT), 0, st, aff, off, ix.start, ix.cursor, ix.ent, ix.lay.cap, ix.cpl, H, W,
                       g.tx, g.ty);
    if (int err = check_launch("nl_index_taps (count)")) return err;
    hipLaunchKernelGGL(nl_scan_tiles, dim3(ix.lay.tiles), dim3(NT), 0, st, ix.start, ix.sums, ix.work, ix.nwork, ix.lay.work_cap, P);
    if (int err = check_launch("nl_scan_tiles")) return err;
    hipLaunchKernelGGL(nl_scan_sums, dim3(1), dim3(NT), 0, st, ix.sums, ix.lay.tiles, ix.start + P);
    if (int err = check_launch("nl_scan_sums")) return err;
    hipLaunchKernelGGL(nl_scan_add, dim3(ix.lay.tiles), dim3(NT), 0, st, ix.start, ix.sums, P);
    if (int err = check_launch("nl_scan_add")) return err;
    hipLaunchKernelGGL((nl_index_taps<K, true, AT, OT>), dim3(g.blocks), dim3(NT), 0, st, aff, off, ix.start, ix.cursor, ix.ent, ix.lay.cap, ix.cpl, H, W,
                       g.tx, g.ty);
    return check_launch("nl_index_taps (fill)");
}

template <bool SAMPLE>
int gather(const Index& ix, const float* src, const float* mask, float* dst, int B, int C, int KK, int H, int W, hipStream_t st) {
    const Grid g = pixel_grid(B, H, W);
    hipLaunchKernelGGL((nl_gather_step<SAMPLE>), dim3(g.blocks), dim3(NT), 0, st, ix.start, ix.ent, ix.cpl, src, mask, dst, ix.lay.cap, C, KK, H, W,
                       g.tx, g.ty);
    if (int err = check_launch("nl_gather_step")) return err;
    const unsigned want = (ix.lay.work_cap + NT / 64 - 1) / (NT / 64), most = (unsigned)num_cus() * 4u;
    hipLaunchKernelGGL((nl_gather_long<SAMPLE>), dim3(want < most ? want : most), dim3(NT), 0, st, ix.start, ix.ent, ix.cpl, src, mask, dst, ix.work,
                       ix.nwork, ix.lay.work_cap, (size_t)B * H * W, ix.lay.cap, C, KK, H * W);
    return check_launch("nl_gather_long");
}

}  // namespace

int nl_backward_det(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout,
                    void* gaff, void* goff, float* gx, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st) {
    const size_t L = (size_t)B * C * H * W, LS = kxk_level_floats(L);
    float* alev = (float*)ws;   // A_1 .. A_{n-1} (and the pinned H_0 of the gate gradient), then the index
    const int lowest = gx ? 0 : 1;
    if (n_iter - 1 >= lowest) {
        const Index ix((char*)ws + sizeof(float) * LS * (size_t)nl_backward_levels(n_iter, sparse != nullptr), (size_t)B * H * W, true);
        const int e = with_nl_types(adt, odt, [&](auto ta, auto to) {
            using AT = typename decltype(ta)::type;
            using OT = typename decltype(to)::type;
            return build_index<3, AT, OT>(ix, (const store_t<AT>*)aff, (const store_t<OT>*)off, B, H, W, st);
        });
        if (e) return e;
        for (int t = n_iter - 1; t >= lowest; --t) {
            const float* src = t + 1 == n_iter ? gout : alev + (size_t)t * LS;
            float* dst = t == 0 ? gx : alev + (size_t)(t - 1) * LS;
            if (int e = gather<false>(ix, src, sparse, dst, B, C, K * K - 1, H, W, st)) return e;
        }
    }
    return nl_gate_gradients(aff, adt, off, odt, x, sparse, hist, gout, gaff, goff, B, C, H, W, K, n_iter, ws, st);
}

int nl_sample_backward_det(const void* off, int odt, const float* f, const float* gout, float* gf, void* goff, int B, int H, int W, int K, void* ws,
                           hipStream_t st) {
    if (gf) {
        const Index ix(ws, (size_t)B * H * W, false);
        const int e = with_gate_type(odt, [&](auto to) {
            using OT = typename decltype(to)::type;
            return build_index<3, float, OT>(ix, (const float*)nullptr, (const store_t<OT>*)off, B, H, W, st);
        });
        if (e) return e;
        if (int e = gather<true>(ix, gout, nullptr, gf, B, 1, K * K - 1, H, W, st)) return e;
    }
    return goff ? nl_sample_backward(off, odt, f, gout, nullptr, goff, B, H, W, K, st) : 0;
}

}  // namespace cspn
