// cspn2d_kxk.hip -- the entries of the 2D K x K engine (cspn2d_kxk_impl.h: the contracts, the kernels and the host paths) at neighbour
// distance one; the dilated instances of the folded and the assembling contract are cspn2d_kxk_dil.hip, so that the two build side by side.
#include "cspn2d_kxk_impl.h"

namespace cspn {

// ---- the entries.  gate / guid in the type of dtype: 0 float32, CSPN_DTYPE_F16 or CSPN_DTYPE_BF16; gg in the same type.  The
// arguments are checked by the caller (cspn_abi.cpp): n_iter >= 1, every view below 2^31 elements, no aliasing, the workspaces as the
// cspn2d_*kxk*_workspace_bytes functions size them ----

// K in {5, 7}; absnorm: the demo module's contract on the raw guide, else the gates as given
int kxk_forward(const void* gate, int dtype, bool absnorm, const float* x, float* out, float* hist, int N, int C, int H, int W, int K, int n_iter,
                void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<5, 7>(K, [&](auto k) {
            return with_bool(absnorm, [&](auto abs) {
                return forward_steps<decltype(k)::value, false, GT, decltype(abs)::value>((const store_t<GT>*)gate, x, out, hist, N, C, H, W, n_iter, ws, st);
            });
        });
    });
}

int kxk_backward(const void* gate, int dtype, bool absnorm, const float* x, const float* hist, const float* gout, void* gg, float* gx, int N, int C,
                 int H, int W, int K, int n_iter, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<5, 7>(K, [&](auto k) {
            return with_bool(absnorm, [&](auto abs) {
                return backward_run<decltype(k)::value, GT, decltype(abs)::value>((const store_t<GT>*)gate, x, hist, gout, (store_t<GT>*)gg, gx, N, C, H, W,
                                                                                 n_iter, ws, st);
            });
        });
    });
}

size_t kxk_norm_fold_floats(int B, int C, int sparse_C, int H, int W, int K) {
    const NormGeo g = norm_geo(B, C, sparse_C, H, W);
    return kxk_level_floats((size_t)g.N * (K * K - 1) * H * W) + kxk_level_floats(g.L);
}

// K in {3, 5, 7}, norm 8SUM / 8SUM_ABS, sparse_C 0 / 1 / C (0 <=> sparse NULL)
int kxk_norm_forward(const void* guid, int dtype, const float* blur, const float* sparse, float* out, float* hist, int B, int C, int sparse_C, int H,
                     int W, int K, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return norm_forward<decltype(k)::value, GT>((const store_t<GT>*)guid, blur, sparse, out, hist, B, C, sparse_C, H, W, n_iter, norm, ws, st);
        });
    });
}

int kxk_norm_backward(const void* guid, int dtype, const float* blur, const float* sparse, const float* hist, const float* gout, void* gg, float* gx,
                      int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return norm_backward<decltype(k)::value, GT>((const store_t<GT>*)guid, blur, sparse, hist, gout, (store_t<GT>*)gg, gx, B, C, sparse_C, H, W,
                                                        n_iter, norm, ws, st);
        });
    });
}

// the assembling contract; n_iter >= 1, steps (host memory) strictly increasing from >= 0 to n_iter, 1 <= T
int kxk_assemble_forward(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out,
                         float* hist, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return assemble_forward<decltype(k)::value, GT>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, out, hist, B, C, sparse_C, H, W, n_iter, norm,
                                                            ws, st);
        });
    });
}

int kxk_assemble_backward(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, const float* hist,
                          const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                          hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return assemble_backward<decltype(k)::value, GT>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, hist, gout, (store_t<GT>*)gg, gx, gc, B, C,
                                                             sparse_C, H, W, n_iter, norm, ws, st);
        });
    });
}

}  // namespace cspn
