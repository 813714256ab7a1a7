// cspn2d_kxk_dil.hip -- the dilated instances of the 2D K x K engine's folded (depth-completion) and assembling contracts: the neighbour
// offset of gate channel k = (t, l) is D (R - t, R - l), D out of Dilations (cspn2d_kxk_impl.h), everything else as at D = 1.  A
// translation unit of its own so that it builds beside cspn2d_kxk.hip.  D = 1 is not instantiated here: the caller (cspn_abi.cpp) sends
// it to the entries of cspn2d_kxk.hip.
#include "cspn2d_kxk_impl.h"

namespace cspn {

bool kxk_dilation_ok(int D) { return D == 1 || dilation_listed(Dilations{}, D); }

// the arguments of kxk_norm_forward / kxk_norm_backward / kxk_assemble_forward / kxk_assemble_backward with D behind K; D checked by the
// caller to be in the list
int kxk_norm_forward_dil(const void* guid, int dtype, const float* blur, const float* sparse, float* out, float* hist, int B, int C, int sparse_C, int H,
                         int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return with_dilation(Dilations{}, D, [&](auto d) {
                return norm_forward<decltype(k)::value, GT, decltype(d)::value>((const store_t<GT>*)guid, blur, sparse, out, hist, B, C, sparse_C, H, W, n_iter,
                                                                                norm, ws, st);
            });
        });
    });
}

int kxk_norm_backward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* hist, const float* gout, void* gg, float* gx,
                          int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return with_dilation(Dilations{}, D, [&](auto d) {
                return norm_backward<decltype(k)::value, GT, decltype(d)::value>((const store_t<GT>*)guid, blur, sparse, hist, gout, (store_t<GT>*)gg, gx, B, C,
                                                                                 sparse_C, H, W, n_iter, norm, ws, st);
            });
        });
    });
}

int kxk_assemble_forward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out,
                             float* hist, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return with_dilation(Dilations{}, D, [&](auto d) {
                return assemble_forward<decltype(k)::value, GT, decltype(d)::value>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, out, hist, B, C,
                                                                                    sparse_C, H, W, n_iter, norm, ws, st);
            });
        });
    });
}

int kxk_assemble_backward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                              const float* hist, const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int D,
                              int n_iter, int norm, void* ws, hipStream_t st) {
    return with_gate_type(dtype, [&](auto gt) {
        using GT = typename decltype(gt)::type;
        return with_k<3, 5, 7>(K, [&](auto k) {
            return with_dilation(Dilations{}, D, [&](auto d) {
                return assemble_backward<decltype(k)::value, GT, decltype(d)::value>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, hist, gout,
                                                                                     (store_t<GT>*)gg, gx, gc, B, C, sparse_C, H, W, n_iter, norm, ws, st);
            });
        });
    });
}

}  // namespace cspn
