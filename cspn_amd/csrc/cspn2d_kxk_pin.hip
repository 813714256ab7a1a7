// cspn2d_kxk_pin.hip -- the pinned instances of the 2D K x K engine's folded (depth-completion) and assembling contracts: after every step
// the level is blended with the measured depth, H = u step(H) + m sparse, m = sign(sparse) pin_conf (cspn2d_kxk_impl.h: PIN, kxk_fold_pin,
// kxk_unfold_pixel_pin).  Only the fold and its adjoint are new kernels; the steps, the gate gradient and the un-siting between them are the
// unpinned contract's templates, instantiated here once more so that this translation unit builds beside cspn2d_kxk.hip and
// cspn2d_kxk_dil.hip.  D = 1 and every dilated instance.
#include "cspn2d_kxk_impl.h"

namespace cspn {

namespace {

// D as a constant: 1, or one out of Dilations (checked by the caller: kxk_dilation_ok)
template <class F>
int with_any_dilation(int D, F&& f) {
    if (D == 1) return f(std::integral_constant<int, 1>{});
    return with_dilation(Dilations{}, D, f);
}

// gate type, K and D of a pinned call as template arguments
template <class F>
int with_pinned_instance(int dtype, int K, int D, F&& f) {
    return with_gate_type(dtype, [&](auto gt) {
        return with_k<3, 5, 7>(K, [&](auto k) { return with_any_dilation(D, [&](auto d) { return f(gt, k, d); }); });
    });
}

}  // namespace

int kxk_norm_forward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, float* out, float* hist, int B, int C,
                         int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_pinned_instance(dtype, K, D, [&](auto gt, auto k, auto d) {
        using GT = typename decltype(gt)::type;
        return norm_forward<decltype(k)::value, GT, decltype(d)::value, true>((const store_t<GT>*)guid, blur, sparse, out, hist, B, C, sparse_C, H, W, n_iter,
                                                                              norm, ws, st, pin);
    });
}

int kxk_norm_backward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* hist, const float* gout, void* gg,
                          float* gx, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_pinned_instance(dtype, K, D, [&](auto gt, auto k, auto d) {
        using GT = typename decltype(gt)::type;
        return norm_backward<decltype(k)::value, GT, decltype(d)::value, true>((const store_t<GT>*)guid, blur, sparse, hist, gout, (store_t<GT>*)gg, gx, B, C,
                                                                               sparse_C, H, W, n_iter, norm, ws, st, pin);
    });
}

int kxk_assemble_forward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* conf, const int* steps, int T,
                             float* out, float* hist, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st) {
    return with_pinned_instance(dtype, K, D, [&](auto gt, auto k, auto d) {
        using GT = typename decltype(gt)::type;
        return assemble_forward<decltype(k)::value, GT, decltype(d)::value, true>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, out, hist, B, C,
                                                                                  sparse_C, H, W, n_iter, norm, ws, st, pin);
    });
}

int kxk_assemble_backward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* conf, const int* steps, int T,
                              const float* hist, const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int D,
                              int n_iter, int norm, void* ws, hipStream_t st) {
    return with_pinned_instance(dtype, K, D, [&](auto gt, auto k, auto d) {
        using GT = typename decltype(gt)::type;
        return assemble_backward<decltype(k)::value, GT, decltype(d)::value, true>((const store_t<GT>*)guid, blur, sparse, conf, steps, T, hist, gout,
                                                                                   (store_t<GT>*)gg, gx, gc, B, C, sparse_C, H, W, n_iter, norm, ws, st, pin);
    });
}

}  // namespace cspn
