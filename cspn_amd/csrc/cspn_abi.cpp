// cspn_abi.cpp -- extern "C" entry points declared in include/cspn_amd.h.
// Replaces the call boundary of Affinity_Propagate.forward
// (reference cspn_pytorch/models/cspn.py:42-83) and of the chained
// fluid.layers.affinity_propagate calls (reference cspn_paddle/demo.py:41-52).
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <utility>

#include "cspn_common.h"
#include "cspn_gate16.h"

namespace cspn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

int num_cus() {
    static std::atomic<int> cache[64];
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev >= 0 && dev < 64) {
        v = cache[dev].load(std::memory_order_relaxed);
        if (v > 0) return v;
    }
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
    if (dev >= 0 && dev < 64) cache[dev].store(v, std::memory_order_relaxed);
    return v;
}

static int check_common(const void* a, const void* b, const void* out, int n_iter, int norm, const void* ws,
                        size_t ws_bytes, size_t need, int norm_max = CSPN_NORM_NONE) {
    if (!a || !b || !out) { set_error("null tensor pointer"); return CSPN_E_BADARG; }
    if (n_iter < 0) { set_error("n_iter must be >= 0 (got %d)", n_iter); return CSPN_E_BADARG; }
    if (norm < CSPN_NORM_8SUM || norm > CSPN_NORM_PRENORM) { set_error("unknown norm_type %d", norm); return CSPN_E_BADARG; }
    if (norm > norm_max) { set_error("norm_type CSPN_NORM_PRENORM is taken by the 2D entry points only"); return CSPN_E_UNSUPPORTED; }
    if (need && (!ws || ws_bytes < need)) {
        set_error("workspace too small: need %zu bytes, got %zu", need, ws_bytes);
        return CSPN_E_WORKSPACE;
    }
    if (need && ((uintptr_t)ws & 255u)) { set_error("workspace must be 256-byte aligned"); return CSPN_E_WORKSPACE; }
    return 0;
}

// ---- the 3 x 3 entry points (cspn2d_* / cspn3d_*): the pieces their checks share ----
// every dimension positive, the first (B) at least b_min; names: one letter per dimension for the text, "BHW" .. "BCDHW"
static int check_shape(const char* names, std::initializer_list<int> dims, int b_min = 0) {
    int i = 0, bad = 0;
    for (int d : dims) bad |= d < (i++ ? 1 : b_min);
    if (!bad) return 0;
    char text[128] = "bad shape";
    size_t n = 9;
    for (int d : dims) n += snprintf(text + n, sizeof(text) - n, " %c=%d", *names++, d);
    set_error("%s", text);
    return CSPN_E_BADARG;
}

// elems values behind one 32-bit index that also counts `planes` planes of them
static int check_index32(long long elems, int planes, const char* what = "") {
    if (elems <= 0x7fffffffLL / planes) return 0;
    set_error("tensor too large for 32-bit plane indexing%s", what);
    return CSPN_E_UNSUPPORTED;
}

// n_iter == 0, forward: the loop body never runs (reference cspn.py:61,66,83)
static int identity_copy(float* out, const float* in, size_t floats, hipStream_t st) {
    hipError_t e = hipMemcpyAsync(out, in, sizeof(float) * floats, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) { set_error("hipMemcpyAsync: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

// n_iter == 0, backward: dL/dfeat = dL/dout, the gates are not used
static int identity_backward(float* grad_feat, const float* grad_out, size_t floats, void* grad_gate, size_t gate_bytes, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (grad_feat) e = hipMemcpyAsync(grad_feat, grad_out, sizeof(float) * floats, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && grad_gate) e = hipMemsetAsync(grad_gate, 0, gate_bytes, st);
    if (e != hipSuccess) { set_error("hipMemcpyAsync / hipMemsetAsync: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

// argument checks of the gate normaliser entry points (cspn_gate_absnorm_f32 / _backward_f32)
static bool overlaps(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

// gsize: bytes of an element of guide (and, in the backward, of out = grad_guide): 4, or 2 for the *_g16 forms
static int absnorm_check(const char* what, const void* guide, const float* a, const void* out, int N, int K, size_t V, size_t gsize = 4, bool out_is_guide_type = false) {
    if (!guide || !a || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (N <= 0 || V == 0) { set_error("%s: bad shape N=%d V=%zu", what, N, V); return CSPN_E_BADARG; }
    if (K != 8 && K != 26 && K != 24 && K != 48) {
        set_error("%s: K must be 8 (2D), 26 (3D), 24 or 48 (2D 5 x 5 / 7 x 7), got %d", what, K);
        return CSPN_E_BADARG;
    }
    if ((size_t)N * V > ((size_t)1 << 39)) { set_error("%s: N * V = %zu voxels is beyond the launch grid", what, (size_t)N * V); return CSPN_E_UNSUPPORTED; }
    const size_t elems = (size_t)N * K * V, gbytes = gsize * elems, obytes = (out_is_guide_type ? gsize : sizeof(float)) * elems;
    const bool a_is_guide = (const void*)a == guide;   // (the forward passes guide twice)
    if (overlaps(out, obytes, guide, gbytes) || overlaps(out, obytes, a, a_is_guide ? gbytes : sizeof(float) * elems)) {
        set_error("%s: the output must not alias an input", what);
        return CSPN_E_BADARG;
    }
    return 0;
}

static size_t absnorm_planes_bytes(int B, int D, int H, int W) {   // the normalised gates of the unfused path, 256-byte multiple
    return round256(26 * sizeof(float) * (size_t)B * D * H * W);
}

// ---- the K x K entry points (cspn2d_*_kxk*) ----
static bool kxk_shape_ok(int B, int C, int H, int W, int K, int n_iter) {
    return B > 0 && C > 0 && H > 0 && W > 0 && (K == 5 || K == 7) && n_iter >= 0 && (long long)B * C * H * W <= 0x7fffffffLL &&
           (long long)B * (K * K - 1) * H * W <= 0x7fffffffLL;
}

static int kxk_check_shape(const char* what, int B, int C, int H, int W, int K, int n_iter) {
    if (K != 5 && K != 7) { set_error("%s: K must be 5 or 7, got %d", what, K); return CSPN_E_BADARG; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (n_iter < 0) { set_error("%s: n_iter must be >= 0 (got %d)", what, n_iter); return CSPN_E_BADARG; }
    if (!kxk_shape_ok(B, C, H, W, K, n_iter)) { set_error("%s: tensor too large for 32-bit element indexing", what); return CSPN_E_UNSUPPORTED; }
    return 0;
}

static size_t kxk_values_bytes(int B, int C, int H, int W) { return sizeof(float) * (size_t)B * C * H * W; }

static int kxk_check_ws(const char* what, const void* ws, size_t ws_bytes, size_t need) {
    if (need && (!ws || ws_bytes < need)) { set_error("%s: workspace too small: need %zu bytes, got %zu", what, need, ws_bytes); return CSPN_E_WORKSPACE; }
    if (need && ((uintptr_t)ws & 255u)) { set_error("%s: workspace must be 256-byte aligned", what); return CSPN_E_WORKSPACE; }
    return 0;
}

// an output range that overlaps any of the (pointer, bytes) ranges given; null pointers and empty ranges are skipped
static bool kxk_overlaps(const void* out, size_t out_bytes, std::initializer_list<std::pair<const void*, size_t>> others) {
    if (!out || !out_bytes) return false;
    for (const auto& o : others)
        if (o.first && o.second && overlaps(out, out_bytes, o.first, o.second)) return true;
    return false;
}

// the *_g16 entry points: the gate dtype, and the 16-bit tensors at even addresses
static int g16_check(const char* what, int dtype, const void* gate, const void* grad_gate) {
    if (dtype != CSPN_DTYPE_F16 && dtype != CSPN_DTYPE_BF16) {
        set_error("%s: gate_dtype must be CSPN_DTYPE_F16 (1) or CSPN_DTYPE_BF16 (2), got %d", what, dtype);
        return CSPN_E_BADARG;
    }
    if (((uintptr_t)gate & 1u) || ((uintptr_t)grad_gate & 1u)) { set_error("%s: a 16-bit tensor must be 2-byte aligned", what); return CSPN_E_BADARG; }
    return 0;
}

// the depth-completion contract over K x K (cspn2d_*_kxk_norm*): K = 3 as well, a mask of 0, 1 or C planes
static bool kxk_norm_shape_ok(int B, int C, int sparse_C, int H, int W, int K, int n_iter) {
    const long long px = (long long)H * W, N = sparse_C > 1 ? (long long)B * C : B;
    return B > 0 && C > 0 && H > 0 && W > 0 && (K == 3 || K == 5 || K == 7) && n_iter >= 0 && (sparse_C == 0 || sparse_C == 1 || sparse_C == C) &&
           (long long)B * C * px <= 0x7fffffffLL && N * (K * K - 1) * px <= 0x7fffffffLL;
}

static int kxk_norm_check(const char* what, const float* sparse, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm) {
    if (K != 3 && K != 5 && K != 7) { set_error("%s: K must be 3, 5 or 7, got %d", what, K); return CSPN_E_BADARG; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (n_iter < 0) { set_error("%s: n_iter must be >= 0 (got %d)", what, n_iter); return CSPN_E_BADARG; }
    if (norm != CSPN_NORM_8SUM && norm != CSPN_NORM_8SUM_ABS) { set_error("%s: norm must be CSPN_NORM_8SUM or CSPN_NORM_8SUM_ABS, got %d", what, norm); return CSPN_E_BADARG; }
    if ((sparse_C != 0 && sparse_C != 1 && sparse_C != C) || (sparse_C == 0) != (sparse == nullptr)) {
        set_error("%s: sparse_C must be 0 (sparse NULL), 1 or C = %d (sparse given), got %d", what, C, sparse_C);
        return CSPN_E_BADARG;
    }
    if (!kxk_norm_shape_ok(B, C, sparse_C, H, W, K, n_iter)) { set_error("%s: tensor too large for 32-bit element indexing", what); return CSPN_E_UNSUPPORTED; }
    return 0;
}

}  // namespace cspn

using namespace cspn;

extern "C" {

int cspn_abi_version(void) { return CSPN_ABI_VERSION; }
const char* cspn_last_error(void) { return g_err; }

int cspn2d_auto_algo(int B, int H, int W, int n_iter) {
    if (fused2d_supported(B, H, W, n_iter)) return CSPN_ALGO_FUSED;
    return padded2d_supported(B, H, W, n_iter) ? CSPN_ALGO_FUSED_PADDED : CSPN_ALGO_STEPWISE;
}

size_t cspn2d_workspace_bytes(int B, int H, int W, int n_iter) {
    if (B <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    size_t a = stepwise2d_workspace(B, H, W, n_iter);
    size_t b = fused2d_supported(B, H, W, n_iter) ? fused2d_workspace(B, H, W, n_iter) : 0;
    if (padded2d_supported(B, H, W, n_iter)) b = padded2d_workspace(B, H, W, n_iter);
    return a > b ? a : b;  // large enough for either algo so callers can A/B
}

int cspn2d_forward_f32_algo(const float* guidance, const float* blur, const float* sparse, float* out, int B,
                            int H, int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes,
                            cspn_stream_t stream) {
    if (int e = check_shape("BHW", {B, H, W})) return e;
    if (B == 0) return 0;
    if (int e = check_index32((long long)B * H * W, 9)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (algo == CSPN_ALGO_AUTO) {
        algo = cspn2d_auto_algo(B, H, W, n_iter);
        if (algo == CSPN_ALGO_FUSED && ((uintptr_t)out & 15u) != 0) algo = CSPN_ALGO_STEPWISE;   // (the fused kernels store aligned float4)
        // the padded path runs the fused kernels on planes inside the caller's workspace: those need the same alignment
        if (algo == CSPN_ALGO_FUSED_PADDED && ((uintptr_t)ws & 15u) != 0) algo = CSPN_ALGO_STEPWISE;
    }
    if (algo == CSPN_ALGO_FUSED_PADDED && n_iter == 0) algo = CSPN_ALGO_STEPWISE;   // n_iter == 0 is the identity copy below whatever the algo (reference cspn.py:61,66,83)
    if (algo == CSPN_ALGO_FUSED_PADDED) {
        if (!padded2d_supported(B, H, W, n_iter)) { set_error("FUSED_PADDED needs W %% 4 != 0 and a shape the fused kernels take (B=%d H=%d W=%d n_iter=%d)", B, H, W, n_iter); return CSPN_E_UNSUPPORTED; }
        if (((uintptr_t)ws & 15u) != 0) { set_error("FUSED_PADDED needs a 16-byte aligned workspace (its padded planes live there)"); return CSPN_E_UNSUPPORTED; }
        if (int e = check_common(guidance, blur, out, n_iter, norm_type, ws, ws_bytes, padded2d_workspace(B, H, W, n_iter), CSPN_NORM_PRENORM)) return e;
        return padded2d_forward(guidance, blur, sparse, out, B, H, W, n_iter, norm_type, ws, st);
    }
    if (algo != CSPN_ALGO_STEPWISE && algo != CSPN_ALGO_FUSED && algo != CSPN_ALGO_FUSED_CXX) { set_error("unknown algo %d", algo); return CSPN_E_BADARG; }
    const bool fused = algo == CSPN_ALGO_FUSED || algo == CSPN_ALGO_FUSED_CXX;
    if (fused && !fused2d_supported(B, H, W, n_iter)) {
        set_error("fused kernel does not support B=%d H=%d W=%d n_iter=%d", B, H, W, n_iter);
        return CSPN_E_UNSUPPORTED;
    }
    size_t need = n_iter == 0 ? 0
                  : (fused ? fused2d_workspace(B, H, W, n_iter)
                                             : stepwise2d_workspace(B, H, W, n_iter));
    if (int e = check_common(guidance, blur, out, n_iter, norm_type, ws, ws_bytes, need, CSPN_NORM_PRENORM)) return e;
    if (n_iter == 0) return identity_copy(out, blur, (size_t)B * H * W, st);
    if (fused) return fused2d_forward(guidance, blur, sparse, out, B, H, W, n_iter, norm_type, ws, st, algo == CSPN_ALGO_FUSED);
    return stepwise2d_forward(guidance, blur, sparse, out, B, H, W, n_iter, norm_type, ws, st);
}

int cspn2d_forward_f32(const float* guidance, const float* blur, const float* sparse, float* out, int B, int H,
                       int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return cspn2d_forward_f32_algo(guidance, blur, sparse, out, B, H, W, n_iter, norm_type, CSPN_ALGO_AUTO, ws,
                                   ws_bytes, stream);
}

// ---- SURVEY 8f-2, second alternative: the normalisation done by the producer of the guidance (include/cspn_amd.h) ----
int cspn2d_normalize_f32(const float* guidance, float* wb, int B, int H, int W, int norm_type, cspn_stream_t stream) {
    if (!guidance || !wb || B <= 0 || H <= 0 || W <= 0) { set_error("bad argument"); return CSPN_E_BADARG; }
    if (norm_type != CSPN_NORM_8SUM && norm_type != CSPN_NORM_8SUM_ABS) { set_error("cspn2d_normalize_f32: norm_type must be 8SUM or 8SUM_ABS (got %d)", norm_type); return CSPN_E_BADARG; }
    if (int e = check_index32((long long)B * H * W, 9)) return e;
    return normalize2d(guidance, wb, B, H, W, norm_type, (hipStream_t)stream);
}

int cspn2d_normalize_backward_f32(const float* guidance, const float* grad_wb, float* grad_guidance, int B, int H, int W, int norm_type,
                                  cspn_stream_t stream) {
    if (!guidance || !grad_wb || !grad_guidance) { set_error("cspn2d_normalize_backward_f32: null pointer"); return CSPN_E_BADARG; }
    if (B <= 0 || H <= 0 || W <= 0) { set_error("cspn2d_normalize_backward_f32: bad shape B=%d H=%d W=%d", B, H, W); return CSPN_E_BADARG; }
    if (norm_type != CSPN_NORM_8SUM && norm_type != CSPN_NORM_8SUM_ABS) { set_error("cspn2d_normalize_backward_f32: norm_type must be 8SUM or 8SUM_ABS (got %d)", norm_type); return CSPN_E_BADARG; }
    if (grad_guidance == guidance || grad_guidance == grad_wb) { set_error("cspn2d_normalize_backward_f32: grad_guidance must not alias an input"); return CSPN_E_BADARG; }
    if (int e = check_index32((long long)B * H * W, 9)) return e;
    return normalize2d_backward(guidance, grad_wb, grad_guidance, B, H, W, norm_type, (hipStream_t)stream);
}

int cspn2d_forward_prenorm_f32(const float* wb, const float* blur, const float* sparse, float* out, int B, int H, int W, int n_iter,
                               void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return cspn2d_forward_f32_algo(wb, blur, sparse, out, B, H, W, n_iter, CSPN_NORM_PRENORM, CSPN_ALGO_AUTO, ws, ws_bytes, stream);
}

size_t cspn2d_backward_workspace_bytes(int B, int H, int W, int n_iter) {
    if (B <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return backward2d_workspace(B, H, W, n_iter);
}

int cspn2d_backward_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                        float* grad_guidance, float* grad_blur, int B, int H, int W, int n_iter, int norm_type, void* ws,
                        size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BHW", {B, H, W})) return e;
    if (B == 0) return 0;
    if (n_iter < 1) { set_error("backward needs n_iter >= 1 (got %d)", n_iter); return CSPN_E_BADARG; }
    if (int e = check_index32((long long)B * H * W, 9)) return e;
    if (!grad_out) { set_error("null grad_out"); return CSPN_E_BADARG; }
    if (int e = check_common(guidance, blur, grad_out, n_iter, norm_type, ws, ws_bytes, backward2d_workspace(B, H, W, n_iter), CSPN_NORM_PRENORM)) return e;
    if (!grad_guidance && !grad_blur) return 0;
    return backward2d(guidance, blur, sparse, grad_out, grad_guidance, grad_blur, B, H, W, n_iter, norm_type, ws, (hipStream_t)stream);
}

size_t cspn2d_history_bytes(int B, int H, int W, int n_iter) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return history2d_bytes(B, H, W, n_iter);
}

int cspn2d_forward_history_f32(const float* guidance, const float* blur, const float* sparse, float* out, void* history,
                               size_t history_bytes, int B, int H, int W, int n_iter, int norm_type, void* ws, size_t ws_bytes,
                               cspn_stream_t stream) {
    if (int e = check_shape("BHW", {B, H, W}, 1)) return e;
    const size_t hb = history2d_bytes(B, H, W, n_iter);
    if (hb == 0) { set_error("no history mode for B=%d H=%d W=%d n_iter=%d", B, H, W, n_iter); return CSPN_E_UNSUPPORTED; }
    if (!history || history_bytes < hb || ((uintptr_t)history & 255u)) { set_error("history buffer too small or misaligned: need %zu bytes", hb); return CSPN_E_WORKSPACE; }
    if (int e = check_common(guidance, blur, out, n_iter, norm_type, ws, ws_bytes, fused2d_workspace(B, H, W, n_iter), CSPN_NORM_PRENORM)) return e;
    if (((uintptr_t)out & 15u) != 0) { set_error("output must be 16-byte aligned"); return CSPN_E_UNSUPPORTED; }
    return forward2d_history(guidance, blur, sparse, out, history, B, H, W, n_iter, norm_type, ws, (hipStream_t)stream);
}

size_t cspn2d_backward_history_workspace_bytes(int B, int H, int W, int n_iter) {
    if (B <= 0 || H <= 0 || W <= 0 || history2d_bytes(B, H, W, n_iter) == 0) return 0;
    return backward2d_history_workspace(B, H, W);
}

int cspn2d_backward_history_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                                const void* history, size_t history_bytes, float* grad_guidance, float* grad_blur, int B, int H,
                                int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BHW", {B, H, W}, 1)) return e;
    const size_t hb = history2d_bytes(B, H, W, n_iter);
    if (hb == 0) { set_error("no history mode for B=%d H=%d W=%d n_iter=%d", B, H, W, n_iter); return CSPN_E_UNSUPPORTED; }
    if (!grad_out) { set_error("null grad_out"); return CSPN_E_BADARG; }
    if (!history || history_bytes < hb) { set_error("history buffer too small: need %zu bytes", hb); return CSPN_E_WORKSPACE; }
    if (int e = check_common(guidance, blur, grad_out, n_iter, norm_type, ws, ws_bytes, backward2d_history_workspace(B, H, W), CSPN_NORM_PRENORM)) return e;
    if (!grad_guidance && !grad_blur) return 0;
    return backward2d_history(guidance, blur, sparse, grad_out, history, grad_guidance, grad_blur, B, H, W, n_iter, norm_type, ws,
                              (hipStream_t)stream);
}

// ---- C channels on shared 2D guidance (include/cspn_amd.h: the cspn2d_*_multi entry points) ----

static int check_multi(int B, int C, int sparse_channels, const float* sparse, int H, int W) {
    if (int e = check_shape("BCHW", {B, C, H, W})) return e;
    if (sparse && sparse_channels != 1 && sparse_channels != C) {
        set_error("sparse has %d channels: 1 (one mask for every channel) or C = %d expected", sparse_channels, C);
        return CSPN_E_BADARG;
    }
    return check_index32((long long)B * C * H * W, 9, " (B*C*H*W)");
}

// the shared-gate forward: one ring launch per pass over the B*C image-channels (the fused assembly path of the single-channel call)
static bool multi_fast(int B, int C, int H, int W, int n_iter) { return B > 0 && n_iter > 0 && fused2d_supported(B * C, H, W, n_iter) && tsw2d_supported(B * C, H, W); }

// the per-channel loop of the fallbacks: channel c of a [B][C][HW] tensor <-> a [B][HW] plane
static hipError_t gather_channel(float* dst, const float* src, int B, int C, int c, size_t HW, hipStream_t st) {
    return hipMemcpy2DAsync(dst, HW * sizeof(float), src + (size_t)c * HW, (size_t)C * HW * sizeof(float), HW * sizeof(float), B,
                            hipMemcpyDeviceToDevice, st);
}
static hipError_t scatter_channel(float* dst, const float* src, int B, int C, int c, size_t HW, hipStream_t st) {
    return hipMemcpy2DAsync(dst + (size_t)c * HW, (size_t)C * HW * sizeof(float), src, HW * sizeof(float), HW * sizeof(float), B,
                            hipMemcpyDeviceToDevice, st);
}
#define MULTI_COPY(call)                                                                                  \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) { set_error("hipMemcpy2DAsync: %s", hipGetErrorString(e_)); return (int)e_; } \
    } while (0)

// a shared mask widened to [B][C][HW] at the front of the workspace (the fast paths)
static size_t widened_bytes(int B, int C, int H, int W) { return round256(sizeof(float) * (size_t)B * C * H * W); }

static int widen_if_shared(const float*& sparse, int sparse_channels, int B, int C, int H, int W, void* ws, hipStream_t st) {
    if (!sparse || sparse_channels == C) return 0;
    if (int e = widen_channels(sparse, (float*)ws, B, C, (size_t)H * W, st)) return e;
    sparse = (const float*)ws;
    return 0;
}

int cspn2d_multi_supported(int B, int C, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)B * C * H * W > 0x7fffffffLL / 9) return 0;
    return multi_fast(B, C, H, W, n_iter) ? 1 : 0;
}

size_t cspn2d_workspace_bytes_multi(int B, int C, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    if (C == 1) return cspn2d_workspace_bytes(B, H, W, n_iter);
    const size_t plane = round256(sizeof(float) * (size_t)B * H * W);
    const size_t loop = 3 * plane + round256(cspn2d_workspace_bytes(B, H, W, n_iter));   // blur, mask and out of one channel + its call's workspace
    const size_t fast = multi_fast(B, C, H, W, n_iter) ? widened_bytes(B, C, H, W) + fused2d_workspace(B * C, H, W, n_iter) : 0;
    return loop > fast ? loop : fast;
}

int cspn2d_forward_multi_f32(const float* guidance, const float* blur, const float* sparse, float* out, int B, int C, int sparse_channels,
                             int H, int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_multi(B, C, sparse_channels, sparse, H, W)) return e;
    if (C == 1) return cspn2d_forward_f32_algo(guidance, blur, sparse, out, B, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
    if (B == 0) return 0;
    if (algo < CSPN_ALGO_AUTO || algo > CSPN_ALGO_FUSED_PADDED) { set_error("unknown algo %d", algo); return CSPN_E_BADARG; }
    if (int e = check_common(guidance, blur, out, n_iter, norm_type, ws, ws_bytes, n_iter == 0 ? 0 : cspn2d_workspace_bytes_multi(B, C, H, W, n_iter),
                             CSPN_NORM_PRENORM)) return e;
    hipStream_t st = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    if (n_iter == 0) return identity_copy(out, blur, (size_t)B * C * HW, st);
    // the fast path where the single-channel call would take the assembly ring too (AUTO / FUSED, 16-byte aligned output)
    if ((algo == CSPN_ALGO_AUTO || algo == CSPN_ALGO_FUSED) && multi_fast(B, C, H, W, n_iter) && ((uintptr_t)out & 15u) == 0) {
        if (int e = widen_if_shared(sparse, sparse_channels, B, C, H, W, ws, st)) return e;
        return fused2d_forward(guidance, blur, sparse, out, B * C, H, W, n_iter, norm_type, (char*)ws + widened_bytes(B, C, H, W), st, true, 0, C);
    }
    // everything else: channel by channel through the single-channel entry point
    const size_t plane = round256(sizeof(float) * (size_t)B * HW);
    float* blur_c = (float*)ws;
    float* sp_c = (float*)((char*)ws + plane);
    float* out_c = (float*)((char*)ws + 2 * plane);
    void* ws_c = (char*)ws + 3 * plane;
    const size_t ws_c_bytes = cspn2d_workspace_bytes(B, H, W, n_iter);
    for (int c = 0; c < C; ++c) {
        MULTI_COPY(gather_channel(blur_c, blur, B, C, c, HW, st));
        const float* sp = sparse;
        if (sparse && sparse_channels == C) { MULTI_COPY(gather_channel(sp_c, sparse, B, C, c, HW, st)); sp = sp_c; }
        if (int e = cspn2d_forward_f32_algo(guidance, blur_c, sp, out_c, B, H, W, n_iter, norm_type, algo, ws_c, ws_c_bytes, stream)) return e;
        MULTI_COPY(scatter_channel(out, out_c, B, C, c, HW, st));
    }
    return 0;
}

size_t cspn2d_history_bytes_multi(int B, int C, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long long)B * C * H * W > 0x7fffffffLL / 9) return 0;
    if (C == 1) return cspn2d_history_bytes(B, H, W, n_iter);
    return multi_fast(B, C, H, W, n_iter) ? history2d_bytes(B * C, H, W, n_iter) : 0;
}

int cspn2d_forward_history_multi_f32(const float* guidance, const float* blur, const float* sparse, float* out, void* history,
                                     size_t history_bytes, int B, int C, int sparse_channels, int H, int W, int n_iter, int norm_type,
                                     void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_multi(B, C, sparse_channels, sparse, H, W)) return e;
    if (C == 1) return cspn2d_forward_history_f32(guidance, blur, sparse, out, history, history_bytes, B, H, W, n_iter, norm_type, ws, ws_bytes, stream);
    if (B == 0) { set_error("bad shape B=0"); return CSPN_E_BADARG; }
    const size_t hb = cspn2d_history_bytes_multi(B, C, H, W, n_iter);
    if (hb == 0) { set_error("no history mode for B=%d C=%d H=%d W=%d n_iter=%d", B, C, H, W, n_iter); return CSPN_E_UNSUPPORTED; }
    if (!history || history_bytes < hb || ((uintptr_t)history & 255u)) { set_error("history buffer too small or misaligned: need %zu bytes", hb); return CSPN_E_WORKSPACE; }
    if (int e = check_common(guidance, blur, out, n_iter, norm_type, ws, ws_bytes, cspn2d_workspace_bytes_multi(B, C, H, W, n_iter), CSPN_NORM_PRENORM)) return e;
    if (((uintptr_t)out & 15u) != 0) { set_error("output must be 16-byte aligned"); return CSPN_E_UNSUPPORTED; }
    hipStream_t st = (hipStream_t)stream;
    if (int e = widen_if_shared(sparse, sparse_channels, B, C, H, W, ws, st)) return e;
    return forward2d_history(guidance, blur, sparse, out, history, B * C, H, W, n_iter, norm_type, nullptr, st, C);
}

size_t cspn2d_backward_multi_workspace_bytes(int B, int C, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    if (C == 1) return cspn2d_backward_workspace_bytes(B, H, W, n_iter);
    if (backward2d_multi_supported(B * C, H, W, n_iter)) return widened_bytes(B, C, H, W) + backward2d_workspace(B * C, H, W, n_iter);
    const size_t plane = round256(sizeof(float) * (size_t)B * H * W);
    return 4 * plane + 8 * plane + round256(backward2d_workspace(B, H, W, n_iter));   // blur, mask, grad_out, grad_blur of one channel; its grad_guidance
}

int cspn2d_backward_multi_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out, float* grad_guidance,
                              float* grad_blur, int B, int C, int sparse_channels, int H, int W, int n_iter, int norm_type,
                              void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_multi(B, C, sparse_channels, sparse, H, W)) return e;
    if (C == 1) return cspn2d_backward_f32(guidance, blur, sparse, grad_out, grad_guidance, grad_blur, B, H, W, n_iter, norm_type, ws, ws_bytes, stream);
    if (B == 0) return 0;
    if (n_iter < 1) { set_error("backward needs n_iter >= 1 (got %d)", n_iter); return CSPN_E_BADARG; }
    if (!grad_out) { set_error("null grad_out"); return CSPN_E_BADARG; }
    if (int e = check_common(guidance, blur, grad_out, n_iter, norm_type, ws, ws_bytes, cspn2d_backward_multi_workspace_bytes(B, C, H, W, n_iter),
                             CSPN_NORM_PRENORM)) return e;
    if (!grad_guidance && !grad_blur) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t HW = (size_t)H * W;
    if (backward2d_multi_supported(B * C, H, W, n_iter)) {
        if (int e = widen_if_shared(sparse, sparse_channels, B, C, H, W, ws, st)) return e;
        return backward2d(guidance, blur, sparse, grad_out, grad_guidance, grad_blur, B * C, H, W, n_iter, norm_type,
                          (char*)ws + widened_bytes(B, C, H, W), st, C);
    }
    const size_t plane = round256(sizeof(float) * (size_t)B * HW);
    float* blur_c = (float*)ws;
    float* sp_c = (float*)((char*)ws + plane);
    float* go_c = (float*)((char*)ws + 2 * plane);
    float* gb_c = (float*)((char*)ws + 3 * plane);
    float* gg_c = (float*)((char*)ws + 4 * plane);
    void* ws_c = (char*)ws + 12 * plane;
    const size_t ws_c_bytes = backward2d_workspace(B, H, W, n_iter);
    for (int c = 0; c < C; ++c) {
        MULTI_COPY(gather_channel(blur_c, blur, B, C, c, HW, st));
        MULTI_COPY(gather_channel(go_c, grad_out, B, C, c, HW, st));
        const float* sp = sparse;
        if (sparse && sparse_channels == C) { MULTI_COPY(gather_channel(sp_c, sparse, B, C, c, HW, st)); sp = sp_c; }
        float* gg = grad_guidance ? (c == 0 ? grad_guidance : gg_c) : nullptr;
        if (int e = cspn2d_backward_f32(guidance, blur_c, sp, go_c, gg, grad_blur ? gb_c : nullptr, B, H, W, n_iter, norm_type, ws_c, ws_c_bytes,
                                        stream)) return e;
        if (grad_guidance && c > 0)
            if (int e = add_inplace(grad_guidance, gg_c, 8 * (size_t)B * HW, st)) return e;
        if (grad_blur) MULTI_COPY(scatter_channel(grad_blur, gb_c, B, C, c, HW, st));
    }
    return 0;
}

size_t cspn2d_backward_history_multi_workspace_bytes(int B, int C, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
    if (C == 1) return cspn2d_backward_history_workspace_bytes(B, H, W, n_iter);
    if (cspn2d_history_bytes_multi(B, C, H, W, n_iter) == 0) return 0;
    return widened_bytes(B, C, H, W) + backward2d_history_workspace(B * C, H, W);
}

int cspn2d_backward_history_multi_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                                      const void* history, size_t history_bytes, float* grad_guidance, float* grad_blur, int B, int C,
                                      int sparse_channels, int H, int W, int n_iter, int norm_type, void* ws, size_t ws_bytes,
                                      cspn_stream_t stream) {
    if (int e = check_multi(B, C, sparse_channels, sparse, H, W)) return e;
    if (C == 1) return cspn2d_backward_history_f32(guidance, blur, sparse, grad_out, history, history_bytes, grad_guidance, grad_blur, B, H, W,
                                                   n_iter, norm_type, ws, ws_bytes, stream);
    if (B == 0) { set_error("bad shape B=0"); return CSPN_E_BADARG; }
    const size_t hb = cspn2d_history_bytes_multi(B, C, H, W, n_iter);
    if (hb == 0) { set_error("no history mode for B=%d C=%d H=%d W=%d n_iter=%d", B, C, H, W, n_iter); return CSPN_E_UNSUPPORTED; }
    if (!grad_out) { set_error("null grad_out"); return CSPN_E_BADARG; }
    if (!history || history_bytes < hb) { set_error("history buffer too small: need %zu bytes", hb); return CSPN_E_WORKSPACE; }
    if (int e = check_common(guidance, blur, grad_out, n_iter, norm_type, ws, ws_bytes, cspn2d_backward_history_multi_workspace_bytes(B, C, H, W, n_iter),
                             CSPN_NORM_PRENORM)) return e;
    if (!grad_guidance && !grad_blur) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (int e = widen_if_shared(sparse, sparse_channels, B, C, H, W, ws, st)) return e;
    return backward2d_history(guidance, blur, sparse, grad_out, history, grad_guidance, grad_blur, B * C, H, W, n_iter, norm_type,
                              (char*)ws + widened_bytes(B, C, H, W), st, C);
}

// a persistent 3D launch of an EARLIER call gave up (cspn3d_persistent.hip): report it once, through whichever 3D call comes next
static int async_failure_of_earlier_call() {
    if (persistent3d_take_status() == 0) return 0;
    set_error("an earlier cspn3d call's persistent kernel gave up waiting for a neighbouring workgroup (not all of its workgroups were "
              "resident: the device is shared with other work that holds compute units); that call's outputs are NaN-filled / invalid. "
              "Re-run it, or request CSPN_ALGO3D_STEPWISE");
    return CSPN_E_ASYNC;
}

int cspn3d_check_status(cspn_stream_t stream) {
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) { set_error("hipStreamSynchronize: %s", hipGetErrorString(e)); return (int)e; }
    return async_failure_of_earlier_call();
}

size_t cspn3d_workspace_bytes(int B, int D, int H, int W, int n_iter) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return stepwise3d_workspace(B, D, H, W, n_iter);
}

size_t cspn3d_workspace_bytes_ex(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return forward3d_workspace(B, D, H, W, n_iter, norm_type, has_sparse != 0);
}

int cspn3d_forward_f32(const float* gate, const float* feat, const float* sparse, float* out, int B, int D, int H,
                       int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return cspn3d_forward_f32_algo(gate, feat, sparse, out, B, D, H, W, n_iter, norm_type, CSPN_ALGO3D_AUTO, ws, ws_bytes, stream);
}

// the checks of cspn3d_forward_f32_algo (gdt 0) and cspn3d_forward_g16_algo, then the engine
static int forward3d_entry(const void* gate, int gdt, const float* feat, const float* sparse, float* out, int B, int D, int H,
                           int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BDHW", {B, D, H, W})) return e;
    if (B == 0) return 0;
    if (int e = check_index32((long long)B * D * H * W, 27)) return e;
    hipStream_t st = (hipStream_t)stream;
    if (algo < CSPN_ALGO3D_AUTO || algo > CSPN_ALGO3D_PERSISTENT) { set_error("unknown 3D algo %d", algo); return CSPN_E_BADARG; }
    if (int e = async_failure_of_earlier_call()) return e;
    // misaligned tensors cannot take the 16-byte paths: they fold like the normalising modes (cspn3d_workspace_bytes()); a 16-bit gate
    // tensor is aligned at 8 bytes (four gates)
    const bool aligned = quads_ok(W, gdt, {gate}, {feat, out, ws});   // (W % 4 != 0 takes the folding path's size from either query)
    size_t need = n_iter == 0 ? 0 : (aligned ? forward3d_workspace(B, D, H, W, n_iter, norm_type, sparse != nullptr)
                                             : stepwise3d_workspace(B, D, H, W, n_iter));
    if (int e = check_common(gate, feat, out, n_iter, norm_type, ws, ws_bytes, need)) return e;
    if (n_iter == 0) return identity_copy(out, feat, (size_t)B * D * H * W, st);
    return stepwise3d_forward(gate, feat, sparse, out, B, D, H, W, n_iter, norm_type, ws, st, algo, gdt);
}

int cspn3d_forward_f32_algo(const float* gate, const float* feat, const float* sparse, float* out, int B, int D, int H,
                            int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return forward3d_entry(gate, 0, feat, sparse, out, B, D, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
}

int cspn3d_forward_g16_algo(const void* gate, int gate_dtype, const float* feat, const float* sparse, float* out, int B, int D, int H,
                            int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_forward_g16_algo", gate_dtype, gate, nullptr)) return e;
    if (norm_type != CSPN_NORM_NONE || sparse) {
        set_error("cspn3d_forward_g16_algo: 16-bit gates cover the Paddle contract only (norm_type CSPN_NORM_NONE, sparse NULL)");
        return CSPN_E_BADARG;
    }
    return forward3d_entry(gate, gate_dtype, feat, sparse, out, B, D, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
}

// every mode on 16-bit guidance: the normalising and masked ones fold through fold3d_kernel<GT> (cspn3d_forward_g16_algo keeps its refusal)
int cspn3d_forward_norm_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, float* out, int B, int D, int H,
                            int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_forward_norm_g16", gate_dtype, guidance, nullptr)) return e;
    return forward3d_entry(guidance, gate_dtype, feat, sparse, out, B, D, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
}

int cspn3d_multi_supported(int B, int C, int D, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return persistent3d_multi_supported(B, C, D, H, W, n_iter) ? 1 : 0;
}

static int forward3d_multi_entry(const void* gate, int gdt, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                                 void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BCDHW", {B, C, D, H, W})) return e;
    if (B == 0) return 0;
    if (int e = async_failure_of_earlier_call()) return e;
    if (int e = check_common(gate, feat, out, n_iter, CSPN_NORM_NONE, ws, ws_bytes,
                             n_iter == 0 ? 0 : forward3d_workspace(B, D, H, W, n_iter, CSPN_NORM_NONE, false))) return e;
    const bool aligned = quads_ok(W, gdt, {gate}, {feat, out, ws});
    if (!aligned || !persistent3d_multi_supported(B, C, D, H, W, n_iter)) {
        set_error("cspn3d_forward_multi_f32 runs the persistent kernel only (W %% 4 == 0, 2 <= n_iter <= 60, 16-byte aligned tensors, "
                  "volume resident on the device): loop over the channels with cspn3d_forward_f32 for B=%d C=%d D=%d H=%d W=%d n_iter=%d",
                  B, C, D, H, W, n_iter);
        return CSPN_E_UNSUPPORTED;
    }
    return persistent3d_forward_multi(gate, feat, out, B, C, D, H, W, n_iter, ws, (hipStream_t)stream, gdt);
}

int cspn3d_forward_multi_f32(const float* gate, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                             void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return forward3d_multi_entry(gate, 0, feat, out, B, C, D, H, W, n_iter, ws, ws_bytes, stream);
}

int cspn3d_forward_multi_g16(const void* gate, int gate_dtype, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                             void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_forward_multi_g16", gate_dtype, gate, nullptr)) return e;
    return forward3d_multi_entry(gate, gate_dtype, feat, out, B, C, D, H, W, n_iter, ws, ws_bytes, stream);
}

size_t cspn3d_backward_workspace_bytes(int B, int D, int H, int W, int n_iter) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return backward3d_workspace(B, D, H, W, n_iter);
}

// the checks of cspn3d_backward_f32 (multi false, C = 1) and cspn3d_backward_multi_f32 (norm_type NONE), then the engine
// gdt: the type of gate and grad_gate (0: float32)
static int backward3d_entry(bool multi, const void* gate, int gdt, const float* feat, const float* grad_out, void* grad_gate, float* grad_feat, int B, int C,
                            int D, int H, int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = multi ? check_shape("BCDHW", {B, C, D, H, W}) : check_shape("BDHW", {B, D, H, W})) return e;
    if (B == 0) return 0;
    const size_t V = (size_t)B * D * H * W;
    if (int e = check_index32((long long)V, 27)) return e;
    if (int e = check_index32((long long)V * C, 2)) return e;
    if (norm_type != CSPN_NORM_NONE) { set_error("the 3D backward covers the Paddle contract only (norm_type NONE: gates used as given, no mask)"); return CSPN_E_UNSUPPORTED; }
    if (int e = async_failure_of_earlier_call()) return e;
    if (int e = check_common(gate, feat, grad_out, n_iter, norm_type, ws, ws_bytes, n_iter == 0 ? 0 : backward3d_workspace(B, D, H, W, n_iter, C, gdt))) return e;
    if (!grad_gate && !grad_feat) return 0;
    if (n_iter == 0) return identity_backward(grad_feat, grad_out, V * C, grad_gate, 26 * V * gate_bytes(gdt), (hipStream_t)stream);
    return backward3d(gate, feat, grad_out, grad_gate, grad_feat, B, D, H, W, n_iter, ws, (hipStream_t)stream, false, C, gdt);
}

int cspn3d_backward_f32(const float* gate, const float* feat, const float* grad_out, float* grad_gate, float* grad_feat, int B,
                        int D, int H, int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return backward3d_entry(false, gate, 0, feat, grad_out, grad_gate, grad_feat, B, 1, D, H, W, n_iter, norm_type, ws, ws_bytes, stream);
}

// the normalising / masked modes (cspn3d_norm_backward.hip); NONE without a mask is cspn3d_backward_f32 / cspn3d_backward_g16.  gdt: the type
// of guidance and grad_guidance (0: float32).  Everything in the workspace is float32, so the normalising and masked modes need the same
// bytes for every type; the Paddle contract on 16-bit gates keeps backward3d()'s widened copy for the transposed sweep
static size_t backward3d_norm_need(int B, int D, int H, int W, int n_iter, int norm_type, bool has_sparse, int gdt) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    if (norm_type < CSPN_NORM_8SUM || norm_type > CSPN_NORM_NONE) return 0;
    if (norm_type == CSPN_NORM_NONE && !has_sparse) return backward3d_workspace(B, D, H, W, n_iter, 1, gdt);
    return backward3d_norm_workspace(B, D, H, W, n_iter);
}

size_t cspn3d_backward_norm_workspace_bytes(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse) {
    return backward3d_norm_need(B, D, H, W, n_iter, norm_type, has_sparse != 0, 0);
}

// the checks of cspn3d_backward_norm_f32 (gdt 0) and cspn3d_backward_norm_g16, then the engine
static int backward3d_norm_entry(const char* what, const void* guidance, int gdt, const float* feat, const float* sparse, const float* grad_out,
                                 void* grad_guidance, float* grad_feat, int B, int D, int H, int W, int n_iter, int norm_type, int algo, void* ws,
                                 size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BDHW", {B, D, H, W})) return e;
    if (B == 0) return 0;
    const size_t V = (size_t)B * D * H * W;
    if (int e = check_index32((long long)V, 27)) return e;
    if (algo < CSPN_ALGO3D_AUTO || algo > CSPN_ALGO3D_PERSISTENT) { set_error("unknown 3D algo %d", algo); return CSPN_E_BADARG; }
    if (norm_type < CSPN_NORM_8SUM || norm_type > CSPN_NORM_NONE) {
        set_error("%s: norm_type must be CSPN_NORM_8SUM, CSPN_NORM_8SUM_ABS or CSPN_NORM_NONE (got %d)", what, norm_type);
        return CSPN_E_BADARG;
    }
    if (int e = async_failure_of_earlier_call()) return e;
    const size_t need = backward3d_norm_need(B, D, H, W, n_iter, norm_type, sparse != nullptr, gdt);
    if (int e = check_common(guidance, feat, grad_out, n_iter, norm_type, ws, ws_bytes, need)) return e;
    const size_t vb = sizeof(float) * V, gb = 26 * V * gate_bytes(gdt);   // (the guidance and its gradient: in elements of their type)
    if (kxk_overlaps(grad_guidance, gb, {{guidance, gb}, {feat, vb}, {sparse, vb}, {grad_out, vb}, {grad_feat, vb}, {ws, need}}) ||
        kxk_overlaps(grad_feat, vb, {{guidance, gb}, {feat, vb}, {sparse, vb}, {grad_out, vb}, {ws, need}})) {
        set_error("%s: an output must not overlap an input, the other output or the workspace", what);
        return CSPN_E_BADARG;
    }
    if (!grad_guidance && !grad_feat) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_backward(grad_feat, grad_out, V, grad_guidance, gb, st);
    if (algo == CSPN_ALGO3D_PERSISTENT &&
        !backward3d_norm_fused(guidance, gdt, feat, sparse, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter, ws)) {
        set_error("persistent 3D kernel does not take this backward (needs W %% 4 == 0, 16-byte aligned tensors, 3 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    const bool stepwise_only = algo == CSPN_ALGO3D_STEPWISE;
    if (norm_type == CSPN_NORM_NONE && !sparse)   // the Paddle contract: AUTO is cspn3d_backward_f32 / cspn3d_backward_g16
        return backward3d(guidance, feat, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter, ws, st, stepwise_only, 1, gdt);
    return backward3d_norm(guidance, gdt, feat, sparse, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter, norm_type, ws, st, stepwise_only);
}

int cspn3d_backward_norm_f32(const float* guidance, const float* feat, const float* sparse, const float* grad_out, float* grad_guidance,
                             float* grad_feat, int B, int D, int H, int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes,
                             cspn_stream_t stream) {
    return backward3d_norm_entry("cspn3d_backward_norm_f32", guidance, 0, feat, sparse, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter,
                                 norm_type, algo, ws, ws_bytes, stream);
}

size_t cspn3d_backward_norm_g16_workspace_bytes(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse) {
    return backward3d_norm_need(B, D, H, W, n_iter, norm_type, has_sparse != 0, CSPN_DTYPE_F16);
}

int cspn3d_backward_norm_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, const float* grad_out,
                             void* grad_guidance, float* grad_feat, int B, int D, int H, int W, int n_iter, int norm_type, int algo, void* ws,
                             size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_backward_norm_g16", gate_dtype, guidance, grad_guidance)) return e;
    return backward3d_norm_entry("cspn3d_backward_norm_g16", guidance, gate_dtype, feat, sparse, grad_out, grad_guidance, grad_feat, B, D, H, W,
                                 n_iter, norm_type, algo, ws, ws_bytes, stream);
}

// ---- the same modes for C channels on shared guidance (feat / out / grad_out / grad_feat [B,C,D,H,W], sparse NULL or [B,1,D,H,W]) ----
static bool norm_multi_query_ok(int B, int C, int D, int H, int W, int n_iter, int norm_type) {
    return B > 0 && C > 0 && D > 0 && H > 0 && W > 0 && n_iter > 0 && norm_type >= CSPN_NORM_8SUM && norm_type <= CSPN_NORM_NONE;
}

size_t cspn3d_forward_norm_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter, int norm_type, int has_sparse) {
    if (!norm_multi_query_ok(B, C, D, H, W, n_iter, norm_type)) return 0;
    if (C == 1) return forward3d_workspace(B, D, H, W, n_iter, norm_type, has_sparse != 0);
    return forward3d_norm_multi_workspace(B, C, D, H, W, n_iter);   // (covers the Paddle contract's persistent3d_workspace too)
}

// one query for both gate types: C = 1 is cspn3d_backward_norm_g16_workspace_bytes (the float32 twin's, and for NONE without a mask the
// widened copy of the Paddle contract's transposed sweep more); NONE without a mask is cspn3d_backward_multi_g16_workspace_bytes
size_t cspn3d_backward_norm_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter, int norm_type, int has_sparse) {
    if (!norm_multi_query_ok(B, C, D, H, W, n_iter, norm_type)) return 0;
    if (C == 1) return backward3d_norm_need(B, D, H, W, n_iter, norm_type, has_sparse != 0, CSPN_DTYPE_F16);
    if (norm_type == CSPN_NORM_NONE && !has_sparse) return backward3d_workspace(B, D, H, W, n_iter, C, CSPN_DTYPE_F16);
    return backward3d_norm_multi_workspace(B, C, D, H, W, n_iter);
}

// the checks of cspn3d_forward_norm_multi_f32 (gdt 0) and cspn3d_forward_norm_multi_g16, then the engine
static int forward3d_norm_multi_entry(const char* what, const void* guidance, int gdt, const float* feat, const float* sparse, float* out, int B,
                                      int C, int D, int H, int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes,
                                      cspn_stream_t stream) {
    if (int e = check_shape("BCDHW", {B, C, D, H, W})) return e;
    if (B == 0) return 0;
    if (C == 1) return forward3d_entry(guidance, gdt, feat, sparse, out, B, D, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
    const size_t V = (size_t)B * D * H * W;
    if (int e = check_index32((long long)V, 27)) return e;
    if (algo < CSPN_ALGO3D_AUTO || algo > CSPN_ALGO3D_PERSISTENT) { set_error("unknown 3D algo %d", algo); return CSPN_E_BADARG; }
    if (norm_type < CSPN_NORM_8SUM || norm_type > CSPN_NORM_NONE) {
        set_error("%s: norm_type must be CSPN_NORM_8SUM, CSPN_NORM_8SUM_ABS or CSPN_NORM_NONE (got %d)", what, norm_type);
        return CSPN_E_BADARG;
    }
    if (int e = async_failure_of_earlier_call()) return e;
    const size_t need = n_iter <= 0 ? 0 : forward3d_norm_multi_workspace(B, C, D, H, W, n_iter);
    if (int e = check_common(guidance, feat, out, n_iter, norm_type, ws, ws_bytes, need)) return e;
    const size_t vb = sizeof(float) * V * C, sb = sizeof(float) * V, gb = 26 * V * gate_bytes(gdt);
    if (kxk_overlaps(out, vb, {{guidance, gb}, {feat, vb}, {sparse, sb}, {ws, need}})) {
        set_error("%s: the output must not overlap an input or the workspace", what);
        return CSPN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_copy(out, feat, V * C, st);
    // the Paddle contract: cspn3d_forward_multi_f32 / _g16 where it runs (the persistent kernel on the gates as given), bitwise
    if (norm_type == CSPN_NORM_NONE && !sparse && algo != CSPN_ALGO3D_STEPWISE && quads_ok(W, gdt, {guidance}, {feat, out, ws}) &&
        persistent3d_multi_supported(B, C, D, H, W, n_iter))
        return persistent3d_forward_multi(guidance, feat, out, B, C, D, H, W, n_iter, ws, st, gdt);
    return forward3d_norm_multi(guidance, gdt, feat, sparse, out, B, C, D, H, W, n_iter, norm_type, ws, st, algo);
}

int cspn3d_forward_norm_multi_f32(const float* guidance, const float* feat, const float* sparse, float* out, int B, int C, int D, int H, int W,
                                  int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return forward3d_norm_multi_entry("cspn3d_forward_norm_multi_f32", guidance, 0, feat, sparse, out, B, C, D, H, W, n_iter, norm_type, algo, ws,
                                      ws_bytes, stream);
}

int cspn3d_forward_norm_multi_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, float* out, int B, int C, int D,
                                  int H, int W, int n_iter, int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_forward_norm_multi_g16", gate_dtype, guidance, nullptr)) return e;
    return forward3d_norm_multi_entry("cspn3d_forward_norm_multi_g16", guidance, gate_dtype, feat, sparse, out, B, C, D, H, W, n_iter, norm_type,
                                      algo, ws, ws_bytes, stream);
}

// the checks of cspn3d_backward_norm_multi_f32 (gdt 0) and cspn3d_backward_norm_multi_g16, in backward3d_norm_entry's order, then the engine
static int backward3d_norm_multi_entry(const char* what, const void* guidance, int gdt, const float* feat, const float* sparse,
                                       const float* grad_out, void* grad_guidance, float* grad_feat, int B, int C, int D, int H, int W, int n_iter,
                                       int norm_type, int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BCDHW", {B, C, D, H, W})) return e;
    if (B == 0) return 0;
    if (C == 1)
        return backward3d_norm_entry(what, guidance, gdt, feat, sparse, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter, norm_type, algo, ws,
                                     ws_bytes, stream);
    const size_t V = (size_t)B * D * H * W;
    if (int e = check_index32((long long)V, 27)) return e;
    if (algo < CSPN_ALGO3D_AUTO || algo > CSPN_ALGO3D_PERSISTENT) { set_error("unknown 3D algo %d", algo); return CSPN_E_BADARG; }
    if (norm_type < CSPN_NORM_8SUM || norm_type > CSPN_NORM_NONE) {
        set_error("%s: norm_type must be CSPN_NORM_8SUM, CSPN_NORM_8SUM_ABS or CSPN_NORM_NONE (got %d)", what, norm_type);
        return CSPN_E_BADARG;
    }
    if (int e = async_failure_of_earlier_call()) return e;
    const bool paddle = norm_type == CSPN_NORM_NONE && !sparse;
    const size_t need = n_iter <= 0 ? 0 : paddle ? backward3d_workspace(B, D, H, W, n_iter, C, gdt) : backward3d_norm_multi_workspace(B, C, D, H, W, n_iter);
    if (int e = check_common(guidance, feat, grad_out, n_iter, norm_type, ws, ws_bytes, need)) return e;
    const size_t vb = sizeof(float) * V * C, sb = sizeof(float) * V, gb = 26 * V * gate_bytes(gdt);
    if (kxk_overlaps(grad_guidance, gb, {{guidance, gb}, {feat, vb}, {sparse, sb}, {grad_out, vb}, {grad_feat, vb}, {ws, need}}) ||
        kxk_overlaps(grad_feat, vb, {{guidance, gb}, {feat, vb}, {sparse, sb}, {grad_out, vb}, {ws, need}})) {
        set_error("%s: an output must not overlap an input, the other output or the workspace", what);
        return CSPN_E_BADARG;
    }
    if (!grad_guidance && !grad_feat) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_backward(grad_feat, grad_out, V * C, grad_guidance, gb, st);
    if (algo == CSPN_ALGO3D_PERSISTENT &&
        !backward3d_norm_multi_fused(guidance, gdt, feat, sparse, grad_out, grad_guidance, grad_feat, B, C, D, H, W, n_iter, ws)) {
        set_error("persistent 3D kernel does not take this backward (needs W %% 4 == 0, 16-byte aligned tensors, 3 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    const bool stepwise_only = algo == CSPN_ALGO3D_STEPWISE;
    if (paddle)   // the Paddle contract: cspn3d_backward_multi_f32 / _g16 (for every shape: its per-step kernels take what the sweeps decline)
        return backward3d(guidance, feat, grad_out, grad_guidance, grad_feat, B, D, H, W, n_iter, ws, st, stepwise_only, C, gdt);
    return backward3d_norm_multi(guidance, gdt, feat, sparse, grad_out, grad_guidance, grad_feat, B, C, D, H, W, n_iter, norm_type, ws, st,
                                 stepwise_only);
}

int cspn3d_backward_norm_multi_f32(const float* guidance, const float* feat, const float* sparse, const float* grad_out, float* grad_guidance,
                                   float* grad_feat, int B, int C, int D, int H, int W, int n_iter, int norm_type, int algo, void* ws,
                                   size_t ws_bytes, cspn_stream_t stream) {
    return backward3d_norm_multi_entry("cspn3d_backward_norm_multi_f32", guidance, 0, feat, sparse, grad_out, grad_guidance, grad_feat, B, C, D, H, W,
                                       n_iter, norm_type, algo, ws, ws_bytes, stream);
}

int cspn3d_backward_norm_multi_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, const float* grad_out,
                                   void* grad_guidance, float* grad_feat, int B, int C, int D, int H, int W, int n_iter, int norm_type, int algo,
                                   void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_backward_norm_multi_g16", gate_dtype, guidance, grad_guidance)) return e;
    return backward3d_norm_multi_entry("cspn3d_backward_norm_multi_g16", guidance, gate_dtype, feat, sparse, grad_out, grad_guidance, grad_feat, B, C,
                                       D, H, W, n_iter, norm_type, algo, ws, ws_bytes, stream);
}

size_t cspn3d_backward_g16_workspace_bytes(int B, int D, int H, int W, int n_iter) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return backward3d_workspace(B, D, H, W, n_iter, 1, CSPN_DTYPE_F16);
}

int cspn3d_backward_g16(const void* gate, int gate_dtype, const float* feat, const float* grad_out, void* grad_gate, float* grad_feat, int B,
                        int D, int H, int W, int n_iter, int norm_type, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_backward_g16", gate_dtype, gate, grad_gate)) return e;
    return backward3d_entry(false, gate, gate_dtype, feat, grad_out, grad_gate, grad_feat, B, 1, D, H, W, n_iter, norm_type, ws, ws_bytes, stream);
}

size_t cspn3d_backward_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return backward3d_workspace(B, D, H, W, n_iter, C);
}

int cspn3d_backward_multi_f32(const float* gate, const float* feat, const float* grad_out, float* grad_gate, float* grad_feat, int B,
                              int C, int D, int H, int W, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return backward3d_entry(true, gate, 0, feat, grad_out, grad_gate, grad_feat, B, C, D, H, W, n_iter, CSPN_NORM_NONE, ws, ws_bytes, stream);
}

size_t cspn3d_backward_multi_g16_workspace_bytes(int B, int C, int D, int H, int W, int n_iter) {
    if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return backward3d_workspace(B, D, H, W, n_iter, C, CSPN_DTYPE_F16);
}

int cspn3d_backward_multi_g16(const void* gate, int gate_dtype, const float* feat, const float* grad_out, void* grad_gate, float* grad_feat, int B,
                              int C, int D, int H, int W, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_backward_multi_g16", gate_dtype, gate, grad_gate)) return e;
    return backward3d_entry(true, gate, gate_dtype, feat, grad_out, grad_gate, grad_feat, B, C, D, H, W, n_iter, CSPN_NORM_NONE, ws, ws_bytes, stream);
}

// ---- the demo's module (reference cspn_paddle/demo.py:20-54): w = |g| / sum_k |g_k| per voxel over one slice's K gates, then the NONE op ----
int cspn_gate_absnorm_f32(const float* guide, float* gate, int N, int K, size_t V, cspn_stream_t stream) {
    if (int e = absnorm_check("cspn_gate_absnorm_f32", guide, guide, gate, N, K, V)) return e;
    return gate_absnorm(guide, gate, N, K, V, (hipStream_t)stream);
}

int cspn_gate_absnorm_backward_f32(const float* guide, const float* grad_gate, float* grad_guide, int N, int K, size_t V,
                                   cspn_stream_t stream) {
    if (int e = absnorm_check("cspn_gate_absnorm_backward_f32", guide, grad_gate, grad_guide, N, K, V)) return e;
    return gate_absnorm_backward(guide, grad_gate, grad_guide, N, K, V, (hipStream_t)stream);
}

// the 3D module's forms on a 16-bit guide (K = 26 only)
static int absnorm_g16_check(const char* what, int dtype, const void* guide, const void* grad_guide, int K) {
    if (int e = g16_check(what, dtype, guide, grad_guide)) return e;
    if (K != 26) { set_error("%s: K must be 26 (the 3D module), got %d", what, K); return CSPN_E_BADARG; }
    return 0;
}

int cspn_gate_absnorm_g16(const void* guide, int gate_dtype, float* gate, int N, int K, size_t V, cspn_stream_t stream) {
    if (int e = absnorm_g16_check("cspn_gate_absnorm_g16", gate_dtype, guide, nullptr, K)) return e;
    if (int e = absnorm_check("cspn_gate_absnorm_g16", guide, (const float*)guide, gate, N, K, V, 2)) return e;
    return gate_absnorm_g16(guide, gate_dtype, gate, N, V, (hipStream_t)stream);
}

int cspn_gate_absnorm_backward_g16(const void* guide, int gate_dtype, const float* grad_gate, void* grad_guide, int N, int K, size_t V,
                                   cspn_stream_t stream) {
    if (int e = absnorm_g16_check("cspn_gate_absnorm_backward_g16", gate_dtype, guide, grad_guide, K)) return e;
    if (int e = absnorm_check("cspn_gate_absnorm_backward_g16", guide, grad_gate, grad_guide, N, K, V, 2, true)) return e;
    return gate_absnorm_backward_g16(guide, gate_dtype, grad_gate, grad_guide, N, V, (hipStream_t)stream);
}

size_t cspn3d_forward_absnorm_workspace_bytes(int B, int D, int H, int W, int n_iter) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || n_iter <= 0) return 0;
    return absnorm_planes_bytes(B, D, H, W) + forward3d_workspace(B, D, H, W, n_iter, CSPN_NORM_NONE, false);
}

static int forward3d_absnorm_entry(const char* what, const void* guide, int gdt, const float* feat, float* out, int B, int D, int H, int W, int n_iter,
                                   int algo, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = check_shape("BDHW", {B, D, H, W})) return e;
    if (B == 0) return 0;
    if (int e = check_index32((long long)B * D * H * W, 27)) return e;
    if (algo < CSPN_ALGO3D_AUTO || algo > CSPN_ALGO3D_PERSISTENT) { set_error("unknown 3D algo %d", algo); return CSPN_E_BADARG; }
    const size_t total = (size_t)B * D * H * W;
    if (guide && feat && out && (overlaps(out, total * sizeof(float), guide, 26 * total * gate_bytes(gdt)) || overlaps(out, total * sizeof(float), feat, total * sizeof(float)))) {
        set_error("%s: out must not alias an input", what);
        return CSPN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (int e = async_failure_of_earlier_call()) return e;
    // misaligned feat / out take the folding path after the normaliser: its 27 planes more (as cspn3d_forward_f32 with such tensors)
    const bool vals_aligned = quads_ok(W, gdt, {}, {feat, out});   // (W % 4 != 0 takes the folding path's size from either query)
    const size_t need = n_iter == 0 ? 0 : absnorm_planes_bytes(B, D, H, W) + (vals_aligned ? forward3d_workspace(B, D, H, W, n_iter, CSPN_NORM_NONE, false)
                                                                                            : stepwise3d_workspace(B, D, H, W, n_iter));
    if (int e = check_common(guide, feat, out, n_iter, CSPN_NORM_NONE, ws, ws_bytes, need)) return e;
    if (n_iter == 0) return identity_copy(out, feat, total, st);
    const bool fused = quads_ok(W, gdt, {guide}, {feat, out, ws}) && persistent3d_supported(B, D, H, W, n_iter);
    if (algo == CSPN_ALGO3D_PERSISTENT && !fused) {
        set_error("persistent 3D kernel does not take this call (needs W %% 4 == 0, 16-byte aligned tensors, 2 <= n_iter <= 60, a chunk per device)");
        return CSPN_E_UNSUPPORTED;
    }
    if (fused && algo != CSPN_ALGO3D_STEPWISE) return persistent3d_forward_absnorm(guide, feat, out, B, D, H, W, n_iter, ws, st, gdt);
    // unfused: the normaliser into the workspace (float32 gates, whatever the guide's type), then the NONE op on it
    float* gate = (float*)ws;
    if (int e = gdt ? gate_absnorm_g16(guide, gdt, gate, B, (size_t)D * H * W, st) : gate_absnorm((const float*)guide, gate, B, 26, (size_t)D * H * W, st)) return e;
    return stepwise3d_forward(gate, feat, nullptr, out, B, D, H, W, n_iter, CSPN_NORM_NONE, (char*)ws + absnorm_planes_bytes(B, D, H, W), st, algo);
}

int cspn3d_forward_absnorm_f32(const float* guide, const float* feat, float* out, int B, int D, int H, int W, int n_iter, int algo,
                               void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return forward3d_absnorm_entry("cspn3d_forward_absnorm_f32", guide, 0, feat, out, B, D, H, W, n_iter, algo, ws, ws_bytes, stream);
}

int cspn3d_forward_absnorm_g16(const void* guide, int gate_dtype, const float* feat, float* out, int B, int D, int H, int W, int n_iter, int algo,
                               void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = g16_check("cspn3d_forward_absnorm_g16", gate_dtype, guide, nullptr)) return e;
    return forward3d_absnorm_entry("cspn3d_forward_absnorm_g16", guide, gate_dtype, feat, out, B, D, H, W, n_iter, algo, ws, ws_bytes, stream);
}


// ---- the 2D NONE op over a K x K neighbourhood, K = 5 or 7 (cspn2d_kxk.hip) ----
size_t cspn2d_kxk_workspace_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_shape_ok(B, C, H, W, K, n_iter) || n_iter < 2) return 0;
    return sizeof(float) * kxk_level_floats((size_t)B * C * H * W) * (n_iter == 2 ? 1 : 2);
}

size_t cspn2d_kxk_history_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_shape_ok(B, C, H, W, K, n_iter) || n_iter < 2) return 0;
    return kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1);
}

// the checks of the eight cspn2d_{forward,backward}_kxk[_absnorm]_{f32,g16} entry points, then the engine.  g16: 16-bit gates of dtype, else dtype 0;
// absnorm: the gates are the raw guide of the demo module's contract (the backward's workspace then also holds 1 / S)
static int kxk_forward_entry(const char* what, const void* gate, bool g16, int dtype, bool absnorm, const float* x, float* out, float* history,
                             size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (!gate || !x || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (g16)
        if (int e = g16_check(what, dtype, gate, nullptr)) return e;
    if (int e = kxk_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1);
    const size_t hb = cspn2d_kxk_history_bytes(B, C, H, W, K, n_iter);
    if (history && history_bytes < hb) { set_error("%s: history buffer too small: need %zu bytes, got %zu", what, hb, history_bytes); return CSPN_E_WORKSPACE; }
    const size_t need = history ? 0 : cspn2d_kxk_workspace_bytes(B, C, H, W, K, n_iter);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0;
    if (kxk_overlaps(out, vb, {{gate, gb}, {x, vb}, {history, hb}, {ws, wb}}) || kxk_overlaps(history, hb, {{gate, gb}, {x, vb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{gate, gb}, {x, vb}})) {
        set_error("%s: out, history and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) {
        hipError_t e = hipMemcpyAsync(out, x, vb, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) { set_error("hipMemcpyAsync: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    return kxk_forward(gate, dtype, absnorm, x, out, history, B, C, H, W, K, n_iter, ws, st);
}

static int kxk_backward_entry(const char* what, const void* gate, bool g16, int dtype, bool absnorm, const float* x, const float* history, size_t history_bytes,
                              const float* grad_out, void* grad_gate, float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws,
                              size_t ws_bytes, cspn_stream_t stream) {
    if (!gate || !x || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (g16)
        if (int e = g16_check(what, dtype, gate, grad_gate)) return e;
    if (int e = kxk_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1);
    const size_t hb = cspn2d_kxk_history_bytes(B, C, H, W, K, n_iter);
    if (grad_gate && hb && (!history || history_bytes < hb)) {
        set_error("%s: the gate gradient needs the forward's history: need %zu bytes, got %zu", what, hb, history ? history_bytes : 0);
        return CSPN_E_BADARG;
    }
    const size_t need = absnorm ? cspn2d_backward_kxk_absnorm_workspace_bytes(B, C, H, W, K, n_iter)
                                : cspn2d_backward_kxk_workspace_bytes(B, C, H, W, K, n_iter);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0, hbu = grad_gate ? hb : 0;
    if (grad_gate && grad_gate == (void*)grad_x) { set_error("%s: grad_gate and grad_x must not alias", what); return CSPN_E_BADARG; }
    if (kxk_overlaps(grad_gate, gb, {{gate, gb}, {x, vb}, {history, hbu}, {grad_out, vb}, {grad_x, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_x, vb, {{gate, gb}, {x, vb}, {history, hbu}, {grad_out, vb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{gate, gb}, {x, vb}, {history, hbu}, {grad_out, vb}})) {
        set_error("%s: grad_gate, grad_x and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (!grad_gate && !grad_x) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) {   // the identity: dL/dx = dL/dout, no gate is read
        hipError_t e = grad_x ? hipMemcpyAsync(grad_x, grad_out, vb, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess && grad_gate) e = hipMemsetAsync(grad_gate, 0, gb, st);
        if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    return kxk_backward(gate, dtype, absnorm, x, history, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter, ws, st);
}

int cspn2d_forward_kxk_f32(const float* gate, const float* x, float* out, float* history, size_t history_bytes, int B, int C, int H, int W,
                           int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_forward_entry("cspn2d_forward_kxk_f32", gate, false, 0, false, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

size_t cspn2d_backward_kxk_workspace_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_shape_ok(B, C, H, W, K, n_iter) || n_iter < 2) return 0;
    return round256(kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1));
}

int cspn2d_backward_kxk_f32(const float* gate, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                            float* grad_gate, float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes,
                            cspn_stream_t stream) {
    return kxk_backward_entry("cspn2d_backward_kxk_f32", gate, false, 0, false, x, history, history_bytes, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter,
                              ws, ws_bytes, stream);
}

// ---- the demo module's contract in the K x K engine (cspn2d_kxk.hip): the raw guide in the gates' place, the checks of the twins above ----
size_t cspn2d_backward_kxk_absnorm_workspace_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_shape_ok(B, C, H, W, K, n_iter) || n_iter < 2) return 0;   // a single step forms 1 / S as it stages: no plane
    return kxk_absnorm_alev_bytes((size_t)B * C * H * W, n_iter) + round256(sizeof(float) * (size_t)B * H * W);
}

int cspn2d_forward_kxk_absnorm_f32(const float* guide, const float* x, float* out, float* history, size_t history_bytes, int B, int C, int H, int W,
                                   int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_forward_entry("cspn2d_forward_kxk_absnorm_f32", guide, false, 0, true, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes,
                             stream);
}

int cspn2d_forward_kxk_absnorm_g16(const void* guide, int gate_dtype, const float* x, float* out, float* history, size_t history_bytes, int B, int C,
                                   int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_forward_entry("cspn2d_forward_kxk_absnorm_g16", guide, true, gate_dtype, true, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_absnorm_f32(const float* guide, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                                    float* grad_guide, float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes,
                                    cspn_stream_t stream) {
    return kxk_backward_entry("cspn2d_backward_kxk_absnorm_f32", guide, false, 0, true, x, history, history_bytes, grad_out, grad_guide, grad_x, B, C, H, W, K,
                              n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_absnorm_g16(const void* guide, int gate_dtype, const float* x, const float* history, size_t history_bytes,
                                    const float* grad_out, void* grad_guide, float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws,
                                    size_t ws_bytes, cspn_stream_t stream) {
    return kxk_backward_entry("cspn2d_backward_kxk_absnorm_g16", guide, true, gate_dtype, true, x, history, history_bytes, grad_out, grad_guide, grad_x, B, C, H, W, K, n_iter, ws,
                              ws_bytes, stream);
}

// ---- K x K propagation with per-step attention, K = 3, 5 or 7 (cspn2d_kxk_dyn.hip): the checks of the kxk_absnorm entry points, with att,
// grad_att and sparse among the ranges.  The n (R+1) attention planes are addressed in size_t by every kernel; an image's planes fit an int ----
static bool kxk_dyn_shape_ok(int B, int C, int H, int W, int K, int n_iter) {
    const long long px = (long long)H * W;
    return B > 0 && C > 0 && H > 0 && W > 0 && (K == 3 || K == 5 || K == 7) && n_iter >= 0 && (long long)B * C * px <= 0x7fffffffLL &&
           (long long)B * (K * K - 1) * px <= 0x7fffffffLL && (long long)B * n_iter * (K / 2 + 1) * px <= 0x7fffffffLL;
}

static int kxk_dyn_check_shape(const char* what, int B, int C, int H, int W, int K, int n_iter) {
    if (K != 3 && K != 5 && K != 7) { set_error("%s: K must be 3, 5 or 7, got %d", what, K); return CSPN_E_BADARG; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (n_iter < 0) { set_error("%s: n_iter must be >= 0 (got %d)", what, n_iter); return CSPN_E_BADARG; }
    if (!kxk_dyn_shape_ok(B, C, H, W, K, n_iter)) { set_error("%s: tensor too large for 32-bit element indexing", what); return CSPN_E_UNSUPPORTED; }
    return 0;
}

// H~_1 .. H~_{n-1}: cspn2d_kxk_history_bytes, which does not take K = 3
static size_t kxk_dyn_history_bytes(int B, int C, int H, int W, int n_iter) { return n_iter < 2 ? 0 : kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1); }

size_t cspn2d_kxk_dyn_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse, int keep_history) {
    if (!kxk_dyn_shape_ok(B, C, H, W, K, n_iter) || n_iter < 1) return 0;
    return round256(sizeof(float) * kxk_level_floats((size_t)B * C * H * W) * (size_t)kxk_dyn_forward_levels(n_iter, has_sparse != 0, keep_history != 0));
}

size_t cspn2d_backward_kxk_dyn_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse) {
    if (!kxk_dyn_shape_ok(B, C, H, W, K, n_iter) || n_iter < 1) return 0;
    return KxkDynBackwardWs(B, C, H, W, K, n_iter, has_sparse != 0).bytes;
}

int cspn2d_forward_kxk_dyn_f32(const float* guidance, const float* att, const float* x, const float* sparse, float* out, float* history,
                               size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    const char* what = "cspn2d_forward_kxk_dyn_f32";
    if (!guidance || !x || !out || (!att && n_iter > 0)) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = kxk_dyn_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), pb = vb / C, gb = pb * (K * K - 1), ab = pb * (size_t)n_iter * (K / 2 + 1);
    const size_t hb = kxk_dyn_history_bytes(B, C, H, W, n_iter);
    if (history && history_bytes < hb) { set_error("%s: history buffer too small: need %zu bytes, got %zu", what, hb, history_bytes); return CSPN_E_WORKSPACE; }
    const size_t need = cspn2d_kxk_dyn_workspace_bytes(B, C, H, W, K, n_iter, sparse != nullptr, history != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0;
    if (kxk_overlaps(out, vb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {history, hb}, {ws, wb}}) ||
        kxk_overlaps(history, hb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}})) {
        set_error("%s: out, history and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_copy(out, x, vb / sizeof(float), st);
    return kxk_dyn_forward(guidance, att, x, sparse, out, history, B, C, H, W, K, n_iter, ws, st);
}

int cspn2d_backward_kxk_dyn_f32(const float* guidance, const float* att, const float* x, const float* sparse, const float* history, size_t history_bytes,
                                const float* grad_out, float* grad_guidance, float* grad_att, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                                void* ws, size_t ws_bytes, cspn_stream_t stream) {
    const char* what = "cspn2d_backward_kxk_dyn_f32";
    if (!guidance || !x || !grad_out || (!att && n_iter > 0)) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = kxk_dyn_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), pb = vb / C, gb = pb * (K * K - 1), ab = pb * (size_t)n_iter * (K / 2 + 1);
    const size_t hb = kxk_dyn_history_bytes(B, C, H, W, n_iter);
    const bool grads = grad_guidance || grad_att;
    if (grads && hb && (!history || history_bytes < hb)) {
        set_error("%s: the guidance and attention gradients need the forward's history: need %zu bytes, got %zu", what, hb, history ? history_bytes : 0);
        return CSPN_E_BADARG;
    }
    const size_t need = cspn2d_backward_kxk_dyn_workspace_bytes(B, C, H, W, K, n_iter, sparse != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0, hbu = grads ? hb : 0;
    if ((grad_guidance && ((void*)grad_guidance == (void*)grad_x || (void*)grad_guidance == (void*)grad_att)) || (grad_att && (void*)grad_att == (void*)grad_x)) {
        set_error("%s: grad_guidance, grad_att and grad_x must not alias", what);
        return CSPN_E_BADARG;
    }
    if (kxk_overlaps(grad_guidance, gb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {history, hbu}, {grad_out, vb}, {grad_att, ab}, {grad_x, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_att, ab, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {history, hbu}, {grad_out, vb}, {grad_x, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_x, vb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {history, hbu}, {grad_out, vb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{guidance, gb}, {att, ab}, {x, vb}, {sparse, pb}, {history, hbu}, {grad_out, vb}})) {
        set_error("%s: grad_guidance, grad_att, grad_x and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (!grads && !grad_x) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_backward(grad_x, grad_out, vb / sizeof(float), grad_guidance, gb, st);   // no attention plane exists
    return kxk_dyn_backward(guidance, att, x, sparse, history, grad_out, grad_guidance, grad_att, grad_x, B, C, H, W, K, n_iter, ws, st);
}

// ---- line-scan propagation, SPN's three-way recurrence (cspn2d_scan.hip); added to ABI 5 after its release, purely additive: the checks of
// the kxk_dyn entry points.  A line (H for directions 0 / 1, W for 2 / 3) has at most SCAN_MAX_LINE pixels ----
static bool scan_args_ok(int B, int C, int Cg, int H, int W, int dirs) {
    return B > 0 && C > 0 && Cg > 0 && H > 0 && W > 0 && C % Cg == 0 && dirs >= 1 && dirs <= 15;
}

static bool scan_shape_ok(int B, int C, int Cg, int H, int W, int dirs) {
    if (!scan_args_ok(B, C, Cg, H, W, dirs)) return false;
    const long long px = (long long)H * W, D = __builtin_popcount(dirs);
    if (((dirs & 3) && H > SCAN_MAX_LINE) || ((dirs & 12) && W > SCAN_MAX_LINE)) return false;
    return (long long)B * D * C * px <= 0x7fffffffLL && (long long)B * D * Cg * 3 * px <= 0x7fffffffLL;
}

static int scan_check_shape(const char* what, int B, int C, int Cg, int H, int W, int dirs) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (Cg <= 0 || C % Cg) { set_error("%s: Cg must divide C (got C=%d Cg=%d)", what, C, Cg); return CSPN_E_BADARG; }
    if (dirs < 1 || dirs > 15) { set_error("%s: dirs must be a non-empty mask of the directions 0 .. 3 (1 .. 15), got %d", what, dirs); return CSPN_E_BADARG; }
    if (!scan_shape_ok(B, C, Cg, H, W, dirs)) {
        set_error("%s: a line of more than %d pixels (H for directions 0 / 1, W for 2 / 3), or a tensor too large for 32-bit element indexing", what, SCAN_MAX_LINE);
        return CSPN_E_UNSUPPORTED;
    }
    return 0;
}

// the forward needs no memory beyond its tensors; the one block keeps the query's "0 = rejected" readable
size_t cspn2d_scan_workspace_bytes(int B, int C, int Cg, int H, int W, int dirs, int has_lam) {
    (void)has_lam;
    return scan_shape_ok(B, C, Cg, H, W, dirs) ? 256 : 0;
}

size_t cspn2d_backward_scan_workspace_bytes(int B, int C, int Cg, int H, int W, int dirs, int has_lam) {
    (void)has_lam;
    return scan_shape_ok(B, C, Cg, H, W, dirs) ? ScanBackwardWs(B, C, Cg, H, W, __builtin_popcount(dirs)).bytes : 0;
}

int cspn2d_forward_scan_f32(const float* x, const float* gates, const float* lam, float* out, int B, int C, int Cg, int H, int W, int dirs, void* ws,
                            size_t ws_bytes, cspn_stream_t stream) {
    const char* what = "cspn2d_forward_scan_f32";
    if (!x || !gates || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = scan_check_shape(what, B, C, Cg, H, W, dirs)) return e;
    const int D = __builtin_popcount(dirs);
    const size_t xb = kxk_values_bytes(B, C, H, W), ob = xb * D, gb = ob / C * Cg * 3;
    const size_t need = cspn2d_scan_workspace_bytes(B, C, Cg, H, W, dirs, lam != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    if (kxk_overlaps(out, ob, {{x, xb}, {gates, gb}, {lam, ob}, {ws, ws_bytes}}) || kxk_overlaps(ws, ws_bytes, {{x, xb}, {gates, gb}, {lam, ob}})) {
        set_error("%s: out and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    return scan_forward(x, gates, lam, out, B, C, Cg, H, W, dirs, (hipStream_t)stream);
}

int cspn2d_backward_scan_f32(const float* x, const float* gates, const float* lam, const float* out, const float* grad_out, float* grad_x,
                             float* grad_gates, float* grad_lam, int B, int C, int Cg, int H, int W, int dirs, void* ws, size_t ws_bytes,
                             cspn_stream_t stream) {
    const char* what = "cspn2d_backward_scan_f32";
    if (!x || !gates || !out || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (grad_lam && !lam) { set_error("%s: grad_lam without lam", what); return CSPN_E_BADARG; }
    if (int e = scan_check_shape(what, B, C, Cg, H, W, dirs)) return e;
    const int D = __builtin_popcount(dirs);
    const size_t xb = kxk_values_bytes(B, C, H, W), ob = xb * D, gb = ob / C * Cg * 3;
    const size_t need = cspn2d_backward_scan_workspace_bytes(B, C, Cg, H, W, dirs, lam != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    if ((grad_x && ((void*)grad_x == (void*)grad_gates || (void*)grad_x == (void*)grad_lam)) || (grad_gates && (void*)grad_gates == (void*)grad_lam)) {
        set_error("%s: grad_x, grad_gates and grad_lam must not alias", what);
        return CSPN_E_BADARG;
    }
    if (kxk_overlaps(grad_x, xb, {{x, xb}, {gates, gb}, {lam, ob}, {out, ob}, {grad_out, ob}, {grad_gates, gb}, {grad_lam, ob}, {ws, ws_bytes}}) ||
        kxk_overlaps(grad_gates, gb, {{x, xb}, {gates, gb}, {lam, ob}, {out, ob}, {grad_out, ob}, {grad_lam, ob}, {ws, ws_bytes}}) ||
        kxk_overlaps(grad_lam, ob, {{x, xb}, {gates, gb}, {lam, ob}, {out, ob}, {grad_out, ob}, {ws, ws_bytes}}) ||
        kxk_overlaps(ws, ws_bytes, {{x, xb}, {gates, gb}, {lam, ob}, {out, ob}, {grad_out, ob}})) {
        set_error("%s: grad_x, grad_gates, grad_lam and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (!grad_x && !grad_gates && !grad_lam) return 0;
    return scan_backward(x, gates, lam, out, grad_out, grad_x, grad_gates, grad_lam, B, C, Cg, H, W, dirs, ws, (hipStream_t)stream);
}

// ---- the depth-completion contract over a K x K neighbourhood, K = 3, 5 or 7 (cspn2d_kxk.hip) ----
size_t cspn2d_kxk_norm_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter) {
    if (!kxk_norm_shape_ok(B, C, sparse_C, H, W, K, n_iter) || n_iter < 1) return 0;
    const size_t levels = n_iter < 2 ? 0 : kxk_level_floats((size_t)B * C * H * W) * (n_iter == 2 ? 1 : 2);
    return sizeof(float) * (kxk_norm_fold_floats(B, C, sparse_C, H, W, K) + levels);
}

size_t cspn2d_kxk_norm_history_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_norm_shape_ok(B, C, 0, H, W, K, n_iter) || n_iter < 2) return 0;
    return kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1);
}

// the checks of the four cspn2d_{forward,backward}_kxk_norm_{f32,g16} entry points, then the engine; g16 and dtype as kxk_forward_entry
static int kxk_norm_forward_entry(const char* what, const void* guidance, bool g16, int dtype, const float* blur, const float* sparse, float* out,
                                  float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                                  size_t ws_bytes, cspn_stream_t stream, int dilation = 1, const KxkPin* pin = nullptr) {
    if (!guidance || !blur || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (g16)
        if (int e = g16_check(what, dtype, guidance, nullptr)) return e;
    if (int e = kxk_norm_check(what, sparse, B, C, sparse_C, H, W, K, n_iter, norm)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1), sb = vb / C * sparse_C;
    const size_t hb = cspn2d_kxk_norm_history_bytes(B, C, H, W, K, n_iter);
    if (history && history_bytes < hb) { set_error("%s: history buffer too small: need %zu bytes, got %zu", what, hb, history_bytes); return CSPN_E_WORKSPACE; }
    const size_t need = n_iter == 0 ? 0
                        : (history ? sizeof(float) * kxk_norm_fold_floats(B, C, sparse_C, H, W, K)
                                   : cspn2d_kxk_norm_workspace_bytes(B, C, sparse_C, H, W, K, n_iter));
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0;
    if (kxk_overlaps(out, vb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {history, hb}, {ws, wb}}) ||
        kxk_overlaps(history, hb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{guidance, gb}, {blur, vb}, {sparse, sb}}) ||
        (pin && (kxk_overlaps(out, vb, {{pin->conf, sb}}) || kxk_overlaps(history, hb, {{pin->conf, sb}}) || kxk_overlaps(ws, wb, {{pin->conf, sb}})))) {
        set_error("%s: out, history and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) {
        hipError_t e = hipMemcpyAsync(out, blur, vb, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) { set_error("hipMemcpyAsync: %s", hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    if (pin) return kxk_norm_forward_pin(guidance, dtype, blur, sparse, *pin, out, history, B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws, st);
    if (dilation != 1) return kxk_norm_forward_dil(guidance, dtype, blur, sparse, out, history, B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws, st);
    return kxk_norm_forward(guidance, dtype, blur, sparse, out, history, B, C, sparse_C, H, W, K, n_iter, norm, ws, st);
}

int cspn2d_forward_kxk_norm_f32(const float* guidance, const float* blur, const float* sparse, float* out, float* history, size_t history_bytes, int B,
                                int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_norm_forward_entry("cspn2d_forward_kxk_norm_f32", guidance, false, 0, blur, sparse, out, history, history_bytes, B, C, sparse_C, H, W, K,
                                  n_iter, norm, ws, ws_bytes, stream);
}

size_t cspn2d_backward_kxk_norm_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter) {
    if (!kxk_norm_shape_ok(B, C, sparse_C, H, W, K, n_iter) || n_iter < 1) return 0;
    return sizeof(float) * 2 * kxk_norm_fold_floats(B, C, sparse_C, H, W, K) + round256(kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1));
}

static int kxk_norm_backward_entry(const char* what, const void* guidance, bool g16, int dtype, const float* blur, const float* sparse,
                                   const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur, int B, int C,
                                   int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream,
                                   int dilation = 1, const KxkPin* pin = nullptr) {
    if (!guidance || !blur || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (g16)
        if (int e = g16_check(what, dtype, guidance, grad_guidance)) return e;
    if (int e = kxk_norm_check(what, sparse, B, C, sparse_C, H, W, K, n_iter, norm)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1), sb = vb / C * sparse_C;
    const size_t hb = cspn2d_kxk_norm_history_bytes(B, C, H, W, K, n_iter);
    float* const grad_sparse = pin ? pin->gs : nullptr;
    float* const grad_pin = pin ? pin->gp : nullptr;
    const bool gates = grad_guidance || grad_pin;   // dL/dpin needs dL/dw' as the guidance gradient does
    if (gates && hb && (!history || history_bytes < hb)) {
        set_error("%s: the guidance gradient%s needs the forward's history: need %zu bytes, got %zu", what, pin ? " and grad_pin" : "", hb,
                  history ? history_bytes : 0);
        return CSPN_E_BADARG;
    }
    const size_t need = cspn2d_backward_kxk_norm_workspace_bytes(B, C, sparse_C, H, W, K, n_iter);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0, hbu = gates ? hb : 0;
    if (grad_guidance && (const void*)grad_guidance == (const void*)grad_blur) { set_error("%s: grad_guidance and grad_blur must not alias", what); return CSPN_E_BADARG; }
    if (kxk_overlaps(grad_guidance, gb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}, {grad_blur, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_blur, vb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}})) {
        set_error("%s: grad_guidance, grad_blur and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (pin) {
        const std::initializer_list<std::pair<const void*, size_t>> inputs = {{guidance, gb}, {blur, vb}, {sparse, sb}, {pin->conf, sb}, {history, hbu}, {grad_out, vb}};
        if (kxk_overlaps(grad_guidance, gb, {{pin->conf, sb}}) || kxk_overlaps(grad_blur, vb, {{pin->conf, sb}}) || kxk_overlaps(ws, wb, {{pin->conf, sb}}) ||
            kxk_overlaps(grad_sparse, sb, inputs) || kxk_overlaps(grad_pin, sb, inputs) ||
            kxk_overlaps(grad_sparse, sb, {{grad_guidance, gb}, {grad_blur, vb}, {grad_pin, sb}, {ws, wb}}) ||
            kxk_overlaps(grad_pin, sb, {{grad_guidance, gb}, {grad_blur, vb}, {ws, wb}})) {
            set_error("%s: grad_sparse, grad_pin, the other gradients and the workspace must not alias an input or each other", what);
            return CSPN_E_BADARG;
        }
    }
    if (!grad_guidance && !grad_blur && !grad_sparse && !grad_pin) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) {   // the identity: dL/dblur = dL/dout, no gate is read
        hipError_t e = grad_blur ? hipMemcpyAsync(grad_blur, grad_out, vb, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess && grad_sparse) e = hipMemsetAsync(grad_sparse, 0, sb, st);
        if (e == hipSuccess && grad_pin) e = hipMemsetAsync(grad_pin, 0, sb, st);
        if (e == hipSuccess && grad_guidance) e = hipMemsetAsync(grad_guidance, 0, gb, st);
        if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    if (pin)
        return kxk_norm_backward_pin(guidance, dtype, blur, sparse, *pin, history, grad_out, grad_guidance, grad_blur, B, C, sparse_C, H, W, K, dilation, n_iter,
                                     norm, ws, st);
    if (dilation != 1)
        return kxk_norm_backward_dil(guidance, dtype, blur, sparse, history, grad_out, grad_guidance, grad_blur, B, C, sparse_C, H, W, K, dilation, n_iter, norm,
                                     ws, st);
    return kxk_norm_backward(guidance, dtype, blur, sparse, history, grad_out, grad_guidance, grad_blur, B, C, sparse_C, H, W, K, n_iter, norm, ws, st);
}

int cspn2d_backward_kxk_norm_f32(const float* guidance, const float* blur, const float* sparse, const float* history, size_t history_bytes,
                                 const float* grad_out, float* grad_guidance, float* grad_blur, int B, int C, int sparse_C, int H, int W, int K,
                                 int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_norm_backward_entry("cspn2d_backward_kxk_norm_f32", guidance, false, 0, blur, sparse, history, history_bytes, grad_out, grad_guidance, grad_blur,
                                   B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

// ---- the four K x K entry points on 16-bit gates / guidance (cspn2d_*_kxk*_g16): the checks of the _f32 twins, the gate tensor and its
// gradient sized and aligned as 2-byte elements ----

int cspn2d_forward_kxk_g16(const void* gate, int gate_dtype, const float* x, float* out, float* history, size_t history_bytes, int B, int C, int H,
                           int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_forward_entry("cspn2d_forward_kxk_g16", gate, true, gate_dtype, false, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_g16(const void* gate, int gate_dtype, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                            void* grad_gate, float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes,
                            cspn_stream_t stream) {
    return kxk_backward_entry("cspn2d_backward_kxk_g16", gate, true, gate_dtype, false, x, history, history_bytes, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes,
                              stream);
}

int cspn2d_forward_kxk_norm_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, float* out, float* history,
                                size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                                size_t ws_bytes, cspn_stream_t stream) {
    return kxk_norm_forward_entry("cspn2d_forward_kxk_norm_g16", guidance, true, gate_dtype, blur, sparse, out, history, history_bytes, B, C, sparse_C, H, W,
                                  K, n_iter, norm, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_norm_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* history,
                                 size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur, int B, int C, int sparse_C,
                                 int H, int W, int K, int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_norm_backward_entry("cspn2d_backward_kxk_norm_g16", guidance, true, gate_dtype, blur, sparse, history, history_bytes, grad_out, grad_guidance,
                                   grad_blur, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

// ---- the assembling contract over K x K levels (cspn2d_*_kxk_assemble*): the folded contract's arguments and checks, plus the confidences, the
// collected iterations (host memory, read here) and, in the backward, dL/dconf ----
size_t cspn2d_kxk_assemble_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter) {
    return cspn2d_kxk_norm_workspace_bytes(B, C, sparse_C, H, W, K, n_iter);   // the fold and the ping-pong levels; out is the third buffer
}

size_t cspn2d_kxk_assemble_history_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!kxk_norm_shape_ok(B, C, 0, H, W, K, n_iter) || n_iter < 1) return 0;
    return kxk_values_bytes(B, C, H, W) * (size_t)n_iter;   // H_1 .. H_n
}

size_t cspn2d_backward_kxk_assemble_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter) {
    const size_t norm = cspn2d_backward_kxk_norm_workspace_bytes(B, C, sparse_C, H, W, K, n_iter);
    return norm ? norm + sizeof(float) * kxk_level_floats((size_t)B * C * H * W) : 0;   // then A_n = conf_{T-1} grad_out
}

// what the assembling entries check before the folded contract's own checks: every pointer by name, the shape, conf's size, the steps
static int kxk_assemble_check(const char* what, std::initializer_list<std::pair<const char*, const void*>> required, const float* sparse, const int* steps, int T,
                              int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm) {
    for (const auto& r : required)
        if (!r.second) { set_error("%s: %s is NULL", what, r.first); return CSPN_E_BADARG; }
    if (K != 3 && K != 5 && K != 7) { set_error("%s: K must be 3, 5 or 7, got %d", what, K); return CSPN_E_BADARG; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (n_iter < 1) { set_error("%s: n_iter must be >= 1 (got %d)", what, n_iter); return CSPN_E_BADARG; }
    if (norm != CSPN_NORM_8SUM && norm != CSPN_NORM_8SUM_ABS) { set_error("%s: norm must be CSPN_NORM_8SUM or CSPN_NORM_8SUM_ABS, got %d", what, norm); return CSPN_E_BADARG; }
    if ((sparse_C != 0 && sparse_C != 1 && sparse_C != C) || (sparse_C == 0) != (sparse == nullptr)) {
        set_error("%s: sparse_C must be 0 (sparse NULL), 1 or C = %d (sparse given), got %d", what, C, sparse_C);
        return CSPN_E_BADARG;
    }
    if (T < 1 || T > n_iter + 1) { set_error("%s: T must be in 1 .. n_iter + 1 = %d, got %d", what, n_iter + 1, T); return CSPN_E_BADARG; }
    const long long px = (long long)H * W, lim = 0x7fffffffLL;
    if ((long long)B * C * px > lim) { set_error("%s: blur / out of B C H W = %lld elements: a view must stay below 2^31 elements", what, (long long)B * C * px); return CSPN_E_BADARG; }
    if ((sparse_C > 1 ? (long long)B * C : B) * (K * K - 1) * px > lim) { set_error("%s: guidance (per mask) of more than 2^31 - 1 elements", what); return CSPN_E_BADARG; }
    if ((long long)B * T * px > lim) { set_error("%s: conf of B T H W = %lld elements: a view must stay below 2^31 elements", what, (long long)B * T * px); return CSPN_E_BADARG; }
    for (int j = 0; j < T; ++j)
        if (steps[j] < 0 || (j && steps[j] <= steps[j - 1])) { set_error("%s: steps must be strictly increasing from >= 0 (steps[%d] = %d)", what, j, steps[j]); return CSPN_E_BADARG; }
    if (steps[T - 1] != n_iter) { set_error("%s: steps[T-1] must be n_iter = %d, got %d", what, n_iter, steps[T - 1]); return CSPN_E_BADARG; }
    return 0;
}

static int kxk_assemble_forward_entry(const char* what, const void* guidance, bool g16, int dtype, const float* blur, const float* sparse, const float* conf,
                                      const int* steps, int T, float* out, float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W,
                                      int K, int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream, int dilation = 1,
                                      const KxkPin* pin = nullptr) {
    if (int e = kxk_assemble_check(what, {{"guidance", guidance}, {"blur", blur}, {"conf", conf}, {"steps", steps}, {"out", out}}, sparse, steps, T, B, C,
                                   sparse_C, H, W, K, n_iter, norm))
        return e;
    if (g16)
        if (int e = g16_check(what, dtype, guidance, nullptr)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1), sb = vb / C * sparse_C, cb = vb / C * T;
    const size_t hb = cspn2d_kxk_assemble_history_bytes(B, C, H, W, K, n_iter);
    if (history && history_bytes < hb) { set_error("%s: history buffer too small: need %zu bytes, got %zu", what, hb, history_bytes); return CSPN_E_WORKSPACE; }
    const size_t need = cspn2d_kxk_assemble_workspace_bytes(B, C, sparse_C, H, W, K, history ? 1 : n_iter);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    if (kxk_overlaps(out, vb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {conf, cb}, {history, hb}, {ws, ws_bytes}}) ||
        kxk_overlaps(history, hb, {{guidance, gb}, {blur, vb}, {sparse, sb}, {conf, cb}, {ws, ws_bytes}}) ||
        kxk_overlaps(ws, ws_bytes, {{guidance, gb}, {blur, vb}, {sparse, sb}, {conf, cb}}) ||
        (pin && (kxk_overlaps(out, vb, {{pin->conf, sb}}) || kxk_overlaps(history, hb, {{pin->conf, sb}}) || kxk_overlaps(ws, ws_bytes, {{pin->conf, sb}})))) {
        set_error("%s: out, history and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (pin)
        return kxk_assemble_forward_pin(guidance, dtype, blur, sparse, *pin, conf, steps, T, out, history, B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws,
                                        (hipStream_t)stream);
    if (dilation != 1)
        return kxk_assemble_forward_dil(guidance, dtype, blur, sparse, conf, steps, T, out, history, B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws,
                                        (hipStream_t)stream);
    return kxk_assemble_forward(guidance, dtype, blur, sparse, conf, steps, T, out, history, B, C, sparse_C, H, W, K, n_iter, norm, ws, (hipStream_t)stream);
}

static int kxk_assemble_backward_entry(const char* what, const void* guidance, bool g16, int dtype, const float* blur, const float* sparse, const float* conf,
                                       const int* steps, int T, const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance,
                                       float* grad_blur, float* grad_conf, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                                       size_t ws_bytes, cspn_stream_t stream, int dilation = 1, const KxkPin* pin = nullptr) {
    if (int e = kxk_assemble_check(what, {{"guidance", guidance}, {"blur", blur}, {"conf", conf}, {"steps", steps}, {"grad_out", grad_out}}, sparse, steps, T, B,
                                   C, sparse_C, H, W, K, n_iter, norm))
        return e;
    if (g16)
        if (int e = g16_check(what, dtype, guidance, grad_guidance)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), gb = vb / C * (K * K - 1) / (g16 ? 2 : 1), sb = vb / C * sparse_C, cb = vb / C * T;
    const size_t hb = cspn2d_kxk_assemble_history_bytes(B, C, H, W, K, n_iter);
    float* const grad_sparse = pin ? pin->gs : nullptr;
    float* const grad_pin = pin ? pin->gp : nullptr;
    const bool reads_history = ((grad_guidance || grad_pin) && n_iter >= 2) || grad_conf;   // H_1 .. H_{n-1} for the gates (dL/dpin too), H_{s_j} for the confidences
    if (reads_history && (!history || history_bytes < hb)) {
        set_error("%s: grad_guidance and grad_conf need the forward's history: need %zu bytes, got %zu", what, hb, history ? history_bytes : 0);
        return CSPN_E_BADARG;
    }
    const size_t need = cspn2d_backward_kxk_assemble_workspace_bytes(B, C, sparse_C, H, W, K, n_iter);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t hbu = reads_history ? hb : 0;
    if ((grad_guidance && ((const void*)grad_guidance == (const void*)grad_blur || (const void*)grad_guidance == (const void*)grad_conf)) ||
        (grad_blur && grad_blur == grad_conf)) {
        set_error("%s: grad_guidance, grad_blur and grad_conf must not alias", what);
        return CSPN_E_BADARG;
    }
    const std::initializer_list<std::pair<const void*, size_t>> inputs = {{guidance, gb}, {blur, vb}, {sparse, sb}, {conf, cb}, {history, hbu}, {grad_out, vb}};
    if (kxk_overlaps(grad_guidance, gb, inputs) || kxk_overlaps(grad_blur, vb, inputs) || kxk_overlaps(grad_conf, cb, inputs) || kxk_overlaps(ws, ws_bytes, inputs) ||
        kxk_overlaps(ws, ws_bytes, {{grad_guidance, gb}, {grad_blur, vb}, {grad_conf, cb}}) ||
        kxk_overlaps(grad_guidance, gb, {{grad_blur, vb}, {grad_conf, cb}}) || kxk_overlaps(grad_blur, vb, {{grad_conf, cb}})) {
        set_error("%s: grad_guidance, grad_blur, grad_conf and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (pin) {
        const std::initializer_list<std::pair<const void*, size_t>> all = {{guidance, gb}, {blur, vb}, {sparse, sb}, {pin->conf, sb}, {conf, cb}, {history, hbu},
                                                                           {grad_out, vb}, {grad_guidance, gb}, {grad_blur, vb}, {grad_conf, cb}, {ws, ws_bytes}};
        if (kxk_overlaps(grad_guidance, gb, {{pin->conf, sb}}) || kxk_overlaps(grad_blur, vb, {{pin->conf, sb}}) || kxk_overlaps(grad_conf, cb, {{pin->conf, sb}}) ||
            kxk_overlaps(ws, ws_bytes, {{pin->conf, sb}}) || kxk_overlaps(grad_sparse, sb, all) || kxk_overlaps(grad_pin, sb, all) ||
            kxk_overlaps(grad_sparse, sb, {{grad_pin, sb}})) {
            set_error("%s: grad_sparse, grad_pin, the other gradients and the workspace must not alias an input or each other", what);
            return CSPN_E_BADARG;
        }
    }
    if (!grad_guidance && !grad_blur && !grad_conf && !grad_sparse && !grad_pin) return 0;
    if (pin)
        return kxk_assemble_backward_pin(guidance, dtype, blur, sparse, *pin, conf, steps, T, history, grad_out, grad_guidance, grad_blur, grad_conf, B, C,
                                         sparse_C, H, W, K, dilation, n_iter, norm, ws, (hipStream_t)stream);
    if (dilation != 1)
        return kxk_assemble_backward_dil(guidance, dtype, blur, sparse, conf, steps, T, history, grad_out, grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H,
                                         W, K, dilation, n_iter, norm, ws, (hipStream_t)stream);
    return kxk_assemble_backward(guidance, dtype, blur, sparse, conf, steps, T, history, grad_out, grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W, K,
                                 n_iter, norm, ws, (hipStream_t)stream);
}

int cspn2d_forward_kxk_assemble_f32(const float* guidance, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out,
                                    float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                                    size_t ws_bytes, cspn_stream_t stream) {
    return kxk_assemble_forward_entry("cspn2d_forward_kxk_assemble_f32", guidance, false, 0, blur, sparse, conf, steps, T, out, history, history_bytes, B, C,
                                      sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

int cspn2d_forward_kxk_assemble_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                    float* out, float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm,
                                    void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return kxk_assemble_forward_entry("cspn2d_forward_kxk_assemble_g16", guidance, true, gate_dtype, blur, sparse, conf, steps, T, out, history, history_bytes, B,
                                      C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_assemble_f32(const float* guidance, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                     const float* history, size_t history_bytes, const float* grad_out, float* grad_guidance, float* grad_blur,
                                     float* grad_conf, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, size_t ws_bytes,
                                     cspn_stream_t stream) {
    return kxk_assemble_backward_entry("cspn2d_backward_kxk_assemble_f32", guidance, false, 0, blur, sparse, conf, steps, T, history, history_bytes, grad_out,
                                       grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

int cspn2d_backward_kxk_assemble_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                     const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur,
                                     float* grad_conf, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, size_t ws_bytes,
                                     cspn_stream_t stream) {
    return kxk_assemble_backward_entry("cspn2d_backward_kxk_assemble_g16", guidance, true, gate_dtype, blur, sparse, conf, steps, T, history, history_bytes,
                                       grad_out, grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream);
}

// ---- the dilated forms (cspn2d_*_kxk_{norm,assemble}_dil): the _g16 entry points with dilation behind K and gate_dtype 0 for float32.  The
// dilation is checked first, then every check of the counterpart; dilation 1 runs the counterpart's own instances ----
static int kxk_dilation_check(const char* what, int dilation) {
    if (kxk_dilation_ok(dilation)) return 0;
    set_error("%s: dilation must be 1 or 2, got %d", what, dilation);
    return CSPN_E_BADARG;
}

int cspn2d_forward_kxk_norm_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, float* out, float* history,
                                size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm, void* ws,
                                size_t ws_bytes, cspn_stream_t stream) {
    if (int e = kxk_dilation_check("cspn2d_forward_kxk_norm_dil", dilation)) return e;
    return kxk_norm_forward_entry("cspn2d_forward_kxk_norm_dil", guidance, gate_dtype != 0, gate_dtype, blur, sparse, out, history, history_bytes, B, C, sparse_C,
                                  H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation);
}

int cspn2d_backward_kxk_norm_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* history,
                                 size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur, int B, int C, int sparse_C,
                                 int H, int W, int K, int dilation, int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = kxk_dilation_check("cspn2d_backward_kxk_norm_dil", dilation)) return e;
    return kxk_norm_backward_entry("cspn2d_backward_kxk_norm_dil", guidance, gate_dtype != 0, gate_dtype, blur, sparse, history, history_bytes, grad_out,
                                   grad_guidance, grad_blur, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation);
}

int cspn2d_forward_kxk_assemble_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                    float* out, float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int dilation,
                                    int n_iter, int norm, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (int e = kxk_dilation_check("cspn2d_forward_kxk_assemble_dil", dilation)) return e;
    return kxk_assemble_forward_entry("cspn2d_forward_kxk_assemble_dil", guidance, gate_dtype != 0, gate_dtype, blur, sparse, conf, steps, T, out, history,
                                      history_bytes, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation);
}

int cspn2d_backward_kxk_assemble_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                     const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur,
                                     float* grad_conf, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm, void* ws,
                                     size_t ws_bytes, cspn_stream_t stream) {
    if (int e = kxk_dilation_check("cspn2d_backward_kxk_assemble_dil", dilation)) return e;
    return kxk_assemble_backward_entry("cspn2d_backward_kxk_assemble_dil", guidance, gate_dtype != 0, gate_dtype, blur, sparse, conf, steps, T, history,
                                       history_bytes, grad_out, grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes,
                                       stream, dilation);
}

// ---- the pinned forms (cspn2d_*_kxk_{norm,assemble}_pin): the _dil entry points with pin_conf behind sparse and, in the backwards, grad_sparse and
// grad_pin behind the other gradients.  The pin is checked first (sparse and pin_conf given, sparse_C != 0), then every check of the _dil counterpart ----
static int kxk_pin_check(const char* what, const float* sparse, const float* pin_conf, int sparse_C) {
    if (sparse && pin_conf && sparse_C != 0) return 0;
    set_error("%s: the pin needs sparse and pin_conf (both non-NULL) with sparse_C 1 or C, got sparse %s, pin_conf %s, sparse_C %d", what,
              sparse ? "given" : "NULL", pin_conf ? "given" : "NULL", sparse_C);
    return CSPN_E_BADARG;
}

int cspn2d_forward_kxk_norm_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf, float* out,
                                float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm,
                                void* ws, size_t ws_bytes, cspn_stream_t stream) {
    const char* what = "cspn2d_forward_kxk_norm_pin";
    if (int e = kxk_pin_check(what, sparse, pin_conf, sparse_C)) return e;
    if (int e = kxk_dilation_check(what, dilation)) return e;
    const KxkPin pin{pin_conf, nullptr, nullptr};
    return kxk_norm_forward_entry(what, guidance, gate_dtype != 0, gate_dtype, blur, sparse, out, history, history_bytes, B, C, sparse_C, H, W, K, n_iter, norm,
                                  ws, ws_bytes, stream, dilation, &pin);
}

int cspn2d_backward_kxk_norm_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                 const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur,
                                 float* grad_sparse, float* grad_pin, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm,
                                 void* ws, size_t ws_bytes, cspn_stream_t stream) {
    const char* what = "cspn2d_backward_kxk_norm_pin";
    if (int e = kxk_pin_check(what, sparse, pin_conf, sparse_C)) return e;
    if (int e = kxk_dilation_check(what, dilation)) return e;
    const KxkPin pin{pin_conf, grad_sparse, grad_pin};
    return kxk_norm_backward_entry(what, guidance, gate_dtype != 0, gate_dtype, blur, sparse, history, history_bytes, grad_out, grad_guidance, grad_blur, B, C,
                                   sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation, &pin);
}

int cspn2d_forward_kxk_assemble_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                    const float* conf, const int* steps, int T, float* out, float* history, size_t history_bytes, int B, int C,
                                    int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm, void* ws, size_t ws_bytes,
                                    cspn_stream_t stream) {
    const char* what = "cspn2d_forward_kxk_assemble_pin";
    if (int e = kxk_pin_check(what, sparse, pin_conf, sparse_C)) return e;
    if (int e = kxk_dilation_check(what, dilation)) return e;
    const KxkPin pin{pin_conf, nullptr, nullptr};
    return kxk_assemble_forward_entry(what, guidance, gate_dtype != 0, gate_dtype, blur, sparse, conf, steps, T, out, history, history_bytes, B, C, sparse_C,
                                      H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation, &pin);
}

int cspn2d_backward_kxk_assemble_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                     const float* conf, const int* steps, int T, const float* history, size_t history_bytes, const float* grad_out,
                                     void* grad_guidance, float* grad_blur, float* grad_conf, float* grad_sparse, float* grad_pin, int B, int C,
                                     int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm, void* ws, size_t ws_bytes,
                                     cspn_stream_t stream) {
    const char* what = "cspn2d_backward_kxk_assemble_pin";
    if (int e = kxk_pin_check(what, sparse, pin_conf, sparse_C)) return e;
    if (int e = kxk_dilation_check(what, dilation)) return e;
    const KxkPin pin{pin_conf, grad_sparse, grad_pin};
    return kxk_assemble_backward_entry(what, guidance, gate_dtype != 0, gate_dtype, blur, sparse, conf, steps, T, history, history_bytes, grad_out,
                                       grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream, dilation, &pin);
}

// ---- non-local propagation with learned offsets (cspn2d_nl.hip): K = 3 only; the error rules of the cspn2d_*_kxk_f32 entry points ----
static bool nl_shape_ok(int B, int C, int H, int W, int K, int n_iter) {
    return B > 0 && C > 0 && H > 0 && W > 0 && K == 3 && n_iter >= 0 && (long long)B * C * H * W <= 0x7fffffffLL &&
           (long long)B * 2 * (K * K - 1) * H * W <= 0x7fffffffLL;
}

static int nl_check_shape(const char* what, int B, int C, int H, int W, int K, int n_iter) {
    if (K != 3) { set_error("%s: K must be 3 (5 and 7 are not built), got %d", what, K); return CSPN_E_UNSUPPORTED; }
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d H=%d W=%d", what, B, C, H, W); return CSPN_E_BADARG; }
    if (n_iter < 0) { set_error("%s: n_iter must be >= 0 (got %d)", what, n_iter); return CSPN_E_BADARG; }
    if (!nl_shape_ok(B, C, H, W, K, n_iter)) { set_error("%s: tensor too large for 32-bit element indexing", what); return CSPN_E_UNSUPPORTED; }
    return 0;
}

static size_t nl_level_bytes(int B, int C, int H, int W) { return sizeof(float) * kxk_level_floats((size_t)B * C * H * W); }

size_t cspn2d_nl_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse) {
    if (!nl_shape_ok(B, C, H, W, K, n_iter)) return 0;
    return nl_level_bytes(B, C, H, W) * (size_t)nl_forward_levels(n_iter, has_sparse != 0);
}

size_t cspn2d_nl_history_bytes(int B, int C, int H, int W, int K, int n_iter) {
    if (!nl_shape_ok(B, C, H, W, K, n_iter) || n_iter < 2) return 0;
    return kxk_values_bytes(B, C, H, W) * (size_t)(n_iter - 1);
}

size_t cspn2d_backward_nl_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse) {
    if (!nl_shape_ok(B, C, H, W, K, n_iter)) return 0;
    return nl_level_bytes(B, C, H, W) * (size_t)nl_backward_levels(n_iter, has_sparse != 0);
}

// the storage types of aff and offset (the *_g16 twins; 0, 0 from the float32 entry points): the last of the checks.  tensors16: every tensor
// stored in those types, NULL where absent
static int nl_dtype_check(const char* what, int aff_dtype, int offset_dtype, std::initializer_list<const void*> aff16,
                          std::initializer_list<const void*> offset16) {
    for (int dt : {aff_dtype, offset_dtype})
        if (dt != 0 && dt != CSPN_DTYPE_F16 && dt != CSPN_DTYPE_BF16) {
            set_error("%s: a dtype code must be 0 (float32), CSPN_DTYPE_F16 (1) or CSPN_DTYPE_BF16 (2), got %d", what, dt);
            return CSPN_E_BADARG;
        }
    if (offset_dtype == 0 ? aff_dtype != 0 : (aff_dtype != 0 && aff_dtype != offset_dtype)) {
        set_error("%s: dtype pair (aff %d, offset %d) is not built: (0, 0), (0, T) and (T, T) are, T = 1 (fp16) or 2 (bf16)", what, aff_dtype, offset_dtype);
        return CSPN_E_UNSUPPORTED;
    }
    uintptr_t bits = 0;
    if (aff_dtype != 0) for (const void* t : aff16) bits |= (uintptr_t)t;
    if (offset_dtype != 0) for (const void* t : offset16) bits |= (uintptr_t)t;
    if (bits & 1u) { set_error("%s: a 16-bit tensor must be 2-byte aligned", what); return CSPN_E_BADARG; }
    return 0;
}

// cspn2d_forward_nl_f32 and its _g16 twin: one set of checks; the dtypes size the ranges of aff and offset and are checked last
static int nl_forward_entry(const char* what, const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse,
                            float* out, float* history, size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes,
                            cspn_stream_t stream) {
    if (!aff || !offset || !x || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = nl_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), sb = sparse ? vb / C : 0;
    const size_t ab = vb / C / sizeof(float) * (K * K - 1) * gate_bytes(aff_dtype), ob = vb / C / sizeof(float) * 2 * (K * K - 1) * gate_bytes(offset_dtype);
    const size_t hb = cspn2d_nl_history_bytes(B, C, H, W, K, n_iter);
    if (history && history_bytes < hb) { set_error("%s: history buffer too small: need %zu bytes, got %zu", what, hb, history_bytes); return CSPN_E_WORKSPACE; }
    // with a history the levels go there: the workspace keeps the pinned H_0 alone (the n_iter = 1 count)
    const size_t need = cspn2d_nl_workspace_bytes(B, C, H, W, K, history && n_iter > 1 ? 1 : n_iter, sparse != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0;
    if (kxk_overlaps(out, vb, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {history, hb}, {ws, wb}}) ||
        kxk_overlaps(history, hb, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}})) {
        set_error("%s: out, history and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (int e = nl_dtype_check(what, aff_dtype, offset_dtype, {aff}, {offset})) return e;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) return identity_copy(out, x, vb / sizeof(float), st);
    return nl_forward(aff, aff_dtype, offset, offset_dtype, x, sparse, out, history, B, C, H, W, K, n_iter, ws, st);
}

int cspn2d_forward_nl_f32(const float* aff, const float* offset, const float* x, const float* sparse, float* out, float* history,
                          size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_forward_entry("cspn2d_forward_nl_f32", aff, 0, offset, 0, x, sparse, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_forward_nl_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse, float* out,
                          float* history, size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes,
                          cspn_stream_t stream) {
    return nl_forward_entry("cspn2d_forward_nl_g16", aff, aff_dtype, offset, offset_dtype, x, sparse, out, history, history_bytes, B, C, H, W, K, n_iter, ws,
                            ws_bytes, stream);
}

// the index of the deterministic backwards behind the levels (cspn_common.h: NlDetIndex); has_c: the propagation's (with the plane c)
static size_t nl_det_index_bytes(int B, int H, int W, bool has_c) { return NlDetIndex((size_t)B * H * W, has_c).bytes; }

size_t cspn2d_backward_nl_det_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse) {
    if (!nl_shape_ok(B, C, H, W, K, n_iter) || n_iter == 0) return 0;   // n_iter 0: the identity, no adjoint step and no index
    return cspn2d_backward_nl_workspace_bytes(B, C, H, W, K, n_iter, has_sparse) + nl_det_index_bytes(B, H, W, true);
}

size_t cspn2d_nl_sample_backward_det_workspace_bytes(int B, int H, int W, int K) {
    if (!nl_shape_ok(B, 1, H, W, K, 0)) return 0;
    return nl_det_index_bytes(B, H, W, false);
}

// cspn2d_backward_nl_f32, its deterministic twin and their _g16 twins: one set of checks, det picks the workspace and the adjoint; the dtypes
// size the ranges of aff, offset and their gradients and are checked last
static int nl_backward_entry(const char* what, bool det, const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x,
                             const float* sparse, const float* history, size_t history_bytes, const float* grad_out, void* grad_aff, void* grad_offset,
                             float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (!aff || !offset || !x || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = nl_check_shape(what, B, C, H, W, K, n_iter)) return e;
    const size_t vb = kxk_values_bytes(B, C, H, W), sb = sparse ? vb / C : 0;
    const size_t ab = vb / C / sizeof(float) * (K * K - 1) * gate_bytes(aff_dtype), ob = vb / C / sizeof(float) * 2 * (K * K - 1) * gate_bytes(offset_dtype);
    const size_t hb = cspn2d_nl_history_bytes(B, C, H, W, K, n_iter);
    const bool gates = grad_aff || grad_offset;
    if (gates && hb && (!history || history_bytes < hb)) {
        set_error("%s: grad_aff and grad_offset need the forward's history: need %zu bytes, got %zu", what, hb, history ? history_bytes : 0);
        return CSPN_E_BADARG;
    }
    const size_t need = det ? cspn2d_backward_nl_det_workspace_bytes(B, C, H, W, K, n_iter, sparse != nullptr)
                            : cspn2d_backward_nl_workspace_bytes(B, C, H, W, K, n_iter, sparse != nullptr);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0, hbu = gates ? hb : 0;
    if (kxk_overlaps(grad_aff, ab, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}, {grad_offset, ob}, {grad_x, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_offset, ob, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}, {grad_x, vb}, {ws, wb}}) ||
        kxk_overlaps(grad_x, vb, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{aff, ab}, {offset, ob}, {x, vb}, {sparse, sb}, {history, hbu}, {grad_out, vb}})) {
        set_error("%s: grad_aff, grad_offset, grad_x and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (int e = nl_dtype_check(what, aff_dtype, offset_dtype, {aff, grad_aff}, {offset, grad_offset})) return e;
    if (!gates && !grad_x) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_iter == 0) {   // the identity: dL/dx = dL/dout, neither aff nor offset is read
        hipError_t e = grad_x ? hipMemcpyAsync(grad_x, grad_out, vb, hipMemcpyDeviceToDevice, st) : hipSuccess;
        if (e == hipSuccess && grad_aff) e = hipMemsetAsync(grad_aff, 0, ab, st);
        if (e == hipSuccess && grad_offset) e = hipMemsetAsync(grad_offset, 0, ob, st);
        if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); return (int)e; }
        return 0;
    }
    return (det ? nl_backward_det : nl_backward)(aff, aff_dtype, offset, offset_dtype, x, sparse, history, grad_out, grad_aff, grad_offset, grad_x, B, C, H, W,
                                                 K, n_iter, ws, st);
}

int cspn2d_backward_nl_f32(const float* aff, const float* offset, const float* x, const float* sparse, const float* history, size_t history_bytes,
                           const float* grad_out, float* grad_aff, float* grad_offset, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                           void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_backward_entry("cspn2d_backward_nl_f32", false, aff, 0, offset, 0, x, sparse, history, history_bytes, grad_out, grad_aff, grad_offset, grad_x, B,
                             C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_nl_det_f32(const float* aff, const float* offset, const float* x, const float* sparse, const float* history, size_t history_bytes,
                               const float* grad_out, float* grad_aff, float* grad_offset, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                               void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_backward_entry("cspn2d_backward_nl_det_f32", true, aff, 0, offset, 0, x, sparse, history, history_bytes, grad_out, grad_aff, grad_offset, grad_x,
                             B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_nl_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse, const float* history,
                           size_t history_bytes, const float* grad_out, void* grad_aff, void* grad_offset, float* grad_x, int B, int C, int H, int W, int K,
                           int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_backward_entry("cspn2d_backward_nl_g16", false, aff, aff_dtype, offset, offset_dtype, x, sparse, history, history_bytes, grad_out, grad_aff,
                             grad_offset, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

int cspn2d_backward_nl_det_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse,
                               const float* history, size_t history_bytes, const float* grad_out, void* grad_aff, void* grad_offset, float* grad_x, int B,
                               int C, int H, int W, int K, int n_iter, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_backward_entry("cspn2d_backward_nl_det_g16", true, aff, aff_dtype, offset, offset_dtype, x, sparse, history, history_bytes, grad_out, grad_aff,
                             grad_offset, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream);
}

// the sampling operator and its two backwards, with their _g16 twins: offset_dtype sizes the ranges of offset and grad_offset, and is checked last
static int nl_sample_entry(const char* what, const void* offset, int offset_dtype, const float* f, float* out, int B, int H, int W, int K,
                           cspn_stream_t stream) {
    if (!offset || !f || !out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = nl_check_shape(what, B, 1, H, W, K, 0)) return e;
    const size_t fb = kxk_values_bytes(B, 1, H, W), kb = fb * (K * K - 1), ob = kb / sizeof(float) * 2 * gate_bytes(offset_dtype);
    if (kxk_overlaps(out, kb, {{offset, ob}, {f, fb}})) { set_error("%s: out must not alias an input", what); return CSPN_E_BADARG; }
    if (int e = nl_dtype_check(what, 0, offset_dtype, {}, {offset})) return e;
    return nl_sample(offset, offset_dtype, f, out, B, H, W, K, (hipStream_t)stream);
}

int cspn2d_nl_sample_f32(const float* offset, const float* f, float* out, int B, int H, int W, int K, cspn_stream_t stream) {
    return nl_sample_entry("cspn2d_nl_sample_f32", offset, 0, f, out, B, H, W, K, stream);
}

int cspn2d_nl_sample_g16(const void* offset, int offset_dtype, const float* f, float* out, int B, int H, int W, int K, cspn_stream_t stream) {
    return nl_sample_entry("cspn2d_nl_sample_g16", offset, offset_dtype, f, out, B, H, W, K, stream);
}

static int nl_sample_backward_entry(const char* what, const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f,
                                    void* grad_offset, int B, int H, int W, int K, cspn_stream_t stream) {
    if (!offset || !f || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = nl_check_shape(what, B, 1, H, W, K, 0)) return e;
    const size_t fb = kxk_values_bytes(B, 1, H, W), kb = fb * (K * K - 1), ob = kb / sizeof(float) * 2 * gate_bytes(offset_dtype);
    if (kxk_overlaps(grad_f, fb, {{offset, ob}, {f, fb}, {grad_out, kb}, {grad_offset, ob}}) ||
        kxk_overlaps(grad_offset, ob, {{offset, ob}, {f, fb}, {grad_out, kb}})) {
        set_error("%s: grad_f and grad_offset must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (int e = nl_dtype_check(what, 0, offset_dtype, {}, {offset, grad_offset})) return e;
    if (!grad_f && !grad_offset) return 0;
    return nl_sample_backward(offset, offset_dtype, f, grad_out, grad_f, grad_offset, B, H, W, K, (hipStream_t)stream);
}

int cspn2d_nl_sample_backward_f32(const float* offset, const float* f, const float* grad_out, float* grad_f, float* grad_offset, int B, int H, int W,
                                  int K, cspn_stream_t stream) {
    return nl_sample_backward_entry("cspn2d_nl_sample_backward_f32", offset, 0, f, grad_out, grad_f, grad_offset, B, H, W, K, stream);
}

int cspn2d_nl_sample_backward_g16(const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f, void* grad_offset, int B,
                                  int H, int W, int K, cspn_stream_t stream) {
    return nl_sample_backward_entry("cspn2d_nl_sample_backward_g16", offset, offset_dtype, f, grad_out, grad_f, grad_offset, B, H, W, K, stream);
}

static int nl_sample_backward_det_entry(const char* what, const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f,
                                        void* grad_offset, int B, int H, int W, int K, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    if (!offset || !f || !grad_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = nl_check_shape(what, B, 1, H, W, K, 0)) return e;
    const size_t fb = kxk_values_bytes(B, 1, H, W), kb = fb * (K * K - 1), ob = kb / sizeof(float) * 2 * gate_bytes(offset_dtype);
    const size_t need = cspn2d_nl_sample_backward_det_workspace_bytes(B, H, W, K);
    if (int e = kxk_check_ws(what, ws, ws_bytes, need)) return e;
    const size_t wb = need ? ws_bytes : 0;
    if (kxk_overlaps(grad_f, fb, {{offset, ob}, {f, fb}, {grad_out, kb}, {grad_offset, ob}, {ws, wb}}) ||
        kxk_overlaps(grad_offset, ob, {{offset, ob}, {f, fb}, {grad_out, kb}, {ws, wb}}) ||
        kxk_overlaps(ws, wb, {{offset, ob}, {f, fb}, {grad_out, kb}})) {
        set_error("%s: grad_f, grad_offset and the workspace must not alias an input or each other", what);
        return CSPN_E_BADARG;
    }
    if (int e = nl_dtype_check(what, 0, offset_dtype, {}, {offset, grad_offset})) return e;
    if (!grad_f && !grad_offset) return 0;
    return nl_sample_backward_det(offset, offset_dtype, f, grad_out, grad_f, grad_offset, B, H, W, K, ws, (hipStream_t)stream);
}

int cspn2d_nl_sample_backward_det_f32(const float* offset, const float* f, const float* grad_out, float* grad_f, float* grad_offset, int B, int H, int W,
                                      int K, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_sample_backward_det_entry("cspn2d_nl_sample_backward_det_f32", offset, 0, f, grad_out, grad_f, grad_offset, B, H, W, K, ws, ws_bytes, stream);
}

int cspn2d_nl_sample_backward_det_g16(const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f, void* grad_offset, int B,
                                      int H, int W, int K, void* ws, size_t ws_bytes, cspn_stream_t stream) {
    return nl_sample_backward_det_entry("cspn2d_nl_sample_backward_det_g16", offset, offset_dtype, f, grad_out, grad_f, grad_offset, B, H, W, K, ws, ws_bytes,
                                        stream);
}

// ---- the guidance heads for K x K propagation (cspn_head_kxk.hip); K = 3 is the 8-plane head's own entry points ----
static int head_kxk_check(const char* what, int B, int C, int h, int w, int H, int W, int K) {
    if (K != 3 && K != 5 && K != 7) { set_error("%s: K must be 3, 5 or 7, got %d", what, K); return CSPN_E_BADARG; }
    if (B < 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) { set_error("%s: bad shape B=%d C=%d h=%d w=%d H=%d W=%d", what, B, C, h, w, H, W); return CSPN_E_BADARG; }
    if (H > 2 * h || W > 2 * w) { set_error("%s: H x W = %d x %d exceeds the unpooled %d x %d", what, H, W, 2 * h, 2 * w); return CSPN_E_BADARG; }
    return 0;
}

static int head_kxk_check_ws(const char* what, const void* ws, size_t ws_bytes, size_t need) {
    if (!ws || ws_bytes < need || ((uintptr_t)ws & 255u) != 0) { set_error("%s: workspace: need %zu bytes, 256-byte aligned", what, need); return CSPN_E_WORKSPACE; }
    return 0;
}

static bool head_kxk_too_large(int B, int C, int h, int w, int H, int W, int K) {
    return (long long)B * (K * K - 1) * H * W >= (1ll << 40) || (long long)C * h * w >= (1ll << 31) || (long long)(K * K - 1) * H * W >= (1ll << 31);
}

// ---- one set of checks for the six head entry points below.  t16: how many of the call's tensors are 16-bit -- 0: none (the float32 heads, dtype unused);
// 1: x and dL/dx (the 8-plane head on fp16 / bf16 feature maps, float32 guidance: cspn_head_g16.hip; K = 3 stands for it); 2: the guidance and its gradient too
// (K = 5 or 7: cspn_head_kxk_g16.hip) ----
static int head_check_16(const char* what, int t16, int dtype, std::initializer_list<const void*> tensors16) {
    if (!t16) return 0;
    if (dtype != CSPN_DTYPE_F16 && dtype != CSPN_DTYPE_BF16) {
        set_error("%s: dtype must be CSPN_DTYPE_F16 (1) or CSPN_DTYPE_BF16 (2), got %d", what, dtype);
        return CSPN_E_BADARG;
    }
    for (const void* p : tensors16)
        if ((uintptr_t)p & 1u) { set_error("%s: a 16-bit tensor must be 2-byte aligned", what); return CSPN_E_BADARG; }
    return 0;
}

// the forward's checks -> an error, 0 to launch, 1 when there is nothing to do (an empty batch), 2 for the float32 heads at K = 3: the 8-plane head's own entry
// point takes over from here (ahead of the size test, which is stricter than its own)
static int head_forward_check(const char* what, const void* x, int t16, int dtype, const float* w_guidance, const float* w_blur, const void* guidance_out,
                              const float* blur_out, int B, int C, int h, int w, int H, int W, int K, const void* ws, size_t ws_bytes, size_t need) {
    if (!x || !w_guidance || !guidance_out) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = head_check_16(what, t16, dtype, {x, t16 == 2 ? guidance_out : nullptr})) return e;
    if (int e = head_kxk_check(what, B, C, h, w, H, W, K)) return e;
    if ((w_blur != nullptr) != (blur_out != nullptr)) { set_error("%s: w_blur and blur_out come together", what); return CSPN_E_BADARG; }
    if (int e = head_kxk_check_ws(what, ws, ws_bytes, need)) return e;
    if (!t16 && K == 3) return 2;
    if (head_kxk_too_large(B, C, h, w, H, W, K)) { set_error("%s: tensor too large", what); return CSPN_E_UNSUPPORTED; }
    return B == 0 ? 1 : 0;
}

// the backward's checks -> as the forward's; nothing to do: an empty batch, no output asked for
static int head_backward_check(const char* what, const void* x, int t16, int dtype, const float* w_guidance, const float* w_blur, const void* grad_guidance,
                               const float* grad_blur, const void* grad_x, const float* grad_w_guidance, const float* grad_w_blur, int B, int C, int h, int w,
                               int H, int W, int K, const void* ws, size_t ws_bytes, size_t need) {
    if (!x || !w_guidance || !grad_guidance) { set_error("%s: null pointer", what); return CSPN_E_BADARG; }
    if (int e = head_check_16(what, t16, dtype, {x, t16 == 2 ? grad_guidance : nullptr, grad_x})) return e;
    if (int e = head_kxk_check(what, B, C, h, w, H, W, K)) return e;
    if ((w_blur != nullptr) != (grad_blur != nullptr)) { set_error("%s: w_blur and grad_blur come together", what); return CSPN_E_BADARG; }
    if (grad_w_blur && !w_blur) { set_error("%s: grad_w_blur without a blur head", what); return CSPN_E_BADARG; }
    if (B == 0 || (!grad_x && !grad_w_guidance && !grad_w_blur)) return 1;
    if (int e = head_kxk_check_ws(what, ws, ws_bytes, need)) return e;
    if (!t16 && K == 3) return 2;
    if (head_kxk_too_large(B, C, h, w, H, W, K)) { set_error("%s: tensor too large", what); return CSPN_E_UNSUPPORTED; }
    return 0;
}

size_t cspn_guidance_head_kxk_workspace_bytes(int B, int C, int h, int w, int K) {
    (void)B; (void)h; (void)w;
    if (C <= 0) return 0;
    return K == 3 ? cspn_guidance_head_workspace_bytes(C) : ((K == 5 || K == 7) ? head_kxk_workspace(C, K) : 0);
}

int cspn_guidance_head_kxk_f32(const float* x, const float* w_guidance, const float* w_blur, float* guidance_out, float* blur_out, int B, int C, int h, int w,
                               int H, int W, int K, void* workspace, size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_kxk_f32";
    int e = head_forward_check(what, x, 0, 0, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, K, workspace, workspace_bytes,
                               cspn_guidance_head_kxk_workspace_bytes(B, C, h, w, K));
    if (e == 2) return cspn_guidance_head_f32(x, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, CSPN_NORM_NONE, workspace, workspace_bytes, stream);
    if (e) return e < 0 ? e : 0;
    return head_kxk_forward(x, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, K, workspace, (hipStream_t)stream);
}

size_t cspn_guidance_head_kxk_backward_workspace_bytes(int B, int C, int h, int w, int K) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    return K == 3 ? cspn_guidance_head_backward_workspace_bytes(B, C, h, w) : ((K == 5 || K == 7) ? head_kxk_backward_workspace(B, C, h, w, K) : 0);
}

int cspn_guidance_head_kxk_backward_f32(const float* x, const float* w_guidance, const float* w_blur, const float* grad_guidance, const float* grad_blur,
                                        float* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w, int H, int W, int K,
                                        void* workspace, size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_kxk_backward_f32";
    int e = head_backward_check(what, x, 0, 0, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H, W, K, workspace,
                                workspace_bytes, cspn_guidance_head_kxk_backward_workspace_bytes(B, C, h, w, K));
    if (e == 2)
        return cspn_guidance_head_backward_f32(x, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H, W, workspace,
                                               workspace_bytes, stream);
    if (e) return e < 0 ? e : 0;
    return head_kxk_backward(x, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H, W, K, workspace,
                             (hipStream_t)stream);
}

// ---- the heads on fp16 / bf16 feature maps with 16-bit guidance, K = 5 or 7 (cspn_head_kxk_g16.hip) ----
static int head_kxk_g16_check_K(const char* what, int K) {
    if (K != 5 && K != 7) { set_error("%s: K must be 5 or 7 (the 8-plane head of K = 3 is float32 only), got %d", what, K); return CSPN_E_BADARG; }
    return 0;
}

size_t cspn_guidance_head_kxk_g16_workspace_bytes(int B, int C, int h, int w, int K) {
    (void)B; (void)h; (void)w;
    return (C > 0 && (K == 5 || K == 7)) ? head_kxk_g16_workspace(C, K) : 0;
}

int cspn_guidance_head_kxk_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, void* guidance_out, float* blur_out, int B, int C, int h,
                               int w, int H, int W, int K, void* workspace, size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_kxk_g16";
    if (int e = head_kxk_g16_check_K(what, K)) return e;
    if (int e = head_forward_check(what, x, 2, dtype, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, K, workspace, workspace_bytes,
                                   cspn_guidance_head_kxk_g16_workspace_bytes(B, C, h, w, K)))
        return e < 0 ? e : 0;
    return head_kxk_g16_forward(x, dtype, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, K, workspace, (hipStream_t)stream);
}

size_t cspn_guidance_head_kxk_backward_g16_workspace_bytes(int B, int C, int h, int w, int K) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    return (K == 5 || K == 7) ? head_kxk_g16_backward_workspace(B, C, h, w, K) : 0;
}

int cspn_guidance_head_kxk_backward_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, const void* grad_guidance,
                                        const float* grad_blur, void* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w, int H,
                                        int W, int K, void* workspace, size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_kxk_backward_g16";
    if (int e = head_kxk_g16_check_K(what, K)) return e;
    if (int e = head_backward_check(what, x, 2, dtype, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H,
                                    W, K, workspace, workspace_bytes, cspn_guidance_head_kxk_backward_g16_workspace_bytes(B, C, h, w, K)))
        return e < 0 ? e : 0;
    return head_kxk_g16_backward(x, dtype, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H, W, K, workspace,
                                 (hipStream_t)stream);
}

// ---- the 8-plane head + the blur head on an fp16 / bf16 feature map, guidance and blur float32: what feeds the 3 x 3 rings (cspn_head_g16.hip) ----
size_t cspn_guidance_head_g16_workspace_bytes(int B, int C, int h, int w) {
    (void)B; (void)h; (void)w;
    return C > 0 ? head_g16_workspace(C) : 0;
}

int cspn_guidance_head_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, float* guidance_out, float* blur_out, int B, int C, int h,
                           int w, int H, int W, void* workspace, size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_g16";
    if (int e = head_forward_check(what, x, 1, dtype, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, 3, workspace, workspace_bytes,
                                   cspn_guidance_head_g16_workspace_bytes(B, C, h, w)))
        return e < 0 ? e : 0;
    return head_g16_forward(x, dtype, w_guidance, w_blur, guidance_out, blur_out, B, C, h, w, H, W, workspace, (hipStream_t)stream);
}

size_t cspn_guidance_head_backward_g16_workspace_bytes(int B, int C, int h, int w) {
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    return head_g16_backward_workspace(B, C, h, w);
}

int cspn_guidance_head_backward_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, const float* grad_guidance, const float* grad_blur,
                                    void* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w, int H, int W, void* workspace,
                                    size_t workspace_bytes, cspn_stream_t stream) {
    static const char* what = "cspn_guidance_head_backward_g16";
    if (int e = head_backward_check(what, x, 1, dtype, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H,
                                    W, 3, workspace, workspace_bytes, cspn_guidance_head_backward_g16_workspace_bytes(B, C, h, w)))
        return e < 0 ? e : 0;
    return head_g16_backward(x, dtype, w_guidance, w_blur, grad_guidance, grad_blur, grad_x, grad_w_guidance, grad_w_blur, B, C, h, w, H, W, workspace,
                             (hipStream_t)stream);
}

}  // extern "C"
