// cspn_common.h -- shared declarations of libcspn_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cspn_amd.h"

namespace cspn {

// Neighbour offsets of the eight affinity channels, derived from the ZeroPad2d
// tuples at reference cspn_pytorch/models/cspn.py:105-128 (dy = 1-top, dx = 1-left):
// channel k couples output pixel p with neighbour p + (DY[k], DX[k]), and -- because
// the reference pads the affinity planes with the SAME tuples as the depth
// (cspn.py:149-167) -- its weight is read AT THE NEIGHBOUR ("neighbour-sited").
__host__ __device__ constexpr int dy2(int k) { return k < 3 ? 1 : (k < 5 ? 0 : -1); }
__host__ __device__ constexpr int dx2(int k) {
    return (k == 0 || k == 3 || k == 5) ? 1 : ((k == 1 || k == 6) ? 0 : -1);
}

// sign() of reference cspn.py:64 (NaN stays NaN like torch.sign -> here NaN compares false -> s itself)
__device__ __forceinline__ float signf(float s) { return s > 0.f ? 1.f : (s < 0.f ? -1.f : s); }

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// CUs of the current device (queried once per device and kept: idempotent memoisation, no other state)
int num_cus();

// ---- stepwise path (one launch per iteration; general shapes) ----
size_t stepwise2d_workspace(int B, int H, int W, int n_iter);
int stepwise2d_forward(const float* g, const float* blur, const float* sparse, float* out, int B, int H, int W,
                       int n_iter, int norm, void* ws, hipStream_t st);
// reference affinity_normalization (cspn.py:85-144) as a stand-alone kernel: g [B,8,H,W] -> gate_wb [B,8,H,W] (norm 8SUM / 8SUM_ABS)
int normalize2d(const float* g, float* wb, int B, int H, int W, int norm, hipStream_t st);
// its adjoint (cspn2d_normalize_backward.hip): g [B,8,H,W] raw, gwb = dL/dgate_wb [B,8,H,W] -> gg = dL/dg [B,8,H,W]
int normalize2d_backward(const float* g, const float* gwb, float* gg, int B, int H, int W, int norm, hipStream_t st);
// W % 4 != 0: the fused path on rows padded to a multiple of 4 columns (cspn2d_stepwise.hip)
bool padded2d_supported(int B, int H, int W, int n_iter);
size_t padded2d_workspace(int B, int H, int W, int n_iter);
int padded2d_forward(const float* g, const float* blur, const float* sparse, float* out, int B, int H, int W, int n_iter, int norm, void* ws,
                     hipStream_t st);
size_t stepwise3d_workspace(int B, int D, int H, int W, int n_iter);
// gdt (here and below): the storage type of the gates, 0 float32 or CSPN_DTYPE_F16 / CSPN_DTYPE_BF16 (stepwise3d_forward: every mode, the
// normalising and masked ones through fold3d_kernel; the persistent entry points: the Paddle contract only, norm NONE and no mask); 16-bit
// gates are widened exactly where they are read (cspn_gate16.h), every value, level and workspace stays float32
int stepwise3d_forward(const void* g, const float* feat, const float* sparse, float* out, int B, int D, int H,
                       int W, int n_iter, int norm, void* ws, hipStream_t st, int algo = 0, int gdt = 0);
// one step of the Paddle contract (W % 4 == 0, 16-byte aligned values, gates aligned to four elements); cp != NULL (float32 gates only):
// hout = cp + that step, the step of the normalising / masked backward on its folded planes (g = w' [B][26][V], cp = c' [B][V])
int step3d_direct(const void* g, int gdt, const float* hin, float* hout, int B, int D, int H, int W, hipStream_t st, const float* cp = nullptr);
// the same step on a gate tensor of any shape and alignment, one voxel a thread (no constant term); fbs: floats from one volume of hin /
// hout to the next.  It skips the taps outside the volume where the others multiply by zero (cspn3d_stepwise.hip)
int step3d_scalar(const void* g, int gdt, const float* hin, float* hout, int B, int D, int H, int W, size_t fbs, hipStream_t st);
// one step on folded planes, one voxel a thread: hout = c + sum_k w_k hin(p + off_k), w_k(p) of batch b at w + b bs + k ps + r, c [B][V]
int step3d_folded(const float* w, const float* c, size_t bs, size_t ps, const float* hin, float* hout, int B, int D, int H, int W, hipStream_t st);
size_t forward3d_workspace(int B, int D, int H, int W, int n_iter, int norm, bool has_sparse);

// ---- 3D, gates resident in registers for all steps (cspn3d_persistent.hip); Paddle contract only ----
bool persistent3d_supported(int B, int D, int H, int W, int n_iter);
size_t persistent3d_workspace(int B, int D, int H, int W);
int persistent3d_forward(const void* gate, const float* feat, float* out, int B, int D, int H, int W, int n_iter, void* ws,
                         hipStream_t st, int gdt = 0);
// the folded form of the normalising / masked modes: wf = 26 planes w' + the constant term c' ([27][B*V], fold3d_kernel)
int persistent3d_forward_folded(const float* wf, const float* feat, float* out, int B, int D, int H, int W, int n_iter, void* ws,
                                hipStream_t st);
// launch options only the test-hook library sets (csrc/cspn_test_hooks.hip): mute = the workgroup that never publishes its
// boundary (its neighbours then run into the poll timeout), coop = hipLaunchCooperativeKernel instead of the event chain
struct P3Options { int mute = -1; bool coop = false; bool placement = true; /* false: tiles in plain workgroup order (A/B of the XCD-aware placement) */
                   bool write_through = false; /* true: no L2-resident stores, every published row goes write-through (A/B, tests) */ };
// the same run for the backward: adjoint = transposed operator; levels + (lv0 + it * lvs) volumes receive step it < n_iter
// C > 1: feat / out / the level volumes hold C value channels per volume ([B][C][V]) on shared gates (the MULTI instantiations)
// gdt != 0: the forward instances only (the transposed one reads float32 gates)
int persistent3d_run(const void* gate, const float* feat, float* out, float* levels, int lv0, int lvs, bool adjoint, int B, int D,
                     int H, int W, int n_iter, void* ws, hipStream_t st, const P3Options& opt = P3Options(), int C = 1, int gdt = 0);
int persistent3d_error_word(const void* ws, int B, int D, int H, int W);
void persistent3d_geo(int B, int D, int H, int W, int n_iter, int* info);   // (test-hook library)
// C value channels per volume that share the gates ([B][C][V] value tensors, [B][26][V] gates used as given)
bool persistent3d_multi_supported(int B, int C, int D, int H, int W, int n_iter);
int persistent3d_forward_multi(const void* gate, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter, void* ws,
                               hipStream_t st, int gdt = 0);

// the demo's module on RAW gates (NRM instantiation): each voxel's 26 gates divided by their abs-sum in the registers, then the n_iter
// steps of persistent3d_forward; same calls as persistent3d_supported
int persistent3d_forward_absnorm(const void* guide, const float* feat, float* out, int B, int D, int H, int W, int n_iter, void* ws,
                                 hipStream_t st, int gdt = 0);

// sticky per-device status of the persistent launches: != 0 once after a launch gave up (a workgroup waited in vain for a
// neighbour: not all workgroups resident); read without synchronisation from a pinned host word, cleared by the read
int persistent3d_take_status();

// ---- the demo's gate normalisation (cspn_gate_norm.hip): guide [N][K][V] -> w_k = |g_k| / sum_j |g_j|, and its adjoint; K = 8, 24, 26
// or 48 ----
int gate_absnorm(const float* g, float* w, int N, int K, size_t V, hipStream_t st);
int gate_absnorm_backward(const float* g, const float* gw, float* gg, int N, int K, size_t V, hipStream_t st);
// the 3D module's forms on an fp16 / bf16 guide (K = 26; gdt CSPN_DTYPE_F16 or CSPN_DTYPE_BF16): the guide widened exactly as it is read, w
// and dL/dw float32, dL/dguide the float32 value rounded once at its store -- the float32 kernels' arithmetic, statement for statement
int gate_absnorm_g16(const void* g, int gdt, float* w, int N, size_t V, hipStream_t st);
int gate_absnorm_backward_g16(const void* g, int gdt, const float* gw, void* gg, int N, size_t V, hipStream_t st);

// ---- the 2D NONE op over a K x K neighbourhood, K = 5 or 7 (cspn2d_kxk.hip): gate [N][K*K-1][H][W], values [N][C][H][W] ----
// gate and gg in the type of dtype: 0 (float32), CSPN_DTYPE_F16 or CSPN_DTYPE_BF16.  A 16-bit gate is widened exactly where it is used
// (bitwise the float32 results on the widened gates); a 16-bit gg is the float32 sum rounded once at its store
// absnorm: the demo module's contract (cspn_paddle/demo.py:20-54) inside the same engine: gate is the raw guide, a_k = |g_k|,
// S = sum_k a_k per pixel, H_{t+1} = (sum_k a_k H_t(p + off_k)) / S; gg = dL/dguide
// a workspace part's bytes, rounded so that the part behind it stays 256-byte aligned
inline size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// a level of the forward's ping-pong workspace, rounded to 64 floats so that both levels stay 256-byte aligned
inline size_t kxk_level_floats(size_t L) { return (L + 63) & ~(size_t)63; }
// hist: NULL (the levels ping-pong in ws: 2 levels of kxk_level_floats) or H_1 .. H_{n-1}, level t at hist + (t - 1) N C H W
int kxk_forward(const void* gate, int dtype, bool absnorm, const float* x, float* out, float* hist, int N, int C, int H, int W, int K, int n_iter,
                void* ws, hipStream_t st);
// ws: A_1 .. A_{n-1} ((n - 1) N C H W floats: kxk_absnorm_alev_bytes), then with absnorm and n_iter >= 2 the float32 plane [N][H][W] of 1 / S;
// gg (summed over C) and gx may each be NULL; hist as the forward kept it
inline size_t kxk_absnorm_alev_bytes(size_t L, int n_iter) { return round256(sizeof(float) * L * (size_t)(n_iter - 1)); }
int kxk_backward(const void* gate, int dtype, bool absnorm, const float* x, const float* hist, const float* gout, void* gg, float* gx, int N, int C,
                 int H, int W, int K, int n_iter, void* ws, hipStream_t st);

// ---- the depth-completion contract over a K x K neighbourhood, K = 3, 5 or 7 (cspn2d_kxk.hip): guidance [B][K*K-1][H][W] raw, blur
// [B][C][H][W], sparse NULL (sparse_C 0) or [B][sparse_C][H][W] with sparse_C 1 or C; normalised, neighbour-sited, pinned, folded into w' and b.
// guid and gg in the type of dtype as above; w' and b stay float32 in the workspace, so the workspace sizes do not depend on it ----
// the folded w' and b in front of each workspace (floats)
size_t kxk_norm_fold_floats(int B, int C, int sparse_C, int H, int W, int K);
// ws: the fold, then (hist NULL) the two ping-pong levels of kxk_forward; hist as kxk_forward
int kxk_norm_forward(const void* guid, int dtype, const float* blur, const float* sparse, float* out, float* hist, int B, int C, int sparse_C, int H,
                     int W, int K, int n_iter, int norm, void* ws, hipStream_t st);
// ws: the fold, dL/dw', dL/db (one fold's size), then A_1 .. A_{n-1}; gg needs hist (n >= 2), gx and gg may each be NULL
int kxk_norm_backward(const void* guid, int dtype, const float* blur, const float* sparse, const float* hist, const float* gout, void* gg, float* gx,
                      int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, hipStream_t st);
// the assembling contract on the same levels: out = sum_j conf_j H_{s_j}, conf [B][T][H][W] shared by the C channels, steps s_0 < .. < s_{T-1} = n_iter
// in host memory (s_0 >= 0), n_iter >= 1.  ws as kxk_norm_forward; hist NULL or H_1 .. H_n (n levels: H_n is not the output)
int kxk_assemble_forward(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out,
                         float* hist, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws, hipStream_t st);
// ws: kxk_norm_backward's, then one level (kxk_level_floats) for A_n = conf_{T-1} gout; gc = dL/dconf; gg, gx, gc may each be NULL; gg (n >= 2) and gc need hist
int kxk_assemble_backward(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, const float* hist,
                          const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm, void* ws,
                          hipStream_t st);
// the same four at dilation D (cspn2d_kxk_dil.hip): the neighbour offset of gate channel (t, l) is D (K/2 - t, K/2 - l); workspaces and
// histories as at D = 1.  kxk_dilation_ok: D is 1 or one of the dilated instances; the _dil functions take one of those, not 1
bool kxk_dilation_ok(int D);
int kxk_norm_forward_dil(const void* guid, int dtype, const float* blur, const float* sparse, float* out, float* hist, int B, int C, int sparse_C, int H,
                         int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_norm_backward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* hist, const float* gout, void* gg, float* gx,
                          int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_assemble_forward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T, float* out,
                             float* hist, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_assemble_backward_dil(const void* guid, int dtype, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                              const float* hist, const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int D,
                              int n_iter, int norm, void* ws, hipStream_t st);
// the same four pinned to the measured depth with a per-pixel confidence (cspn2d_kxk_pin.hip), at D = 1 or a dilated instance: after every
// step H = u step(H) + m sparse, m = sign(sparse) conf, u = 1 - m (folded: w' = u wb, b = (u c) blur + m sparse).  conf has the planes of
// sparse (sparse_C 1 or C, never 0); gs = dL/dsparse and gp = dL/dpin (the same planes) may each be NULL; gp needs hist as gg does
struct KxkPin {
    const float* conf = nullptr;
    float* gs = nullptr;
    float* gp = nullptr;
};
int kxk_norm_forward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, float* out, float* hist, int B, int C,
                         int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_norm_backward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* hist, const float* gout, void* gg,
                          float* gx, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_assemble_forward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* conf, const int* steps, int T,
                             float* out, float* hist, int B, int C, int sparse_C, int H, int W, int K, int D, int n_iter, int norm, void* ws, hipStream_t st);
int kxk_assemble_backward_pin(const void* guid, int dtype, const float* blur, const float* sparse, const KxkPin& pin, const float* conf, const int* steps, int T,
                              const float* hist, const float* gout, void* gg, float* gx, float* gc, int B, int C, int sparse_C, int H, int W, int K, int D,
                              int n_iter, int norm, void* ws, hipStream_t st);

// ---- K x K propagation with per-step attention, K = 3, 5 or 7 (cspn2d_kxk_dyn.hip): guid [N][K*K-1][H][W] raw and centre-sited, att
// [N][n (R+1)][H][W] used as given (channel s (R+1) + r: r = 0 the pixel's own term of step s, r >= 1 its ring r), values [N][C][H][W] on the
// shared guid / att, sparse NULL or [N][H][W] (pinned where > 0 before every step; the result is not pinned).  float32 throughout ----
// levels of kxk_level_floats(N C H W) floats in the forward's workspace: the pinned H_0 (with sparse), then the ping-pong pair unless the levels
// go to a history
inline int kxk_dyn_forward_levels(int n_iter, bool sparse, bool history) {
    return n_iter <= 0 ? 0 : (sparse ? 1 : 0) + (history ? 0 : (n_iter >= 3 ? 2 : n_iter - 1));
}
// the backward's workspace, in bytes from its start (every part 256-byte aligned): A_1 .. A_{n-1}, the 2 R ring-sum planes of the raw gates
// ([N][2 R][H][W]), and with sparse the pinned H_0
struct KxkDynBackwardWs {
    size_t rings, h0, bytes;
    KxkDynBackwardWs(int N, int C, int H, int W, int K, int n_iter, bool sparse) {
        const size_t HW = (size_t)H * W, L = (size_t)N * C * HW;
        rings = round256(sizeof(float) * L * (size_t)(n_iter - 1));
        h0 = rings + round256(sizeof(float) * (size_t)N * 2 * (K / 2) * HW);
        bytes = h0 + (sparse ? round256(sizeof(float) * L) : 0);
    }
};
// hist: NULL, or the pinned levels 1 .. n-1, level t at hist + (t - 1) N C H W
int kxk_dyn_forward(const float* guid, const float* att, const float* x, const float* sparse, float* out, float* hist, int N, int C, int H, int W, int K,
                    int n_iter, void* ws, hipStream_t st);
// gg (summed over C), ga and gx may each be NULL; gg / ga need hist where n_iter >= 2
int kxk_dyn_backward(const float* guid, const float* att, const float* x, const float* sparse, const float* hist, const float* gout, float* gg, float* ga,
                     float* gx, int N, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st);

// ---- line-scan propagation, SPN's three-way recurrence (cspn2d_scan.hip): x [B][C][H][W], gates [B][D Cg 3][H][W] used as
// given (channel (d Cg + j) 3 + k), lam NULL or [B][D C][H][W], out [B][D C][H][W]; dirs a 4-bit mask of {0 left->right, 1 right->left,
// 2 top->bottom, 3 bottom->top}, D its size.  float32 throughout ----
// the longest line (H for directions 0 / 1, W for 2 / 3): 8 pixels for each of a workgroup's 256 threads
constexpr int SCAN_MAX_LINE = 2048;
// the backward's workspace, in bytes from its start (every part 256-byte aligned): grad_x of the directions d = 1 .. D-1 ([D-1][B][C][H][W]),
// grad_gates of a group's channels r = 1 .. C/Cg - 1 ([C/Cg - 1][B][D Cg 3][H][W]); never empty
struct ScanBackwardWs {
    size_t xpart, gpart, bytes;
    ScanBackwardWs(int B, int C, int Cg, int H, int W, int D) {
        const size_t HW = (size_t)H * W;
        xpart = 256;
        gpart = xpart + round256(sizeof(float) * (size_t)(D - 1) * B * C * HW);
        bytes = gpart + round256(sizeof(float) * (size_t)(C / Cg - 1) * B * D * Cg * 3 * HW);
    }
};
int scan_forward(const float* x, const float* gates, const float* lam, float* out, int B, int C, int Cg, int H, int W, int dirs, hipStream_t st);
// gx (summed over the directions), gg (summed over a group's channels) and gl may each be NULL
int scan_backward(const float* x, const float* gates, const float* lam, const float* out, const float* gout, float* gx, float* gg, float* gl, int B, int C,
                  int Cg, int H, int W, int dirs, void* ws, hipStream_t st);

// ---- non-local propagation with learned offsets, K = 3 (cspn2d_nl.hip): aff [B][KK][H][W] used as given, off [B][2 KK][H][W] (dy_k, dx_k
// interleaved), values [B][C][H][W] on shared aff / off, sparse NULL or [B][H][W] (pinned where > 0).  Neighbour k's base is (t - R, l - R):
// the deformable convolution's sign, the opposite of the K x K engine's.  adt / odt: the storage types of aff (and gaff) and of off (and goff),
// 0 float32 or CSPN_DTYPE_F16 / CSPN_DTYPE_BF16, in one of the pairs (0, 0), (0, T), (T, T) (checked by the caller); 16-bit values are widened
// exactly where they are read, 16-bit gradients are the float32 sums rounded once at their store; values, levels and workspaces stay float32 ----
// levels of kxk_level_floats(B C H W) floats in the forward's workspace: the pinned H_0 (with sparse) and the ping-pong pair; with a history
// the levels go there and only the pinned H_0 is left (the n_iter = 1 count)
inline int nl_forward_levels(int n_iter, bool sparse) { return n_iter <= 0 ? 0 : (sparse ? (n_iter >= 2 ? 2 : 1) : (n_iter >= 3 ? 2 : n_iter - 1)); }
// the backward's: the adjoint levels 1 .. n-1 as the scatter leaves them, then (with sparse) the pinned H_0 of the gate gradient
inline int nl_backward_levels(int n_iter, bool sparse) { return n_iter <= 0 ? 0 : n_iter - 1 + (sparse ? 1 : 0); }
// hist: NULL, or the pinned levels 1 .. n-1, level t at hist + (t - 1) B C H W
int nl_forward(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, float* out, float* hist, int B, int C, int H, int W,
               int K, int n_iter, void* ws, hipStream_t st);
// gaff, goff and gx may each be NULL; gaff / goff need hist where n_iter >= 2.  NOT run-to-run bitwise: the adjoint scatters with float atomics
int nl_backward(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout, void* gaff,
                void* goff, float* gx, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st);
// the sampling operator out_k(p) = bil(f, p + base_k + d_k(p)), f [B][H][W] -> out [B][KK][H][W], and its backward (gf by the scatter, goff
// written once; either may be NULL)
int nl_sample(const void* off, int odt, const float* f, float* out, int B, int H, int W, int K, hipStream_t st);
int nl_sample_backward(const void* off, int odt, const float* f, const float* gout, float* gf, void* goff, int B, int H, int W, int K, hipStream_t st);
// the tail of nl_backward: gaff / goff (each may be NULL) from the levels A_1 .. A_{n-1} at the start of ws, (1 - m) already applied or not;
// with sparse, the pinned H_0 goes to the level behind them
int nl_gate_gradients(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout,
                      void* gaff, void* goff, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st);
// ---- the same two backwards, run-to-run bitwise (cspn2d_nl_det.hip): the adjoint gathers through an inverted index of the operator and sums
// in an order-independent way; no float atomics ----
constexpr unsigned NL_DET_LONG = 128;        // lists longer than this are summed by a whole wave
constexpr size_t NL_DET_SCAN_TILE = 2048;    // counts a workgroup of the scan's first pass
// the index over P = B H W destinations, in bytes from its start (every part 256-byte aligned): the worklist counter, the starts (P + 1
// uint32), the fill cursors (P uint32) -- these three zeroed by each call --, the plane c (P floats; the propagation's index only), the
// worklist (work_cap uint32: at most 32 P / 129 lists are longer than NL_DET_LONG), the scan's partial sums (one uint32 a tile), the
// entries (8 bytes each, at most 32 P)
struct NlDetIndex {
    size_t counter, start, cursor, zeroed, cplane, work, sums, entries, bytes, cap;
    unsigned work_cap, tiles;
    NlDetIndex(size_t P, bool has_c) {
        work_cap = (unsigned)(P / 4 + 1);
        tiles = (unsigned)((P + NL_DET_SCAN_TILE - 1) / NL_DET_SCAN_TILE);
        cap = 32 * P;
        counter = 0;
        start = 256;
        cursor = start + round256(4 * (P + 1));
        zeroed = cplane = cursor + round256(4 * P);
        work = cplane + (has_c ? round256(4 * P) : 0);
        sums = work + round256(4 * (size_t)work_cap);
        entries = sums + round256(4 * (size_t)tiles);
        bytes = entries + 8 * cap;
    }
};
// ws: nl_backward's levels, then the index (with the plane c)
int nl_backward_det(const void* aff, int adt, const void* off, int odt, const float* x, const float* sparse, const float* hist, const float* gout,
                    void* gaff, void* goff, float* gx, int B, int C, int H, int W, int K, int n_iter, void* ws, hipStream_t st);
// ws: the index (without the plane c)
int nl_sample_backward_det(const void* off, int odt, const float* f, const float* gout, float* gf, void* goff, int B, int H, int W, int K, void* ws,
                           hipStream_t st);

// ---- backward of the 3D op, Paddle contract only (cspn3d_backward.hip) ----
// C > 1: feat / gout / gf are [B][C][V] on shared gates; gg [B][26][V] is the sum over the channels
// gdt: the storage type of g and gg; 16-bit: where the fused sweeps can run, the workspace also holds the float32 copy of the gates the
// transposed sweep reads
size_t backward3d_workspace(int B, int D, int H, int W, int n_iter, int C = 1, int gdt = 0);
// that workspace's parts, in bytes from its start: the levels H_1 .. H_{n-1} (hist) and A_1 .. A_{n-1} (ahist), each level B C volumes laid
// out like feat ([B][C][V]), the spare volume A_0 goes to when the caller does not want grad_feat, what the persistent kernel wants (pers),
// and -- 16-bit gates on a shape the fused sweeps take, else 0 -- the float32 copy of the gates (wide)
struct Backward3dLayout {
    size_t hist, ahist, a0, pers, wide, bytes;
    Backward3dLayout(int B, int C, int D, int H, int W, int n_iter, int gdt);
};
int backward3d(const void* g, const float* feat, const float* gout, void* gg, float* gf, int B, int D, int H, int W, int n_iter,
               void* ws, hipStream_t st, bool stepwise_only = false /* test-hook library: one launch per step */, int C = 1, int gdt = 0);
// n gates (n % 4 == 0, g 8-byte and w 16-byte aligned) widened exactly into float32
int widen_gates(const void* g, int gdt, float* w, size_t n, hipStream_t st);

// ---- backward of the 3D op in its normalising / masked modes (cspn3d_norm_backward.hip): norm 8SUM / 8SUM_ABS, or NONE with a mask; g raw
// guidance [B][26][V], sparse NULL or [B][V]; gg and gf may each be NULL.  The adjoint sweep runs through the persistent kernel's transposed
// instance where backward3d_norm_fused() holds and stepwise_only is false, every other launch is per step.  gdt: the storage type of g and gg
// (0 float32, CSPN_DTYPE_F16, CSPN_DTYPE_BF16; read where used, gg rounded once at its store); the workspace is float32 for every type ----
size_t backward3d_norm_workspace(int B, int D, int H, int W, int n_iter);
bool backward3d_norm_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, const void* gg, const float* gf,
                           int B, int D, int H, int W, int n_iter, const void* ws);
int backward3d_norm(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, void* gg, float* gf, int B, int D, int H,
                    int W, int n_iter, int norm, void* ws, hipStream_t st, bool stepwise_only);

// ---- the same modes for C value channels on SHARED guidance (feat / out / gout / gf [B][C][V], sparse NULL or [B][V]): the fold runs once
// per call into w' [B][26][V] and coef [B][V], each channel's constant term is coef H_{0,c}; gg is the sum over the channels ----
// (cspn3d_norm_backward.hip) vec here and below: four voxels a thread (the caller's quads_ok), else one
int fold3d_shared(const void* g, int gdt, const float* sparse, float* wp, float* kp, int B, int D, int H, int W, int norm, bool vec, hipStream_t st);
// (cspn3d_stepwise.hip) one step of all channels: hout_c = kp h0_c + sum_k wp_k hin_c(p + off_k)
int step3d_shared(const float* wp, const float* kp, const float* h0, const float* hin, float* hout, int B, int C, int D, int H, int W, bool vec,
                  hipStream_t st);
size_t forward3d_norm_multi_workspace(int B, int C, int D, int H, int W, int n_iter);
bool forward3d_norm_multi_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* out, int B, int C, int D, int H, int W,
                                int n_iter, const void* ws);
int forward3d_norm_multi(const void* g, int gdt, const float* feat, const float* sparse, float* out, int B, int C, int D, int H, int W, int n_iter,
                         int norm, void* ws, hipStream_t st, int algo);
// (cspn3d_persistent.hip) all steps of all channels in one launch, wp and kp resident: the <HASC, MULTI> instance
int persistent3d_forward_shared(const float* wp, const float* kp, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                                void* ws, hipStream_t st);
size_t backward3d_norm_multi_workspace(int B, int C, int D, int H, int W, int n_iter);
bool backward3d_norm_multi_fused(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, const void* gg, const float* gf,
                                 int B, int C, int D, int H, int W, int n_iter, const void* ws);
int backward3d_norm_multi(const void* g, int gdt, const float* feat, const float* sparse, const float* gout, void* gg, float* gf, int B, int C,
                          int D, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, bool stepwise_only);

// ---- the producer of the path's inputs (cspn_head.hip): Unpool + 3x3 conv C -> 8 (guidance) and C -> 1 (blur) as one kernel; mode 0 raw guidance,
// 1 / 2 gate_wb of '8sum' / '8sum_abs' (the normalisation fused behind the conv) ----
size_t head_workspace(int C);
size_t head_backward_workspace(int B, int C, int h, int w);
int head_backward(const float* x, const float* w6, const float* w5, const float* gg, const float* gb, float* dx, float* dw6, float* dw5, int B, int C, int h,
                  int w, int H, int W, void* ws, hipStream_t st);
int head_forward(const float* x, const float* w6, const float* w5, float* gout, float* bout, int B, int C, int h, int w, int H, int W, int mode,
                 void* ws, hipStream_t st);

// ---- the heads for K x K propagation, K = 5 or 7 (cspn_head_kxk.hip): C -> K*K-1 (raw guidance) and C -> 1 (blur) on the matrix cores ----
size_t head_kxk_workspace(int C, int K);
int head_kxk_forward(const float* x, const float* wg, const float* wb, float* gout, float* bout, int B, int C, int h, int w, int H, int W, int K, void* ws,
                     hipStream_t st);
size_t head_kxk_backward_workspace(int B, int C, int h, int w, int K);
int head_kxk_backward(const float* x, const float* wg, const float* wb, const float* gg, const float* gb, float* dx, float* dwg, float* dwb, int B, int C,
                      int h, int w, int H, int W, int K, void* ws, hipStream_t st);
// the same on fp16 / bf16 x, guidance, dL/dguidance and dL/dx (cspn_head_kxk_g16.hip; dtype CSPN_DTYPE_F16 or CSPN_DTYPE_BF16, checked by the caller):
// float32 master weights rounded once per call, float32 blur, dL/dblur (rounded once as it enters the GEMMs) and weight gradients
size_t head_kxk_g16_workspace(int C, int K);
int head_kxk_g16_forward(const void* x, int dtype, const float* wg, const float* wb, void* gout, float* bout, int B, int C, int h, int w, int H, int W, int K,
                         void* ws, hipStream_t st);
size_t head_kxk_g16_backward_workspace(int B, int C, int h, int w, int K);
int head_kxk_g16_backward(const void* x, int dtype, const float* wg, const float* wb, const void* gg, const float* gb, void* dx, float* dwg, float* dwb, int B,
                          int C, int h, int w, int H, int W, int K, void* ws, hipStream_t st);
// the 8-plane head + the blur head on fp16 / bf16 x and dL/dx (cspn_head_g16.hip): guidance, blur and their gradients float32 (the gradients rounded once as
// they enter the GEMMs), float32 master weights rounded once per call, float32 weight gradients
size_t head_g16_workspace(int C);
int head_g16_forward(const void* x, int dtype, const float* wg, const float* wb, float* gout, float* bout, int B, int C, int h, int w, int H, int W, void* ws,
                     hipStream_t st);
size_t head_g16_backward_workspace(int B, int C, int h, int w);
int head_g16_backward(const void* x, int dtype, const float* wg, const float* wb, const float* gg, const float* gb, void* dx, float* dwg, float* dwb, int B, int C,
                      int h, int w, int H, int W, void* ws, hipStream_t st);

// ---- fused path (all iterations in one launch; time-skewed wave ring) ----
bool fused2d_supported(int B, int H, int W, int n_iter);
size_t fused2d_workspace(int B, int H, int W, int n_iter);
// plan_mode (test-hook library only; the ABI passes 0): 0 the linear plan, 1 the same without XCD-aware placement, 2 band groups;
// + 8: the 8-wave x 4-row loop of rounds 1-5 (cspn2d_tsw.hip) also for the passes the round-6 loop (cspn2d_tsw4.hip) would take;
// + 16: the round-6 loop for every full first pass it supports (also the short streams on which the dispatcher prefers the other)
// C > 1 (the assembly ring only): B image-channels [B][H][W] on B / C guidance images (cspn2d_forward_multi_f32)
int fused2d_forward(const float* g, const float* blur, const float* sparse, float* out, int B, int H, int W,
                    int n_iter, int norm, void* ws, hipStream_t st, bool use_asm = true, int plan_mode = 0, int C = 1);

// ---- the same ring with the main loop in gfx950 assembly (cspn2d_tsw.hip); one pass = 24 iterations, or -- a FIRST pass only
// (hin == blur, no history) -- n_early = 1 .. 23 of them ----
bool tsw2d_supported(int B, int H, int W);
// C > 1: B image-channels, C of them on each guidance image (cspn2d_tsw_plan.h PlanGeo::C)
int tsw2d_pass(const float* gd, const float* blur, const float* hin, const float* sparse, float* out, int B, int H,
               int W, int norm, hipStream_t st, float* hist = nullptr, int plan_mode = 0, int n_early = 0, int C = 1);
// ---- round 6: the same ring as 12 waves x 3 rows at 168 VGPRs -- three waves per SIMD (cspn2d_tsw4.hip, tools/tswgen/kernel4.py): FIRST
// passes of exactly 24 iterations ----
bool tsw4_supported(int B, int H, int W);
bool tsw4_preferred(int B, int H, int W, bool sparse);   // long streams on the linear plan: where it is the faster of the two rings
int tsw4_pass(const float* gd, const float* blur, const float* sparse, float* out, int B, int H, int W, int norm, hipStream_t st,
              int plan_mode = 0, int C = 1);
#ifdef CSPN_EXPERIMENTS
// ---- experiments kept out of the default build (make EXPERIMENTS=1): the round-3 loop (cspn2d_tsw3.hip: LDS-DMA row slots;
// ties with the loop above on long streams, slower on short ones: profiles/r03_perf_notes.md) and the sited8 guidance layout ----
bool tsw3_supported(int B, int H, int W, bool sparse, bool hin_differs);
int tsw3_pass(const float* gd, const float* blur, const float* hin, const float* sparse, float* out, int B, int H, int W,
              int norm, hipStream_t st);
#endif
int guidance_to_sited8(const float* g, float* out, int B, int H, int W, int norm, hipStream_t st);
int tsw2d_pass_sited8(const float* g8, const float* blur, const float* sparse, float* out, int B, int H, int W, int norm,
                      hipStream_t st);
int tsw2d_adjoint_pass(const float* wf, const float* a_in, float* a0, int B, int H, int W, hipStream_t st, float* hist);

// ---- multi-channel 2D entry points (cspn2d_multi.hip) ----
int widen_channels(const float* src, float* dst, int B, int C, size_t HW, hipStream_t st);   // [B][HW] -> [B][C][HW]
int add_inplace(float* dst, const float* src, size_t n, hipStream_t st);                      // dst += src

// ---- backward of the 2D op (cspn2d_backward.hip) ----
size_t backward2d_workspace(int B, int H, int W, int n_iter);
// that workspace's parts, in bytes from its start.  Where the ring's sweeps take the call (ckpt): the forward's checkpoints (hh), the folded
// coefficients (wf), the adjoint's checkpoints (ah), A_0 (a0) and a scratch output; `history` bytes of it are what a training forward keeps
// (forward2d_history), and `adjoint` bytes from `ah` what backward2d_history wants as its workspace.  Else one launch per step: the folded
// coefficients (wf), their transposes (wt), H_1 .. H_{N-1} (hh) and A_0 .. A_{N-1} (ah)
struct Backward2dLayout {
    bool ckpt;
    size_t hh, wf, wt, ah, a0, scratch, history, adjoint, bytes;
    Backward2dLayout(int B, int H, int W, int n_iter);
    static Backward2dLayout checkpointed(int B, int H, int W);

private:
    Backward2dLayout() = default;
};
// C > 1 (cspn2d_backward_multi_f32; the assembly sweeps only, backward2d_multi_supported): B counts image-channels [B][H][W], C of them share
// each of the B / C guidance images; gg [B / C][8][H][W] is the sum over the channels
int backward2d(const float* g, const float* blur, const float* sparse, const float* gout, float* gg, float* gb, int B, int H,
               int W, int n_iter, int norm, void* ws, hipStream_t st, int C = 1);
bool backward2d_multi_supported(int BC, int H, int W, int n_iter);
// training mode: the forward keeps its checkpoints (every fourth level + the folded coefficients; 24-iteration passes the assembly
// kernel takes), the backward starts there
size_t history2d_bytes(int B, int H, int W, int n_iter);  // 0: not available for this shape
int forward2d_history(const float* g, const float* blur, const float* sparse, float* out, void* history, int B, int H, int W,
                      int n_iter, int norm, void* ws, hipStream_t st, int C = 1);
size_t backward2d_history_workspace(int B, int H, int W);
int backward2d_history(const float* g, const float* blur, const float* sparse, const float* gout, const void* history, float* gg,
                       float* gb, int B, int H, int W, int n_iter, int norm, void* ws, hipStream_t st, int C = 1);

}  // namespace cspn
