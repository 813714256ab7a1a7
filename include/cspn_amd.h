/*
 * cspn_amd.h -- C ABI of the MI355X-native CSPN propagation engine (libcspn_amd.so).
 *
 * This is the drop-in boundary for the ONE hot path of XinJCheng/CSPN:
 * Affinity_Propagate (reference: cspn_pytorch/models/cspn.py:14-83) and the
 * 3x3x3 / pre-normalised-gate call site of the Paddle demo
 * (reference: cspn_paddle/demo.py:41-43,50-52).  Plain pointers and sizes only,
 * no torch types.  The binding a reference maintainer adds is ~25 lines of
 * ctypes; cspn_amd/cspn.py is that binding, packaged.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (fp32, contiguous NCHW / NCDHW) valid on
 *     the current HIP device; the call only ENQUEUES work on `stream` and returns
 *     (no hipDeviceSynchronize, no device allocation; safe to call from several
 *     host threads, cf. nn.DataParallel at reference cspn_pytorch/eval.py:117).
 *     State the library keeps between calls -- the complete list:
 *       (1) the persistent 3D kernel's, per device: the event that chains its
 *           launches, one pinned status word and two launch counters (see
 *           cspn3d_check_status);
 *       (2) memoisation with no effect on results: the CU count per device, and
 *           per host thread the last four 2D forward plans (cut positions of the
 *           linear plan, ~1 ms of host arithmetic per new shape).
 *     Nothing else: the library reads no environment variable and exports no test
 *     switch.  What tests and measuring tools need beyond this header (plan dumps,
 *     plan A/B, a persistent launch with a muted workgroup) is a SEPARATE library,
 *     libcspn_amd_hooks.so (csrc/cspn_test_hooks.hip), which links against this
 *     one and passes the test's choice as an argument of internal entry points;
 *   - inputs are never written; `out` must not alias an input;
 *   - return 0 on success, a negative CSPN_E_* code on argument errors, or a
 *     positive hipError_t; cspn_last_error() gives a thread-local message;
 *   - `workspace` must hold cspn{2,3}d_workspace_bytes(...) bytes, 256-B aligned,
 *     and must stay untouched until the enqueued work has finished.
 */
#ifndef CSPN_AMD_H
#define CSPN_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_ABI_VERSION 5   /* 2: cspn3d_check_status, CSPN_E_ASYNC, smaller cspn3d_workspace_bytes_ex; 3: cspn3d_forward_multi_f32;
                              * 4: CSPN_NORM_PRENORM, cspn2d_normalize_f32, cspn2d_forward_prenorm_f32, cspn3d_backward_multi_f32; the
                              *    sited8 experiment's three entry points left the ABI (hook library, experiment builds); CSPN_ALGO_FUSED_PADDED
                              *    (what AUTO returns for W % 4 != 0; cspn2d_workspace_bytes grows accordingly for such widths);
                              * 5: cspn_guidance_head_f32 (the producer of the path's inputs) and cspn_guidance_head_backward_f32; CSPN_NORM_PRENORM on the 2D backward entry points;
                              *    later, purely additive (no signature or behaviour changed, so the version stays): cspn2d_normalize_backward_f32,
                              *    the cspn2d_*_multi entry points (C channels on shared 2D guidance), the demo's gate normalisation
                              *    (cspn_gate_absnorm_f32 / _backward_f32, cspn3d_forward_absnorm_f32), the 2D K x K entry points
                              *    (cspn2d_*_kxk*, K = 5 / 7), K = 24 / 48 on the gate normaliser and the depth-completion contract over
                              *    K x K (cspn2d_*_kxk_norm*, K = 3 / 5 / 7), the guidance heads that feed it (cspn_guidance_head_kxk_*),
                              *    fp16 / bf16 gates and guidance on the K x K entry points (cspn2d_*_kxk*_g16, CSPN_DTYPE_*), the demo module's
                              *    gate normalisation inside the K x K engine (cspn2d_*_kxk_absnorm_*), the 8-plane heads on a 16-bit feature map with float32 guidance
                              *    (cspn_guidance_head_g16, cspn_guidance_head_backward_g16), fp16 / bf16 gates and guides on the 3D entry points of the
                              *    Paddle contract (cspn3d_*_g16, cspn_gate_absnorm*_g16), the backward of the 3D normalising / masked modes
                              *    (cspn3d_backward_norm_f32), dilated K x K propagation (cspn2d_*_kxk_{norm,assemble}_dil),
                              *    K x K propagation pinned to the measured depth with a confidence (cspn2d_*_kxk_{norm,assemble}_pin),
                              *    K x K propagation with per-step attention (cspn2d_*_kxk_dyn_*),
                              *    line-scan propagation, SPN's three-way recurrence (cspn2d_*_scan_*) */

/* hipStream_t, spelled without the HIP headers. NULL = the null stream. */
typedef void* cspn_stream_t;

/* norm_type: reference cspn_pytorch/models/cspn.py:19,36 ('8sum' | '8sum_abs');
 * NONE = gates are used as given, centre-sited, no centre term -- the contract of
 * fluid.layers.affinity_propagate (reference cspn_paddle/README.md:54: "should be
 * normalized in the channel dimension" by the caller, cspn_paddle/demo.py:47-49). */
enum { CSPN_NORM_8SUM = 0, CSPN_NORM_8SUM_ABS = 1, CSPN_NORM_NONE = 2,
       CSPN_NORM_PRENORM = 3 /* 2D only: `guidance` holds the reference's gate_wb (see cspn2d_normalize_f32 below) */ };

/* algo: AUTO picks the fused kernel whenever the shape allows it (W % 4 == 0, 16-byte aligned output).  FUSED runs images at
 * least 256 columns wide through the assembly main loop for EVERY n_iter (round 5): n_iter = 24 k + r is one short first pass
 * of r iterations (a row is stored when it completes level r) followed by k passes of 24 -- one launch per pass, 40 / 44 B
 * per pixel and pass; narrower images and FUSED_CXX (A/B tests) take the compiler-generated version of the same kernel. */
enum { CSPN_ALGO_AUTO = 0, CSPN_ALGO_STEPWISE = 1, CSPN_ALGO_FUSED = 2, CSPN_ALGO_FUSED_CXX = 3,
       CSPN_ALGO_FUSED_PADDED = 4 /* W % 4 != 0 (what AUTO picks there, round 5): the inputs are laid out once in the workspace with rows padded to a
                                    * multiple of 4 columns (zeros; 8SUM / 8SUM_ABS are normalised on the way, for the real width), the fused path
                                    * runs on those and the output is copied back: three more passes over the data instead of one launch per iteration */ };

/* gate_dtype of the *_g16 entry points: the storage type of the gate / guidance tensor and of its gradient */
enum { CSPN_DTYPE_F16 = 1 /* IEEE binary16 */, CSPN_DTYPE_BF16 = 2 /* bfloat16 */ };

enum {
    CSPN_E_BADARG = -1,   /* null pointer, non-positive size, unknown enum      */
    CSPN_E_WORKSPACE = -2, /* workspace too small or misaligned                  */
    CSPN_E_UNSUPPORTED = -3, /* algo explicitly requested but shape not supported */
    CSPN_E_ASYNC = -4      /* an EARLIER call failed on the device after it had returned (cspn3d_check_status) */
};

int cspn_abi_version(void);
const char* cspn_last_error(void);

/* ---- 2D: replaces Affinity_Propagate.forward, reference cspn.py:42-83 -------
 * (affinity_normalization :85-144, pad_blur_depth :147-172, sum_conv :44-53 and
 * the elementwise tail :70-81 are all inside this one call)
 *   guidance [B,8,H,W]  raw affinities as the backbone emits them (cspn.py:42)
 *   blur     [B,1,H,W]  coarse depth, also the H_0 of the centre term (cspn.py:58,76)
 *   sparse   [B,1,H,W]  or NULL; only its sign is used (cspn.py:64,81)
 *   out      [B,1,H,W]
 *   n_iter   = prop_time (cspn.py:31,66); 0 copies blur to out                  */
size_t cspn2d_workspace_bytes(int B, int H, int W, int n_iter);
int cspn2d_forward_f32(const float* guidance, const float* blur, const float* sparse, float* out,
                       int B, int H, int W, int n_iter, int norm_type,
                       void* workspace, size_t workspace_bytes, cspn_stream_t stream);
/* same, with an explicit kernel choice (tests and bench use it to A/B the paths) */
int cspn2d_forward_f32_algo(const float* guidance, const float* blur, const float* sparse, float* out,
                            int B, int H, int W, int n_iter, int norm_type, int algo,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);
/* which kernel AUTO would run for this shape: CSPN_ALGO_FUSED, CSPN_ALGO_FUSED_PADDED (W % 4 != 0: rows padded in the workspace) or
 * CSPN_ALGO_STEPWISE (also AUTO's fallback when `out` / the workspace is not 16-byte aligned) */
int cspn2d_auto_algo(int B, int H, int W, int n_iter);

/* ---- 2D with the normalisation moved to the producer (second alternative: "fuse normalisation into that conv's
 * epilogue", the conv being gud_up_proj_layer6 at cspn_pytorch/models/torch_resnet_cspn_nyu.py:187-206,318-319,372-373).
 * The contract is the reference's own intermediate: `gate_wb`, what affinity_normalization returns (cspn.py:85-144, used at
 * :69-76) -- wb [B,8,H,W] with wb_k(p) = G_k(p) / sum_j |G_j(p)|, G_k(p) = g~_k(p + off_k), zero outside the image: normalised AND
 * consumer-sited, the same 32 B/pixel as the raw guidance.  norm_type CSPN_NORM_PRENORM on cspn2d_forward_f32 / _algo takes such a
 * tensor in the `guidance` argument: what is left of the fold is sigma = sum_k wb_k, the centre term (1 - sigma) H_0 (cspn.py:76)
 * and the mask (cspn.py:81) -- no abs-sum, no reciprocal, no edge patching, aligned loads.  Results: those of CSPN_NORM_8SUM /
 * _8SUM_ABS on the raw guidance up to the rounding of the division (<= 1e-6 relative; NaN where sum |G| = 0, as the reference).
 * Every shape and n_iter the forward takes.  Backward (ABI 5): cspn2d_backward_f32 / _history_f32 with CSPN_NORM_PRENORM return dL/d(wb) in grad_guidance --
 * dL/dwb_k(p) = (1 - m)(dW'_k - dC H_0)(p), no normalisation chain, no scatter -- and dL/d(blur_depth); cspn2d_normalize_backward_f32 (below) chains dL/d(wb) into the raw guidance.
 * cspn2d_normalize_f32 is that producer epilogue as a stand-alone kernel (norm_type 8SUM or 8SUM_ABS; tests, A/B timing):
 * 36 B read + 32 B written per pixel.  cspn2d_forward_prenorm_f32 = cspn2d_forward_f32 with norm_type CSPN_NORM_PRENORM. */
int cspn2d_normalize_f32(const float* guidance, float* wb, int B, int H, int W, int norm_type, cspn_stream_t stream);
/* The adjoint of cspn2d_normalize_f32 (what torch autograd computes through affinity_normalization, cspn.py:85-144, for the cropped gate_wb):
 *   guidance      [B,8,H,W]  the raw guidance, as cspn2d_normalize_f32 takes it
 *   grad_wb       [B,8,H,W]  dL/d(gate_wb), consumer-sited: what cspn2d_backward_f32 / _history_f32 return in grad_guidance under CSPN_NORM_PRENORM
 *   grad_guidance [B,8,H,W]  dL/d(guidance) (must not alias either input)
 * With g~ = g (8SUM) or |g| (8SUM_ABS), G_k(p) = g~_k(p + off_k) (0 outside the image), S(p) = sum_j |G_j(p)|, T(p) = sum_j grad_wb_j(p) G_j(p):
 *   dL/dg_k(p + off_k) = ( grad_wb_k(p) / S(p) - sign(G_k(p)) T(p) / S(p)^2 )  [ * sign(g_k(p + off_k)) for 8SUM_ABS ],
 * the chain cspn2d_backward_f32 evaluates inside the raw route; elements no pixel reads get 0, S(p) = 0 gives NaN (IEEE, as torch).
 * norm_type 8SUM or 8SUM_ABS; every B, H, W >= 1; 4-byte-aligned pointers.  No workspace, no atomics: every output element is written
 * once, deterministic.  96 B/pixel (raw guidance + grad_wb read, grad_guidance written). */
int cspn2d_normalize_backward_f32(const float* guidance, const float* grad_wb, float* grad_guidance, int B, int H, int W, int norm_type,
                                  cspn_stream_t stream);
int cspn2d_forward_prenorm_f32(const float* wb, const float* blur, const float* sparse, float* out,
                               int B, int H, int W, int n_iter, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- 2D backward: the gradient torch autograd computes through Affinity_Propagate.forward (reference cspn.py:42-83),
 * i.e. what reference cspn_pytorch/train.py:196-198 back-propagates through.
 *   grad_out      [B,1,H,W]  dL/d(out)
 *   grad_guidance [B,8,H,W]  dL/d(guidance), or NULL to skip
 *   grad_blur     [B,1,H,W]  dL/d(blur_depth) (as level-0 value and as H_0 of the centre / mask terms), or NULL to skip
 * sparse_depth gets no gradient (only its sign is used, cspn.py:64).  n_iter >= 1.  norm_type: 8SUM, 8SUM_ABS, NONE, or PRENORM (then `guidance` = gate_wb and
 * grad_guidance = dL/d(gate_wb), see above).  Fast path (two sweeps of the assembly ring that keep every fourth
 * level + one recomputing final pass): W >= 256, W % 4 == 0, n_iter = 4, 8 .. 24 (24 only until round 5); everything else runs one launch per step.
 * For n_iter < 24 both sweeps still run the full 24-level ring and discard the levels beyond n_iter (the checkpoint of level n_iter is stored when the row passes it;
 * `out` briefly holds level 24 before the level-n_iter plane overwrites it): correct, but their cost does not shrink with n_iter (profiles/r05_backward_niter.jsonl),
 * and the discarded levels may hold Inf / NaN -- never read `scratch` or `out` of a call that has not completed. */
size_t cspn2d_backward_workspace_bytes(int B, int H, int W, int n_iter);
int cspn2d_backward_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                        float* grad_guidance, float* grad_blur, int B, int H, int W, int n_iter, int norm_type,
                        void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* Training mode (optional, faster): the forward also keeps what the backward needs -- every fourth intermediate level (H_4, H_8 ..
 * H_20; the backward recomputes the three in between) and the folded coefficients, 13 planes of B*H*W floats, cspn2d_history_bytes() bytes, 256-B aligned; 0 = not available for this shape / n_iter (available: W >= 256, W % 4 == 0, n_iter = 4, 8 .. 24; else use
 * cspn2d_forward_f32 + cspn2d_backward_f32, which recomputes the history).  This is what torch autograd does for the
 * reference by saving ~27 temporaries per iteration.
 *   cspn2d_forward_history_f32: same result as cspn2d_forward_f32, plus `history`; workspace cspn2d_workspace_bytes().
 *   cspn2d_backward_history_f32: same result as cspn2d_backward_f32 from that history; workspace
 *   cspn2d_backward_history_workspace_bytes(). */
size_t cspn2d_history_bytes(int B, int H, int W, int n_iter);
int cspn2d_forward_history_f32(const float* guidance, const float* blur, const float* sparse, float* out, void* history,
                               size_t history_bytes, int B, int H, int W, int n_iter, int norm_type,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_history_workspace_bytes(int B, int H, int W, int n_iter);
int cspn2d_backward_history_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                                const void* history, size_t history_bytes, float* grad_guidance, float* grad_blur,
                                int B, int H, int W, int n_iter, int norm_type,
                                void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- 3D: replaces n_iter chained fluid.layers.affinity_propagate calls,
 * reference cspn_paddle/demo.py:41-43,50-52 (kernel_size == 3 only, demo.py:90)
 *   gate [B,26,D,H,W], feat [B,1,D,H,W], sparse [B,1,D,H,W] or NULL, out [B,1,D,H,W] */
size_t cspn3d_workspace_bytes(int B, int D, int H, int W, int n_iter);   /* enough for every mode */
/* what this particular call needs with 16-byte aligned tensors (norm NONE without a mask: two value volumes + the exchange
 * buffers of the persistent kernel, ~14 MB; the folding modes, and misaligned tensors: 27 planes more = cspn3d_workspace_bytes) */
size_t cspn3d_workspace_bytes_ex(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse);
int cspn3d_forward_f32(const float* gate, const float* feat, const float* sparse, float* out,
                       int B, int D, int H, int W, int n_iter, int norm_type,
                       void* workspace, size_t workspace_bytes, cspn_stream_t stream);
/* algo: AUTO keeps the 26 gates of every voxel in registers across all n_iter steps (persistent kernel, one pass over the
 * gate tensor per forward) when W % 4 == 0, the tensors are 16-byte aligned and 2 <= n_iter <= 60 -- the Paddle contract
 * (norm NONE, no mask) directly, the normalising / masked modes after one folding pass; STEPWISE = one launch and one pass
 * over the gates (or the 27 folded planes) per step.  The persistent kernel needs all of its workgroups resident at once;
 * launches of one process are chained so that two of them never share the device: one process per GPU. */
enum { CSPN_ALGO3D_AUTO = 0, CSPN_ALGO3D_STEPWISE = 1, CSPN_ALGO3D_PERSISTENT = 2 };
/* Failures that only show on the device.  The workgroups of the persistent kernel wait for each other; if some of them never get
 * a compute unit (another process, a CU mask, a long kernel of another library on the device), the waiting ones give up after
 * ~0.5 s, fill the voxels they own with NaN -- the call's `out` then never passes for a result -- and raise a sticky per-device
 * status word.  The NEXT cspn3d_* call of the process on that device (forward or backward, any stream) finds it without a
 * synchronisation, returns CSPN_E_ASYNC instead of enqueuing anything (the reporting call itself is NOT run: call again), and
 * remembers that this launch has been reported: the status word holds the NUMBER of the launch that gave up, so the same
 * launch's other workgroups, which run into their own timeouts later, do not produce a second report.  (A launch captured into a
 * HIP graph replays with frozen arguments: it raises a fixed marker instead, which is cleared when reported, so EVERY failing
 * replay is reported -- possibly twice, if more of its workgroups time out after the report.)  cspn3d_check_status
 * synchronises `stream` first, so it also reports the call just made: 0, CSPN_E_ASYNC or a hipError_t.
 * Pre-flight: the persistent kernel is only chosen when hipOccupancyMaxActiveBlocksPerMultiprocessor x the CU count says all of
 * its workgroups fit the device at once; otherwise AUTO runs the per-step kernels (and PERSISTENT returns CSPN_E_UNSUPPORTED). */
int cspn3d_check_status(cspn_stream_t stream);
int cspn3d_forward_f32_algo(const float* gate, const float* feat, const float* sparse, float* out,
                            int B, int D, int H, int W, int n_iter, int norm_type, int algo,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* C input channels on SHARED gates (reference cspn_paddle/README.md:56: "gate_weight would be shared in the channel dimension for
 * input when C>1"; call site demo.py:41-43): feat, out [B,C,D,H,W], gate [B,26,D,H,W] used as given (norm NONE, no mask), n_iter
 * chained steps.  The gates of a chunk are read ONCE and stay in the registers while the steps run for channel after channel
 * (a per-channel loop over cspn3d_forward_f32 reads the 104 B/voxel of gates C times).  cspn3d_multi_supported() != 0 where the
 * persistent kernel takes the call (W % 4 == 0, 2 <= n_iter <= 60, 16-byte aligned tensors, the volume fits the device);
 * elsewhere the entry point returns CSPN_E_UNSUPPORTED and the caller loops over the channels.  Workspace:
 * cspn3d_workspace_bytes_ex(B, D, H, W, n_iter, CSPN_NORM_NONE, 0).  Same failure reporting as above (CSPN_E_ASYNC). */
int cspn3d_multi_supported(int B, int C, int D, int H, int W, int n_iter);
int cspn3d_forward_multi_f32(const float* gate, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                             void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* Backward of the 3D op under the Paddle contract (norm_type CSPN_NORM_NONE, no mask): the reference op is differentiated by
 * the demo's optimiser (cspn_paddle/demo.py:65-75, `feat` has stop_gradient=False).  grad_out [B,1,D,H,W];
 * grad_gate [B,26,D,H,W] and grad_feat [B,1,D,H,W] are outputs, either may be NULL.  n_iter chained steps with the same
 * gates are differentiated as one op (n_iter = 1 is the single fluid.layers.affinity_propagate call). */
size_t cspn3d_backward_workspace_bytes(int B, int D, int H, int W, int n_iter);
int cspn3d_backward_f32(const float* gate, const float* feat, const float* grad_out, float* grad_gate, float* grad_feat,
                        int B, int D, int H, int W, int n_iter, int norm_type,
                        void* workspace, size_t workspace_bytes, cspn_stream_t stream);
/* The same for C input channels on SHARED gates (reference cspn_paddle/README.md:56; the demo's optimiser differentiates the op,
 * demo.py:65-75): feat, grad_out, grad_feat [B,C,D,H,W]; grad_gate [B,26,D,H,W] = the gate gradient SUMMED over the channels (what
 * autograd accumulates into a shared tensor).  Any shape and n_iter >= 1; with n_iter >= 3 where cspn3d_multi_supported() holds, the
 * level-keeping forward and the transposed sweep are ONE persistent launch each for all channels (gates resident in the registers
 * across the channels) and the gate planes are written once.  Outputs may be NULL.  C = 1 is cspn3d_backward_f32. */
size_t cspn3d_backward_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter);
int cspn3d_backward_multi_f32(const float* gate, const float* feat, const float* grad_out, float* grad_gate, float* grad_feat,
                              int B, int C, int D, int H, int W, int n_iter,
                              void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* Backward of the 3D op in its normalising and masked modes -- what cspn3d_forward_f32 computes with CSPN_NORM_8SUM / CSPN_NORM_8SUM_ABS
 * (its default: the 3D form of Affinity_Propagate's contract) or with a mask: guidance [B,26,D,H,W] RAW, feat / grad_out [B,1,D,H,W], sparse
 * [B,1,D,H,W] or NULL (only its sign is used; it gets no gradient); grad_guidance [B,26,D,H,W] and grad_feat [B,1,D,H,W] are outputs, either may
 * be NULL (both: returns 0, launches nothing).  Per voxel p, off_k the offset of channel k, everything outside the volume zero:
 *   forward   G_k(p) = g~_k(p + off_k), g~ = |g| (8SUM_ABS) or g;  S = sum_j |G_j|, wb_k = G_k / S, sigma = sum_k wb_k
 *             (NONE: G_k(p) = g_k(p), S = 1, no centre term);  m = sign(sparse) (0 without), u = 1 - m
 *             w'_k = u wb_k,  c' = (u (1 - sigma) + m) H_0  (NONE: m H_0),  H_0 = feat,  H_{t+1}(p) = c'(p) + sum_k w'_k(p) H_t(p + off_k)
 *   backward  A_n = grad_out, A_t(q) = sum_k w'_k(q - off_k) A_{t+1}(q - off_k);  dW'_k(p) = sum_t A_{t+1}(p) H_t(p + off_k), dC = sum_t A_{t+1}
 *             grad_feat = A_0 + dC (u (1 - sigma) + m);  dwb_k = u (dW'_k - dC H_0)   (NONE: grad_guidance_k = u dW'_k)
 *             T = sum_j dwb_j G_j,  dG_k = dwb_k / S - sign(G_k) T / S^2,  grad_guidance_k(q) = dG_k(q - off_k) [x sign(g_k(q)) for 8SUM_ABS]
 *   sign(0) = 0 (torch's abs backward); S = 0 gives NaN as in the forward.  Every output element is written once, no atomics: two calls
 *   with the same algo are bitwise equal.  The fold is recomputed into the workspace; the forward levels run one launch per step, and only
 *   where grad_guidance is wanted.
 * norm_type CSPN_NORM_NONE with sparse NULL is cspn3d_backward_f32 (bitwise; algo STEPWISE: its per-step kernels); CSPN_NORM_PRENORM or an
 *   unknown value: CSPN_E_BADARG.  algo: CSPN_ALGO3D_STEPWISE runs one launch per adjoint step, for every shape and alignment;
 *   CSPN_ALGO3D_AUTO runs the n adjoint steps as ONE launch of the persistent kernel's transposed instance on w' where that instance takes
 *   the call (W % 4 == 0, every pointer 16-byte aligned, 3 <= n_iter <= 60, the volume fits the device: the fused sweep of
 *   cspn3d_backward_f32, failures reported the same way: CSPN_E_ASYNC, cspn3d_check_status) and per step elsewhere; CSPN_ALGO3D_PERSISTENT
 *   returns CSPN_E_UNSUPPORTED where AUTO would not use that instance.  Any B, D, H, W >= 1 and 4-byte aligned pointers; 16-byte loads and
 *   stores where W % 4 == 0 and every pointer is 16-byte aligned.  n_iter = 0: grad_feat = grad_out, grad_guidance = 0.  An output that overlaps an input,
 *   the other output or the workspace: CSPN_E_BADARG; a workspace smaller than cspn3d_backward_norm_workspace_bytes() or not 256-byte
 *   aligned: CSPN_E_WORKSPACE; the query returns 0 for an invalid shape or norm_type.  One channel; C channels on shared guidance:
 *   cspn3d_forward_norm_multi_f32 / cspn3d_backward_norm_multi_f32 below; float16 / bfloat16 guidance: cspn3d_backward_norm_g16 below. */
size_t cspn3d_backward_norm_workspace_bytes(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse);
int cspn3d_backward_norm_f32(const float* guidance, const float* feat, const float* sparse, const float* grad_out,
                             float* grad_guidance, float* grad_feat, int B, int D, int H, int W, int n_iter,
                             int norm_type, int algo, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the demo's module (reference cspn_paddle/demo.py:20-54, CSPN.cspn): guide = abs(guide) (:24), each slice of K = 3^d - 1 gate
 * channels divided by its own channel sum at the voxel (:34-36,47-49), then the chained propagation (:40-43,50-52) -- what a port of the
 * demo otherwise writes in torch in front of cspn3d_forward_f32 with CSPN_NORM_NONE.  Throughout w_k = |g_k| * r, r = 1 / S,
 * S = sum_{j=0..K-1} |g_j| added in channel order (one arithmetic form for the stand-alone and the fused kernel: bitwise equal);
 * an all-zero voxel gives 0 * inf = NaN, where torch's 0 / 0 gives NaN.
 * cspn_gate_absnorm_f32: guide [N,K,V] raw -> gate [N,K,V] = w (K = 8 or 26; 24 or 48 for the 2D K x K op below; V = voxels of a slice).  K * 4 B read + K * 4 B written per voxel.
 * cspn_gate_absnorm_backward_f32: the adjoint, guide [N,K,V] raw, grad_gate = dL/dw -> grad_guide = dL/dguide
 *   dL/dg_k = sign(g_k) (dL/dw_k - sum_j w_j dL/dw_j) * r, sign(0) = 0 (torch's abs backward): S and w are recomputed from guide, no
 *   workspace, no atomics (every output element written once); NaN in all K gradients of an all-zero voxel, as torch.
 * Both: any N, V >= 1 and 4-byte-aligned pointers (16-byte loads where V % 4 == 0 and every pointer is 16-byte aligned); K other than
 * 8 / 24 / 26 / 48, a null pointer or an output that overlaps an input: CSPN_E_BADARG.
 * cspn3d_forward_absnorm_f32: guide [B,26,D,H,W] RAW, feat / out [B,1,D,H,W]: the result of cspn_gate_absnorm_f32 followed by
 *   cspn3d_forward_f32(..., CSPN_NORM_NONE).  algo (CSPN_ALGO3D_*): AUTO normalises the resident gates inside the persistent kernel
 *   (no HBM bytes for it) wherever the NONE op would take the persistent kernel (W % 4 == 0, 2 <= n_iter <= 60, 16-byte aligned
 *   guide / feat / out / workspace, the volume fits the device), and elsewhere normalises into the workspace and runs the NONE op on it;
 *   STEPWISE always takes that second route (one launch per step); PERSISTENT returns CSPN_E_UNSUPPORTED where the kernel cannot take
 *   the call.  Workspace: cspn3d_forward_absnorm_workspace_bytes() covers both routes for 16-byte aligned feat / out (misaligned ones
 *   need cspn3d_workspace_bytes() more, as the folding path after the normaliser).  n_iter = 0 copies feat to out.  Failures of the
 *   persistent kernel are reported as for cspn3d_forward_f32: CSPN_E_ASYNC and cspn3d_check_status.  Gradients: the backward of the
 *   NONE op on w (cspn3d_backward_f32) chained through cspn_gate_absnorm_backward_f32. */
int cspn_gate_absnorm_f32(const float* guide, float* gate, int N, int K, size_t V, cspn_stream_t stream);
int cspn_gate_absnorm_backward_f32(const float* guide, const float* grad_gate, float* grad_guide, int N, int K, size_t V,
                                   cspn_stream_t stream);
size_t cspn3d_forward_absnorm_workspace_bytes(int B, int D, int H, int W, int n_iter);
int cspn3d_forward_absnorm_f32(const float* guide, const float* feat, float* out, int B, int D, int H, int W, int n_iter, int algo,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the 3D entry points of the Paddle contract on 16-bit gates (what a stereo head under autocast emits), gate_dtype CSPN_DTYPE_F16 or
 * CSPN_DTYPE_BF16 right after the gate pointer.  gate / guide and grad_gate / grad_guide are of that type; feat, out, grad_out, grad_feat,
 * every level and the workspace stay float32.  A gate is widened to float32 exactly where it is read (fp16 subnormals kept, bf16 = its
 * bits shifted left by 16) and every multiply-add, sum and division is the float32 kernel's in the same order: out and grad_feat are
 * BITWISE what the _f32 twin gives on the widened gates for the same shape, pointer alignments and path (persistent kernel or the same
 * per-step kernels; the same algo).  grad_gate / grad_guide is the float32 value rounded once, to nearest even, at its single store
 * (no atomics, every element written once): bitwise the _f32 twin's result converted to the type.
 * Dispatch: the _f32 twin's with the gate pointer's 16-byte condition at 8 bytes (four gates); W % 4 == 0 stays the condition of the
 * vector and persistent paths.  The persistent kernel reads a thread's quads with 8-byte loads and widens them into the gate registers
 * it already has (forward, level-keeping forward, multi-channel and raw-guide instances).  Its transposed instance has no 16-bit form:
 * the fused backward sweeps (n_iter >= 3 where the persistent kernel takes the call) widen the gates once into the workspace with an
 * exact streaming pass and run the float32 instance on that copy, which the *_g16_workspace_bytes queries account for.
 * All checks and return codes of the _f32 twins apply, gate ranges counted in 2-byte elements; any other gate_dtype or an odd address
 * of a 16-bit tensor: CSPN_E_BADARG.
 * cspn3d_forward_g16_algo: cspn3d_forward_f32_algo with norm_type CSPN_NORM_NONE and sparse NULL -- anything else CSPN_E_BADARG (the
 *   normalising and masked modes on 16-bit guidance have their own entry point, cspn3d_forward_norm_g16 below).  Workspace: cspn3d_workspace_bytes_ex / cspn3d_workspace_bytes as the twin.
 * cspn3d_forward_multi_g16, cspn3d_backward_g16, cspn3d_backward_multi_g16: as their twins; workspaces of the backward:
 *   cspn3d_backward_g16_workspace_bytes / cspn3d_backward_multi_g16_workspace_bytes (the same for both 16-bit types).
 * cspn3d_forward_absnorm_g16: guide RAW in 16 bits; the unfused route normalises into float32 gates in the workspace
 *   (cspn3d_forward_absnorm_workspace_bytes as the twin).
 * cspn_gate_absnorm_g16 / cspn_gate_absnorm_backward_g16: the normaliser of the 3D module (K = 26 only, else CSPN_E_BADARG) on a 16-bit
 *   guide: gate and grad_gate float32, grad_guide in the guide's type. */
int cspn3d_forward_g16_algo(const void* gate, int gate_dtype, const float* feat, const float* sparse, float* out,
                            int B, int D, int H, int W, int n_iter, int norm_type, int algo,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn3d_forward_multi_g16(const void* gate, int gate_dtype, const float* feat, float* out, int B, int C, int D, int H, int W, int n_iter,
                             void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn3d_forward_absnorm_g16(const void* guide, int gate_dtype, const float* feat, float* out, int B, int D, int H, int W, int n_iter, int algo,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn3d_backward_g16_workspace_bytes(int B, int D, int H, int W, int n_iter);
int cspn3d_backward_g16(const void* gate, int gate_dtype, const float* feat, const float* grad_out, void* grad_gate, float* grad_feat,
                        int B, int D, int H, int W, int n_iter, int norm_type,
                        void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn3d_backward_multi_g16_workspace_bytes(int B, int C, int D, int H, int W, int n_iter);
int cspn3d_backward_multi_g16(const void* gate, int gate_dtype, const float* feat, const float* grad_out, void* grad_gate, float* grad_feat,
                              int B, int C, int D, int H, int W, int n_iter,
                              void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn_gate_absnorm_g16(const void* guide, int gate_dtype, float* gate, int N, int K, size_t V, cspn_stream_t stream);
int cspn_gate_absnorm_backward_g16(const void* guide, int gate_dtype, const float* grad_gate, void* grad_guide, int N, int K, size_t V,
                                   cspn_stream_t stream);

/* ---- the 3D depth-completion contract (normalising and masked modes) on 16-bit guidance: the same exact-widening contract as above.
 * guidance and grad_guidance are of gate_dtype; feat, sparse, out, grad_out, grad_feat, w', c', coef, dG, every level and the workspace
 * stay float32.  No float32 copy of the guidance or of its gradient is made.
 * cspn3d_forward_norm_g16: cspn3d_forward_f32_algo in EVERY mode (CSPN_NORM_8SUM, CSPN_NORM_8SUM_ABS, CSPN_NORM_NONE with or without a
 *   mask) on 16-bit guidance; out is bitwise the twin's on the widened guidance.  The fold reads each gate where it uses it; the steps are
 *   the twin's (persistent kernel on the folded planes, or per step).  CSPN_NORM_NONE with sparse NULL is cspn3d_forward_g16_algo.
 *   Workspace: cspn3d_workspace_bytes_ex / cspn3d_workspace_bytes as the twin (guidance aligned to 8 bytes where the twin wants 16).
 * cspn3d_backward_norm_g16: cspn3d_backward_norm_f32's checks in its order, the guidance's and grad_guidance's ranges counted in 2-byte
 *   elements.  grad_feat is bitwise the twin's on the widened guidance; grad_guidance is the twin's float32 value rounded once, to nearest
 *   even, at its single store (NaN where the twin has NaN, zero where no voxel reads the gate), no atomics.  The fold, the gate-gradient
 *   epilogue and the gather read the 16-bit guidance directly (8-byte loads of four gates, at 2-byte alignment for the neighbour-sited
 *   reads); the vector kernels need W % 4 == 0, guidance and grad_guidance 8-byte aligned and every float32 tensor 16-byte aligned, the
 *   same condition decides CSPN_ALGO3D_PERSISTENT.  The adjoint sweep runs on the float32 w' as in the twin.
 *   CSPN_NORM_NONE with sparse NULL is cspn3d_backward_g16 (bitwise; algo STEPWISE: its per-step kernels).
 * cspn3d_backward_norm_g16_workspace_bytes: in the normalising and masked modes exactly cspn3d_backward_norm_workspace_bytes (everything
 *   in the workspace is float32); for CSPN_NORM_NONE with has_sparse 0 it is cspn3d_backward_g16_workspace_bytes, which keeps the
 *   widened copy the transposed sweep of the Paddle contract reads.  The same for both 16-bit types. */
int cspn3d_forward_norm_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, float* out,
                            int B, int D, int H, int W, int n_iter, int norm_type, int algo,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn3d_backward_norm_g16_workspace_bytes(int B, int D, int H, int W, int n_iter, int norm_type, int has_sparse);
int cspn3d_backward_norm_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, const float* grad_out,
                             void* grad_guidance, float* grad_feat, int B, int D, int H, int W, int n_iter,
                             int norm_type, int algo, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the 3D depth-completion contract for C value channels on SHARED guidance: feat / out / grad_out / grad_feat [B,C,D,H,W], guidance
 * [B,26,D,H,W] raw (float32, or of gate_dtype in the _g16 forms), sparse NULL or [B,1,D,H,W] shared by the channels -- the 3D form of the
 * broadcast of reference cspn_pytorch/models/cspn.py:58-81 and of "gate_weight would be shared in the channel dimension for input when C>1"
 * (cspn_paddle/README.md:56).  With the shared quantities of cspn3d_backward_norm_f32 above (w'_k, coef = u (1 - sigma) + m; NONE: m):
 *   forward   H_{0,c} = feat_c,  H_{t+1,c}(p) = coef(p) H_{0,c}(p) + sum_k w'_k(p) H_{t,c}(p + off_k),  out_c = H_{n,c}
 *   backward  A_{n,c} = grad_out_c,  A_{t,c}(q) = sum_k w'_k(q - off_k) A_{t+1,c}(q - off_k),  dC_c = sum_t A_{t+1,c}
 *             grad_feat_c = A_{0,c} + dC_c coef;  dW'_k = sum_c sum_t A_{t+1,c}(p) H_{t,c}(p + off_k) (c outer, t inner: a fixed order)
 *             dwb_k = u (dW'_k - sum_c dC_c H_{0,c}), then the fold's adjoint and the gather of cspn3d_backward_norm_f32
 *   grad_guidance is the sum over the channels, every element written once, no atomics: two calls with the same algo are bitwise equal.
 *   The constant term is formed as coef H_0, so for C > 1 a channel of out is close to, not bitwise, the single-channel call's (which forms
 *   (1 - m) ((1 - sigma) H_0) + m H_0).  The fold runs ONCE per call (w' and coef into the workspace); a step of all C channels reads them
 *   once (108 + 12 C bytes a voxel where C single-channel steps move 116 C), and where the persistent kernel takes the call (W % 4 == 0,
 *   every pointer 16-byte aligned, guidance of a 16-bit type 8-byte, 2 <= n_iter <= 60, cspn3d_multi_supported) they stay resident in
 *   registers / LDS across the steps and the channels.  The backward's adjoint sweep of all channels is one launch of the transposed
 *   multi-channel instance where 3 <= n_iter <= 60 and the same conditions hold for n_iter - 1 and n_iter, per step and channel elsewhere.
 * C = 1 IS the single-channel entry point (cspn3d_forward_f32_algo / cspn3d_forward_norm_g16 / cspn3d_backward_norm_f32 / _g16), bitwise.
 * CSPN_NORM_NONE with sparse NULL is the Paddle contract: the backward is cspn3d_backward_multi_f32 / _g16 (bitwise); the forward is
 *   cspn3d_forward_multi_f32 / _g16 (bitwise) where that runs (algo AUTO or PERSISTENT, aligned, cspn3d_multi_supported) and the per-step
 *   kernels with coef = 0 elsewhere.
 * Checks and return codes as cspn3d_backward_norm_f32: CSPN_NORM_PRENORM or an unknown norm_type: CSPN_E_BADARG; an output that overlaps
 *   an input, the other output or the workspace: CSPN_E_BADARG; workspace too small or not 256-byte aligned: CSPN_E_WORKSPACE; n_iter = 0:
 *   out = feat, grad_feat = grad_out, grad_guidance = 0; either output of the backward may be NULL; CSPN_ALGO3D_PERSISTENT returns
 *   CSPN_E_UNSUPPORTED where AUTO would not fuse; failures of a persistent launch: CSPN_E_ASYNC and cspn3d_check_status.
 * The _g16 forms follow the contract above: out and grad_feat bitwise the _f32 twin's on the widened guidance on the same path,
 *   grad_guidance that twin's float32 value rounded once at its single store.
 * The workspace queries return 0 for an invalid shape or norm_type; one backward query serves both guidance types.  At C = 1 they are
 *   cspn3d_workspace_bytes_ex and cspn3d_backward_norm_g16_workspace_bytes (= cspn3d_backward_norm_workspace_bytes in every mode but NONE
 *   without a mask). */
size_t cspn3d_forward_norm_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter, int norm_type, int has_sparse);
int cspn3d_forward_norm_multi_f32(const float* guidance, const float* feat, const float* sparse, float* out,
                                  int B, int C, int D, int H, int W, int n_iter, int norm_type, int algo,
                                  void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn3d_forward_norm_multi_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, float* out,
                                  int B, int C, int D, int H, int W, int n_iter, int norm_type, int algo,
                                  void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn3d_backward_norm_multi_workspace_bytes(int B, int C, int D, int H, int W, int n_iter, int norm_type, int has_sparse);
int cspn3d_backward_norm_multi_f32(const float* guidance, const float* feat, const float* sparse, const float* grad_out,
                                   float* grad_guidance, float* grad_feat, int B, int C, int D, int H, int W, int n_iter,
                                   int norm_type, int algo, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn3d_backward_norm_multi_g16(const void* guidance, int gate_dtype, const float* feat, const float* sparse, const float* grad_out,
                                   void* grad_guidance, float* grad_feat, int B, int C, int D, int H, int W, int n_iter,
                                   int norm_type, int algo, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- 2D over a K x K neighbourhood, K = 2R+1 in {5, 7}: fluid.layers.affinity_propagate(input, gate_weight, kernel_size) with
 * kernel_size 5 or 7, the NONE contract (gates used as given, centre-sited, no centre term, any sign; reference cspn_paddle/README.md:54-56).
 *   gate [B,KK,H,W], KK = K*K - 1; x / out [B,C,H,W], the C channels share the gates.
 *   Channel order: gate channel k is the k-th pair (t, l) in raster order over {0..K-1}^2 skipping the centre (R, R); its neighbour
 *   offset is (dy, dx) = (R - t, R - l) (with K = 3 this is the order of the 3 x 3 op).
 *   H_0 = x, H_{t+1}(p) = sum_{k=0..KK-1} g_k(p) H_t(p + off_k) (zero outside the image, summed in channel order), out = H_n.
 * cspn2d_forward_kxk_f32: history NULL -> the levels ping-pong in the workspace (cspn2d_kxk_workspace_bytes); history non-NULL ->
 *   H_1 .. H_{n-1} are kept there ([n-1][B][C][H][W], cspn2d_kxk_history_bytes; no workspace needed) for cspn2d_backward_kxk_f32.
 *   n_iter = 0 copies x to out.  One launch per step; per step and pixel 4 KK + 8 C bytes.
 * cspn2d_backward_kxk_f32: grad_out = dL/dout -> grad_x = dL/dx = A_0 and grad_gate = dL/dgate, summed over the C channels; either may
 *   be NULL.  A_n = grad_out, A_t(q) = sum_k g_k(q - off_k) A_{t+1}(q - off_k); dL/dg_k(p) = sum_{t<n} sum_c A_{t+1}(p) H_t(p + off_k),
 *   accumulated in registers over t, then c, every element written once (no atomics: deterministic).  The workspace
 *   (cspn2d_backward_kxk_workspace_bytes) keeps A_1 .. A_{n-1}; grad_gate needs the history of a forward with the same arguments.
 * All four: any 4-byte aligned pointers (16-byte loads and stores where W % 4 == 0 and the pointer is 16-byte aligned), any
 * H, W >= 1.  K other than 5 / 7, a null input, a size <= 0, an output, history or workspace overlapping an input or another output:
 * CSPN_E_BADARG; B C H W or B KK H W above 2^31 - 1 elements: CSPN_E_UNSUPPORTED; a workspace or history too small, or a workspace
 * not 256-byte aligned: CSPN_E_WORKSPACE.  The byte-count queries return 0 where the call needs nothing or the shape is invalid. */
size_t cspn2d_kxk_workspace_bytes(int B, int C, int H, int W, int K, int n_iter);
size_t cspn2d_kxk_history_bytes(int B, int C, int H, int W, int K, int n_iter);
int cspn2d_forward_kxk_f32(const float* gate, const float* x, float* out, float* history, size_t history_bytes,
                           int B, int C, int H, int W, int K, int n_iter,
                           void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_kxk_workspace_bytes(int B, int C, int H, int W, int K, int n_iter);
int cspn2d_backward_kxk_f32(const float* gate, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                            float* grad_gate, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the depth-completion contract of Affinity_Propagate (reference cspn_pytorch/models/cspn.py:42-144) over a K x K neighbourhood,
 * K = 2R+1 in {3, 5, 7}: the guidance normalised, each gate sited at its neighbour, a (1 - gate_sum) blur term, sparse depth pinned.
 *   guidance [B,KK,H,W] raw, KK = K*K - 1, in the channel order of the NONE op above: channel k is the k-th pair (t, l) in raster order
 *   over {0..K-1}^2 skipping the centre, offset off_k = (R - t, R - l); the reference's padding generalised is ZeroPad2d((l, K-1-l, t, K-1-t))
 *   followed by a crop of R on each side (K = 3: gate1 .. gate8 of cspn.py:104-131).  blur / out [B,C,H,W], the C channels share the
 *   guidance (the reference's broadcast); sparse NULL with sparse_C = 0, or [B,sparse_C,H,W] with sparse_C 1 (one mask for all channels) or C.
 *   norm CSPN_NORM_8SUM or CSPN_NORM_8SUM_ABS (g = |guidance|).  Per pixel p, zero outside the image:
 *     G_k(p) = g_k(p + off_k), wb_k = G_k / sum_j |G_j| (channel order; 0 / 0 = NaN as in the reference), c = 1 - sum_k wb_k,
 *     m = sign(sparse), u = 1 - m, H_0 = blur, H_{t+1} = u (sum_k wb_k H_t(p + off_k) + c blur) + m blur, out = H_n.
 *   The engine folds this into w'_k = u wb_k and b = (u c + m) blur (one launch) and runs the K x K step with b as its start value;
 *   with sparse_C = C > 1 the channels become images of their own w'.
 * cspn2d_forward_kxk_norm_f32: history NULL -> the workspace holds the fold and two ping-pong levels (cspn2d_kxk_norm_workspace_bytes);
 *   history non-NULL -> H_1 .. H_{n-1} are kept there ([n-1][B][C][H][W], cspn2d_kxk_norm_history_bytes) and the workspace needs only the
 *   fold (what cspn2d_kxk_norm_workspace_bytes returns for n_iter = 1).  n_iter = 0 copies blur to out.  Per step and pixel 4 KK + 12 C bytes.
 * cspn2d_backward_kxk_norm_f32: grad_out = dL/dout -> grad_guidance = dL/dguidance (summed over the C channels) and grad_blur = dL/dblur;
 *   either may be NULL; sparse gets no gradient (only its sign is used, cspn.py:64).  It recomputes the fold, runs the adjoint steps on w',
 *   one gate-gradient pass that also sums dL/db, then the fold's adjoint per pixel and a gather back to the raw guidance: every element
 *   written once (no atomics: deterministic).  grad_guidance with n_iter >= 2 needs the history of a forward with the same arguments.
 * Argument errors as the NONE op's block above, plus: K other than 3 / 5 / 7, norm other than 8SUM / 8SUM_ABS, sparse_C other than
 * 0 / 1 / C or not matching a NULL / non-NULL sparse: CSPN_E_BADARG.  cspn2d_forward_kxk_f32 still takes K = 5 / 7 only. */
size_t cspn2d_kxk_norm_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter);
size_t cspn2d_kxk_norm_history_bytes(int B, int C, int H, int W, int K, int n_iter);
int cspn2d_forward_kxk_norm_f32(const float* guidance, const float* blur, const float* sparse, float* out, float* history, size_t history_bytes,
                                int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm,
                                void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_kxk_norm_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter);
int cspn2d_backward_kxk_norm_f32(const float* guidance, const float* blur, const float* sparse, const float* history, size_t history_bytes,
                                 const float* grad_out, float* grad_guidance, float* grad_blur, int B, int C, int sparse_C, int H, int W, int K,
                                 int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the four K x K entry points above on 16-bit gates / guidance (what a head under autocast emits), gate_dtype CSPN_DTYPE_F16 or
 * CSPN_DTYPE_BF16.  gate / guidance and grad_gate / grad_guidance are of that type; x, blur, sparse, out, history, grad_out, grad_x /
 * grad_blur and the workspace (w' and b of the folded contract included) stay float32, and the byte-count queries above apply unchanged.
 *   Exact widening: a 16-bit gate is widened to float32 where it is used and every multiply-add and sum is the float32 one of the _f32
 *   entry point in the same order, so out and grad_x / grad_blur are bitwise what the _f32 entry point returns for the widened tensor.
 *   grad_gate / grad_guidance is accumulated in float32 exactly as there and rounded once, to nearest even with subnormals kept, at its
 *   single store: bitwise the _f32 gradient converted to gate_dtype.  No atomics; every element written once.
 *   Per step and pixel the NONE op reads 2 KK + 8 C bytes.  The 16-bit tensors need 2-byte alignment (8-byte loads and stores where
 *   W % 4 == 0 and the pointer is 8-byte aligned).  Argument errors as the _f32 twins, plus: any other gate_dtype: CSPN_E_BADARG ("dtype"
 *   in cspn_last_error()); a 16-bit tensor at an odd address: CSPN_E_BADARG. */
int cspn2d_forward_kxk_g16(const void* gate, int gate_dtype, const float* x, float* out, float* history, size_t history_bytes,
                           int B, int C, int H, int W, int K, int n_iter,
                           void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_g16(const void* gate, int gate_dtype, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                            void* grad_gate, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_forward_kxk_norm_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, float* out, float* history,
                                size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm,
                                void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_norm_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* history,
                                 size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur, int B, int C, int sparse_C,
                                 int H, int W, int K, int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- assembling K x K propagation levels per pixel (CSPN++, "context-aware" CSPN): the depth-completion contract above, but the result is
 * a per-pixel weighted sum of collected levels,
 *     out(b,c,p) = sum_{j<T} conf(b,j,p) H_{s_j}(b,c,p),     H_0 = blur, H_t the levels of cspn2d_forward_kxk_norm_*
 *   conf [B,T,H,W] float32, shared by the C channels; steps = {s_0 < s_1 < .. < s_{T-1} = n_iter}, s_0 >= 0, T ints in HOST memory, read
 *   before the call returns; 1 <= T <= n_iter + 1; n_iter >= 1.  The other arguments are those of the _kxk_norm_ entry points.  The engine
 *   runs the same fold and the same step; a step that produces a collected level also updates out from the level it holds in registers
 *   (4 + 8 C bytes per pixel more than a plain step's 4 KK + 12 C; the first collected step 4 + 4 C, out is written before it is read, so
 *   it need not be initialised); a collected level 0 rides on the first step.  The levels ping-pong in two workspace planes and out is
 *   a third buffer (cspn2d_kxk_assemble_workspace_bytes; with a history: that query's value for n_iter = 1, the fold).
 *   history: NULL, or n levels H_1 .. H_n ([n][B][C][H][W], cspn2d_kxk_assemble_history_bytes: H_n is not the output here).
 * Backward: grad_out = dL/dout -> grad_guidance, grad_blur (as the _kxk_norm_ backward) and grad_conf [B,T,H,W]; each may be NULL.
 *     A_n = conf_{T-1} grad_out (one plane at the end of the workspace), A_t = step^T(A_{t+1}) + [t = s_j] conf_j grad_out, added in the
 *     adjoint step's store; grad_blur also receives conf_0 grad_out where s_0 = 0; grad_conf(b,j,p) = sum_c grad_out(b,c,p) H_{s_j}(b,c,p),
 *     summed in channel order, every element written once (no atomics: deterministic).  grad_guidance (n_iter >= 2) and grad_conf need the
 *     history of a forward with the same arguments.  With T = 1 and conf = 1 every result is bitwise the _kxk_norm_ entry point's.
 * The _g16 twins take the guidance (and return grad_guidance) in gate_dtype under the rule of the 16-bit block above; conf stays float32.
 * Errors: a NULL pointer (named in cspn_last_error()), K, norm, sparse_C, n_iter < 1, T or steps out of the rules above, a view of 2^31
 * elements or more, an output aliasing an input or another output: CSPN_E_BADARG; a workspace or history too small or a workspace not
 * 256-byte aligned: CSPN_E_WORKSPACE.  The byte-count queries return 0 for arguments the entries refuse. */
size_t cspn2d_kxk_assemble_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter);
size_t cspn2d_kxk_assemble_history_bytes(int B, int C, int H, int W, int K, int n_iter);
size_t cspn2d_backward_kxk_assemble_workspace_bytes(int B, int C, int sparse_C, int H, int W, int K, int n_iter);
int cspn2d_forward_kxk_assemble_f32(const float* guidance, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                    float* out, float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K,
                                    int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_forward_kxk_assemble_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf,
                                    const int* steps, int T, float* out, float* history, size_t history_bytes, int B, int C, int sparse_C,
                                    int H, int W, int K, int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_assemble_f32(const float* guidance, const float* blur, const float* sparse, const float* conf, const int* steps, int T,
                                     const float* history, size_t history_bytes, const float* grad_out, float* grad_guidance, float* grad_blur,
                                     float* grad_conf, int B, int C, int sparse_C, int H, int W, int K, int n_iter, int norm,
                                     void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_assemble_g16(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf,
                                     const int* steps, int T, const float* history, size_t history_bytes, const float* grad_out,
                                     void* grad_guidance, float* grad_blur, float* grad_conf, int B, int C, int sparse_C, int H, int W, int K,
                                     int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- dilated K x K propagation (dilated CSPN++, as PENet's refinement runs each of its 3 x 3 / 5 x 5 / 7 x 7 propagations: once with
 * the neighbours two pixels apart, then once more at distance one): the _kxk_norm_ and _kxk_assemble_ contracts above with the neighbour
 * offset of gate channel k = (t, l) scaled by dilation D,
 *     off_k = D * (K/2 - t, K/2 - l),     D = 1 or 2,
 *   and nothing else changed: G_k(p) = g_k(p + off_k) (zero outside the image), wb_k = G_k / sum_j |G_j|, the (1 - sum_k wb_k) blur term,
 *   the mask, the steps, the assembled sum.  A pixel whose neighbours all lie outside the image (possible at D = 2: the middle row of a
 *   3 x 1 image) is 0 / 0 = NaN, as with the reference's torch.div.
 * Each entry mirrors its _g16 counterpart with `dilation` behind K; gate_dtype is 0 for float32 guidance (grad_guidance float32) or
 *   CSPN_DTYPE_F16 / CSPN_DTYPE_BF16 under the rule of the 16-bit block above.  The workspace and history sizes do not depend on the
 *   dilation: cspn2d_kxk_norm_workspace_bytes, cspn2d_kxk_norm_history_bytes, cspn2d_backward_kxk_norm_workspace_bytes and the three
 *   cspn2d_*kxk_assemble_*_bytes queries apply unchanged.  dilation 1 runs the very kernels of the _f32 / _g16 entry points (bitwise their
 *   results).  Deterministic: sums in channel order, every element written once.
 * Errors: those of the counterpart, and a dilation other than 1 or 2: CSPN_E_BADARG ("dilation" in cspn_last_error()), checked first,
 *   before anything touches the GPU. */
int cspn2d_forward_kxk_norm_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, float* out, float* history,
                                size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm,
                                void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_norm_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* history,
                                 size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur, int B, int C, int sparse_C,
                                 int H, int W, int K, int dilation, int n_iter, int norm, void* workspace, size_t workspace_bytes,
                                 cspn_stream_t stream);
int cspn2d_forward_kxk_assemble_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf,
                                    const int* steps, int T, float* out, float* history, size_t history_bytes, int B, int C, int sparse_C,
                                    int H, int W, int K, int dilation, int n_iter, int norm, void* workspace, size_t workspace_bytes,
                                    cspn_stream_t stream);
int cspn2d_backward_kxk_assemble_dil(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* conf,
                                     const int* steps, int T, const float* history, size_t history_bytes, const float* grad_out,
                                     void* grad_guidance, float* grad_blur, float* grad_conf, int B, int C, int sparse_C, int H, int W, int K,
                                     int dilation, int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- K x K propagation pinned to the measured depth with a per-pixel confidence (CSPN++ / PENet: after every step the value at a
 * measured pixel is replaced by the measurement, weighted by a learned confidence): the _kxk_norm_ / _kxk_assemble_ contracts above,
 * dilation included, with the blend after every step
 *     sigma = sign(sparse),   m = sigma * pin_conf,   u = 1 - m
 *     H_{t+1}(p) = u (sum_k wb_k H_t(p + off_k) + cc blur) + m sparse,      H_0 = blur,   cc = 1 - sum_k wb_k
 *   folded as w'_k = u wb_k and b = (u cc) blur + m sparse, evaluated in exactly this form.  sparse enters by its value as well as its
 *   sign; pin_conf is float32 with the planes of sparse ([B,sparse_C,H,W], sparse_C 1 or C) and is used as given: no sigmoid, no clamp.
 *   With pin_conf = 1, sparse >= 0 and blur = sparse where sparse > 0 the results are bitwise those of the unpinned entry points; with
 *   pin_conf = 0 bitwise those of the call without a mask.  The assembled sum over collected levels is unchanged on top of these levels.
 * Gradients, with dw'_k and db_c the gradients of the folded w' and b (i over the images of one guidance image, c over the channels
 *   that share a mask plane):
 *     dwb_k      = sum_i u_i (dw'_{i,k} - sum_c blur_{i,c} db_{i,c})      -> grad_guidance as in the unpinned contract
 *     grad_blur  = A_0 + (u cc) db_c
 *     grad_sparse = m sum_c db_c                                          (through the value; the sign has no derivative)
 *     grad_pin   = sigma (sum_c db_c (sparse - cc blur_c) - sum_k wb_k dw'_k)   (exactly 0 where sparse == 0)
 *   grad_sparse and grad_pin have the planes of sparse and may each be NULL, as may grad_guidance, grad_blur and grad_conf.  grad_pin
 *   needs dw', hence with n_iter >= 2 the forward's history, like grad_guidance.
 * Each entry has the arguments of its _dil counterpart with pin_conf behind sparse (and grad_sparse, grad_pin behind the other
 *   gradients); gate_dtype 0 is float32 guidance, CSPN_DTYPE_F16 / CSPN_DTYPE_BF16 under the rule of the 16-bit block above (float32
 *   results bitwise those on the widened guidance, grad_guidance rounded once).  Workspaces and histories are those of the unpinned
 *   contract: the six cspn2d_*kxk_{norm,assemble}_*_bytes queries apply with the call's sparse_C.  Deterministic: sums in channel order,
 *   every element written once, no atomics.
 * Errors: a NULL sparse or pin_conf, or sparse_C == 0: CSPN_E_BADARG ("pin" in cspn_last_error()), checked first; then every check of
 *   the _dil counterpart, all before anything touches the GPU. */
int cspn2d_forward_kxk_norm_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                float* out, float* history, size_t history_bytes, int B, int C, int sparse_C, int H, int W, int K,
                                int dilation, int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_norm_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                 const float* history, size_t history_bytes, const float* grad_out, void* grad_guidance, float* grad_blur,
                                 float* grad_sparse, float* grad_pin, int B, int C, int sparse_C, int H, int W, int K, int dilation,
                                 int n_iter, int norm, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_forward_kxk_assemble_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                    const float* conf, const int* steps, int T, float* out, float* history, size_t history_bytes, int B,
                                    int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm, void* workspace,
                                    size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_assemble_pin(const void* guidance, int gate_dtype, const float* blur, const float* sparse, const float* pin_conf,
                                     const float* conf, const int* steps, int T, const float* history, size_t history_bytes,
                                     const float* grad_out, void* grad_guidance, float* grad_blur, float* grad_conf, float* grad_sparse,
                                     float* grad_pin, int B, int C, int sparse_C, int H, int W, int K, int dilation, int n_iter, int norm,
                                     void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- non-local propagation with learned offsets (the refinement step of NLSPN and of the models built on it): every pixel reads its
 * K K - 1 neighbours by bilinear interpolation at p + base_k + d_k(p), a modulated deformable convolution with an all-ones weight,
 * iterated on the same offsets and affinities.  K = 3 (KK = 8) only: any other K is CSPN_E_UNSUPPORTED ("K" in cspn_last_error()).
 * Tensors, all float32, contiguous NCHW:
 *     aff    [B,KK,H,W]     used as given, any sign: the caller has normalised them
 *     offset [B,2 KK,H,W]   channel 2k is dy_k, channel 2k + 1 is dx_k (the deformable convolution's layout without the centre pair)
 *     x, out [B,C,H,W]      the C channels share aff and offset
 *     sparse [B,1,H,W] or NULL   measured depth, pinned where > 0
 * Neighbour k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre; its base is base_k = (t - R, l - R), R = K / 2.
 *   THIS IS THE DEFORMABLE CONVOLUTION'S SIGN, THE OPPOSITE OF THE K x K ENTRY POINTS' off_k = (R - t, R - l) above.
 *     m = [sparse > 0] (0 without sparse)      c(p) = 1 - sum_k aff_k(p)      H_0 = x
 *     Ht_t = (1 - m) H_t + m sparse                                            (before every step)
 *     H_{t+1}(p) = c(p) Ht_t(p) + sum_k aff_k(p) bil(Ht_t, p + base_k + d_k(p))      out = H_n (not pinned)
 *     bil(F, p + base + d):  fy = dy - floor(dy), fx = dx - floor(dx)  (the fraction of the OFFSET: exact in float32),
 *                            (y0, x0) = p + base + (floor dy, floor dx) in integer arithmetic,
 *                            (1-fy)(1-fx) F[y0,x0] + (1-fy) fx F[y0,x0+1] + fy (1-fx) F[y0+1,x0] + fy fx F[y0+1,x0+1],
 *                            a corner outside the image contributes 0
 *   Every finite offset is valid (+-1e9 included: floor d is clamped before it is converted, everything out there is outside the image).
 *   A NaN or infinite offset gives an unspecified value but never an access outside the tensors.  n_iter = 0 copies x.
 * Gradients, A_n = grad_out, for t = n-1 .. 0:
 *     At_t(q) = c(q) A_{t+1}(q) + sum_{p,k} aff_k(p) w_{p,k->q} A_{t+1}(p)     (the transpose of the gather: a scatter)
 *     A_t = (1 - m) At_t,   grad_x = A_0,   sparse gets no gradient
 *     grad_aff_k(p) = sum_t sum_c A_{t+1}(p) (bil_k(Ht_t)(p) - Ht_t(p))
 *     grad_dy_k(p)  = sum_t sum_c A_{t+1}(p) aff_k(p) [(1-fx)(F[y0+1,x0] - F[y0,x0]) + fx (F[y0+1,x0+1] - F[y0,x0+1])], F = Ht_t, outside 0;
 *     grad_dx_k likewise in x: floor has zero derivative and d fy / d dy = 1.
 *   grad_aff, grad_offset and grad_x may each be NULL.  grad_aff and grad_offset need, for n_iter >= 2, the history of a forward with the
 *   same arguments.
 * THE BACKWARD IS NOT RUN-TO-RUN BITWISE, the first such path of this library: the scatter adds with float atomics (one hardware
 *   float add each, no compare-and-swap loop) in arrival order, so At_t and through it every gradient can differ in its last bits between
 *   two identical calls.  The forward and cspn2d_nl_sample_f32 are bitwise reproducible; cspn2d_nl_sample_backward_f32's grad_f is not.
 *   cspn2d_backward_nl_det_f32 and cspn2d_nl_sample_backward_det_f32 (below) are run-to-run bitwise in every gradient.
 * history: H_1 .. H_{n-1} as the steps store them (pinned), cspn2d_nl_history_bytes() bytes.  Workspaces, 256-byte aligned:
 *   cspn2d_nl_workspace_bytes(.., n_iter, has_sparse) for a forward without a history; with one, the levels go to the history and the
 *   forward needs cspn2d_nl_workspace_bytes(.., 1, has_sparse) (the pinned H_0).  cspn2d_backward_nl_workspace_bytes(): At_1 .. At_{n-1}
 *   and, with sparse, the pinned H_0.
 * cspn2d_nl_sample_f32: the sampling operator on its own, out_k(p) = bil(f, p + base_k + d_k(p)), f [B,1,H,W] -> out [B,KK,H,W]
 *   (confidence-modulated affinities need it); its backward gives grad_f [B,1,H,W] by the scatter and grad_offset [B,2 KK,H,W] written
 *   once, each may be NULL.
 * Errors, as cspn2d_forward_kxk_f32 / cspn2d_backward_kxk_f32: a null input, a size <= 0, n_iter < 0, or an output, history or
 *   workspace overlapping an input or another output: CSPN_E_BADARG; K != 3, or B C H W or B 2KK H W above 2^31 - 1 elements:
 *   CSPN_E_UNSUPPORTED; a workspace or history too small, or a workspace not 256-byte aligned: CSPN_E_WORKSPACE.  The byte queries return
 *   0 where nothing is needed or the shape is invalid.  Any 4-byte aligned pointers and any H, W >= 1; 16-byte loads of aff, offset and the
 *   levels where W % 4 == 0 and the pointers are 16-byte aligned. */
size_t cspn2d_nl_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse);
size_t cspn2d_nl_history_bytes(int B, int C, int H, int W, int K, int n_iter);
int cspn2d_forward_nl_f32(const float* aff, const float* offset, const float* x, const float* sparse, float* out, float* history,
                          size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* workspace, size_t workspace_bytes,
                          cspn_stream_t stream);
size_t cspn2d_backward_nl_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse);
int cspn2d_backward_nl_f32(const float* aff, const float* offset, const float* x, const float* sparse, const float* history,
                           size_t history_bytes, const float* grad_out, float* grad_aff, float* grad_offset, float* grad_x, int B, int C,
                           int H, int W, int K, int n_iter, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_nl_sample_f32(const float* offset, const float* f, float* out, int B, int H, int W, int K, cspn_stream_t stream);
int cspn2d_nl_sample_backward_f32(const float* offset, const float* f, const float* grad_out, float* grad_f, float* grad_offset, int B,
                                  int H, int W, int K, cspn_stream_t stream);

/* ---- the same two backwards, RUN-TO-RUN BITWISE (cspn2d_nl_det.hip): a deterministic function of their inputs, with no float atomics.
 * The contract, arguments, error rules and messages are those of cspn2d_backward_nl_f32 / cspn2d_nl_sample_backward_f32 above; the
 * sampling backward takes a workspace here (the scatter form takes none), in the argument order of cspn2d_backward_nl_f32, and the
 * workspace may alias no tensor.  Results agree with the scatter forms within rounding, not bit for bit.
 * The adjoint of the gather is formed as a gather: per call (it is the same for all n_iter steps) an inverted index of the operator is
 * built in CSR form over the P = B H W destinations q -- count the taps per destination (integer atomics), an exclusive scan of the P
 * counts (three plain passes), fill the lists (an integer atomic cursor per destination).  An entry is 8 bytes: the uint32 code
 * p 32 + k 4 + corner (p the source pixel within the image) and the float32 coefficient fl32(aff_k(p) w_corner(p, k)) (the sampling
 * operator: w alone); only taps with a non-zero weight enter.  The starts are uint32: at most 32 P <= 2^32 - 2 entries, by the guard
 * B 2KK H W <= 2^31 - 1.  The order of a list's entries is arbitrary; the sum does not depend on it:
 *     terms   tau_0 = fl32(c(q) A_{t+1}(q)),  tau_i = fl32(coef_i A_{t+1}(p_i));  m of them
 *     e = floor(log2 max |tau_i|),  L = ceil(log2 m),  s = 61 - e - L
 *     q_i = llrint(ldexp((double)tau_i, s))   (exact scaling, round to nearest even, |q_i| <= 2^(62 - L)),  S = sum q_i in int64 (associative)
 *     At_t(q) = ldexpf((float)S, -s)  (one rounding to nearest);  A_t = (1 - m(q)) At_t(q) is what is stored
 *   all terms zero: +0; a NaN term, or infinities of both signs: the quiet NaN 0x7fc00000; else an infinite term: that infinity.  The
 *   result is a function of the multiset of terms alone.  Its error against the exact sum of the tau_i is one float32 rounding plus at
 *   most m 2^(-s-1) <= 2^(2L - 62) max |tau_i|.  Lists of more than 128 entries are summed by a whole wave (the integer sum makes any
 *   split reproducible), shorter ones by one lane.  grad_aff / grad_offset come from the kernel of the scatter form (every element
 *   written once, sums in a fixed order) on these levels; the sampling backward's grad_offset likewise.
 * Workspaces, 256-byte aligned, closed forms with r(b) = b rounded up to a multiple of 256 and P = B H W:
 *     index(P, c) = 256 + r(4 (P + 1)) + r(4 P) + c r(4 P) + r(4 (P / 4 + 1)) + r(4 ceil(P / 2048)) + 256 P
 *                   (the worklist counter, the starts, the fill cursors, the plane c(q), the worklist, the scan's partials, the entries)
 *     cspn2d_backward_nl_det_workspace_bytes(..)        = cspn2d_backward_nl_workspace_bytes(..) + index(P, 1)      (the levels first;
 *                                                          0 for n_iter = 0: the identity has no adjoint step)
 *     cspn2d_nl_sample_backward_det_workspace_bytes(..) = index(P, 0)
 *   about 270 bytes a pixel beyond the scatter form's.  Both are pure host arithmetic and return 0 for every argument set for which the
 *   queries above return 0.  Everything the index reads before it writes (counts, cursors, the worklist counter) is zeroed by the call
 *   itself, in stream order. */
size_t cspn2d_backward_nl_det_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse);
int cspn2d_backward_nl_det_f32(const float* aff, const float* offset, const float* x, const float* sparse, const float* history,
                               size_t history_bytes, const float* grad_out, float* grad_aff, float* grad_offset, float* grad_x, int B,
                               int C, int H, int W, int K, int n_iter, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_nl_sample_backward_det_workspace_bytes(int B, int H, int W, int K);
int cspn2d_nl_sample_backward_det_f32(const float* offset, const float* f, const float* grad_out, float* grad_f, float* grad_offset,
                                      int B, int H, int W, int K, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the six non-local entry points on fp16 / bf16 affinities and offsets: what a head under mixed precision emits, taken as it is.
 * Each mirrors its _f32 twin above, with a dtype code right behind the pointer it describes: aff is stored as aff_dtype, offset as
 * offset_dtype, each 0 (float32), CSPN_DTYPE_F16 or CSPN_DTYPE_BF16.  grad_aff is stored as aff_dtype, grad_offset as offset_dtype.  x, sparse,
 * out, history, grad_out, grad_x, f, grad_f and every workspace level stay float32: the byte queries of the twins serve these calls
 * unchanged, and no widened copy of aff or offset is made anywhere.
 *     pair (aff_dtype, offset_dtype)
 *     (0, 0)    the float32 kernels: bitwise the _f32 entry point
 *     (0, T)    float32 affinities (normalised in float32 by the caller, as NonLocal_Propagate does) on offsets as emitted
 *     (T, T)    both 16-bit, T = CSPN_DTYPE_F16 or CSPN_DTYPE_BF16
 *   (T, 0) and fp16 mixed with bf16: CSPN_E_UNSUPPORTED; a code outside {0, 1, 2}: CSPN_E_BADARG; both with "dtype" in cspn_last_error().
 * The contract is the twins' with two storage types: a 16-bit value is widened to float32 exactly where it is read (fp16 subnormals kept,
 *   bf16 = its bits shifted left by 16), after which every operation is the float32 kernel's.  So the fraction d - floor(d) is the widened
 *   offset's, every finite 16-bit offset is valid, and an fp16 offset that has overflowed to +-inf, or a NaN, gives an unspecified value but
 *   never an access outside the tensors (every corner is outside the image, through the same clamp).
 *     out, history     bitwise cspn2d_forward_nl_f32 on the widened aff and offset, on the vector and on the guarded scalar kernels
 *     _det backwards   grad_x (grad_f) bitwise the _det_f32 twin on the widened tensors; grad_aff / grad_offset bitwise that twin's float32
 *                      value rounded once, to nearest even (fp16 subnormals kept), at its single store
 *     scatter backwards  the same within the scatter's run-to-run differences
 *     cspn2d_nl_sample_g16   bitwise cspn2d_nl_sample_f32 on the widened offset
 * Checks: the twins', in their order and with their messages (null pointers, shape, n_iter, K != 3, the 32-bit indexing guard, history,
 *   workspace, aliasing with the ranges of aff, offset and their gradients counted in the stored element size); the dtype checks come last.
 *   A 16-bit tensor must be 2-byte aligned.  8-byte loads of four 16-bit values (16-byte loads of float32 ones) in the forward where
 *   W % 4 == 0 and every tensor is aligned to four of its elements; any other alignment or width takes the guarded scalar kernel. */
int cspn2d_forward_nl_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse, float* out,
                          float* history, size_t history_bytes, int B, int C, int H, int W, int K, int n_iter, void* workspace,
                          size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_nl_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse,
                           const float* history, size_t history_bytes, const float* grad_out, void* grad_aff, void* grad_offset, float* grad_x,
                           int B, int C, int H, int W, int K, int n_iter, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_nl_det_g16(const void* aff, int aff_dtype, const void* offset, int offset_dtype, const float* x, const float* sparse,
                               const float* history, size_t history_bytes, const float* grad_out, void* grad_aff, void* grad_offset,
                               float* grad_x, int B, int C, int H, int W, int K, int n_iter, void* workspace, size_t workspace_bytes,
                               cspn_stream_t stream);
int cspn2d_nl_sample_g16(const void* offset, int offset_dtype, const float* f, float* out, int B, int H, int W, int K, cspn_stream_t stream);
int cspn2d_nl_sample_backward_g16(const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f, void* grad_offset,
                                  int B, int H, int W, int K, cspn_stream_t stream);
int cspn2d_nl_sample_backward_det_g16(const void* offset, int offset_dtype, const float* f, const float* grad_out, float* grad_f,
                                      void* grad_offset, int B, int H, int W, int K, void* workspace, size_t workspace_bytes,
                                      cspn_stream_t stream);

/* ---- the demo module's contract (reference cspn_paddle/demo.py:20-54) inside the K x K engine, K = 5 or 7: guide [B,KK,H,W] raw, any
 * sign, in the channel order of the NONE op; x / out [B,C,H,W], the C channels share the guide.  With a_k = |g_k| and
 * S(p) = sum_k a_k(p), summed in channel order in float32:
 *     H_{t+1}(p) = (sum_k a_k(p) H_t(p + off_k)) * (1 / S(p))      H_0 = x, out = H_n, zero outside the image
 *     A_t(q)     = sum_k a_k(q - off_k) A_{t+1}(q - off_k) * (1 / S(q - off_k)),   A_n = grad_out, grad_x = A_0
 *     dW_k(p)    = sum_{t<n} sum_c A_{t+1}(p) H_t(p + off_k),   grad_guide_k = sign(g_k) (dW_k - (sum_j a_j dW_j) / S) / S,  sign(0) = 0
 *   what cspn_gate_absnorm_f32 followed by cspn2d_forward_kxk_f32 computes, up to rounding (the scale is applied once, after the sum),
 *   without the normalised gates: no tensor of the guide's size is written, read back or kept.  A pixel whose KK gates are all zero
 *   gives NaN (0 * inf), as 0 / 0 there.
 * history, the forward's workspace and their byte counts are those of cspn2d_forward_kxk_f32 (cspn2d_kxk_workspace_bytes,
 * cspn2d_kxk_history_bytes).  The backward's workspace (cspn2d_backward_kxk_absnorm_workspace_bytes) keeps A_1 .. A_{n-1} and one
 * float32 plane [B,H,W] of 1 / S; 0 for n_iter <= 1.  The _g16 twins take a guide of gate_dtype under the rule of the 16-bit block above:
 * out and grad_x bitwise the _f32 entry point's on the widened guide, grad_guide its float32 value rounded once.  No atomics.
 * Arguments, alignment and error codes exactly as cspn2d_forward_kxk_f32 / _g16 and cspn2d_backward_kxk_f32 / _g16. */
int cspn2d_forward_kxk_absnorm_f32(const float* guide, const float* x, float* out, float* history, size_t history_bytes,
                                   int B, int C, int H, int W, int K, int n_iter,
                                   void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_forward_kxk_absnorm_g16(const void* guide, int gate_dtype, const float* x, float* out, float* history, size_t history_bytes,
                                   int B, int C, int H, int W, int K, int n_iter,
                                   void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_kxk_absnorm_workspace_bytes(int B, int C, int H, int W, int K, int n_iter);
int cspn2d_backward_kxk_absnorm_f32(const float* guide, const float* x, const float* history, size_t history_bytes, const float* grad_out,
                                    float* grad_guide, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                                    void* workspace, size_t workspace_bytes, cspn_stream_t stream);
int cspn2d_backward_kxk_absnorm_g16(const void* guide, int gate_dtype, const float* x, const float* history, size_t history_bytes,
                                    const float* grad_out, void* grad_guide, float* grad_x, int B, int C, int H, int W, int K, int n_iter,
                                    void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- K x K propagation with per-step attention (the "dynamic, centre-sited" contract), K = 3, 5 or 7, R = K / 2, KK = K*K - 1, float32,
 * contiguous NCHW.  Where every contract above uses the same affinities on every step, here a small head emits an attention for every step
 * and every distance ring of the neighbourhood, plus one for the pixel itself; the affinities are re-weighted and re-normalised on each step.
 *   guidance [B,KK,H,W]        raw, any sign, centre-sited (read at p), in the channel order of the NONE op: off_k = (R - t, R - l)
 *   att      [B,n (R+1),H,W]   used as given, any sign; channel t (R+1) + r: r = 0 is the pixel's own term of step t (it only enters the
 *                              divisor), r >= 1 is ring r of step t, ring(k) = max(|dy|, |dx|) of off_k
 *   x / out  [B,C,H,W]         the C channels share guidance and att
 *   sparse   [B,1,H,W] or NULL pinned where > 0: the level is pinned before every step, out = H_n is not
 * With m = [sparse > 0], H_0 = x, Ht_t = (1 - m) H_t + m sparse:
 *     wh_k = att_{t,ring(k)}(p) g_k(p)     D_t(p) = att_{t,0}(p) + sum_k |wh_k|     w_k = wh_k / D_t     c_t = 1 - sum_k w_k
 *     H_{t+1}(p) = c_t(p) Ht_t(p) + sum_k w_k(p) Ht_t(p + off_k)
 *   a neighbour outside the image contributes 0 (its w_k still counts in D and c).  The sum runs on wh_k in channel order and is scaled by
 *   1 / D_t once, after it; c_t is formed as (att_{t,0} + sum_k (|wh_k| - wh_k)) / D_t.
 * Backward, A_n = grad_out, e_k = sum_c A_{t+1}(p) (Ht_t(p + off_k) - Ht_t(p)), T = sum_k w_k e_k:
 *     At_t(q) = c_t(q) A_{t+1}(q) + sum_k wh_k(q') (A_{t+1} / D_t)(q'),  q' = q - off_k      A_t = (1 - m) At_t      grad_x = A_0
 *     dL/dwh_k = (e_k - sign(wh_k) T) / D_t      grad_att_{t,0} = -T / D_t      grad_att_{t,r} = sum_{k in ring r} g_k dL/dwh_k
 *     grad_guidance_k = sum_t att_{t,ring(k)} dL/dwh_k                                       sign(0) = 0; sparse has no gradient
 * D_t = 0 gives the non-finite pattern of these formulas; nothing is guarded.  No modulated or normalised gate and no gradient of one is stored:
 * guidance and att are the only gate-sized tensors.  No atomics: forward and backward are run-to-run bitwise.
 * history (optional in the forward): Ht_1 .. Ht_{n-1}, [n-1][B][C][H][W], (n_iter - 1) B C H W floats -- cspn2d_kxk_history_bytes for K = 5 / 7,
 *   the same count (cspn2d_kxk_norm_history_bytes) for K = 3; grad_guidance and grad_att need it where n_iter >= 2.
 * Workspaces: cspn2d_kxk_dyn_workspace_bytes(..., has_sparse, keep_history) holds the pinned H_0 (with sparse) and, without a history, the
 *   ping-pong levels; cspn2d_backward_kxk_dyn_workspace_bytes(..., has_sparse) holds A_1 .. A_{n-1}, 2 R planes [B,H,W] of ring sums of the
 *   guidance and (with sparse) the pinned H_0.  Both are pure host arithmetic, multiples of 256, and 0 wherever the arguments are rejected
 *   (K not 3 / 5 / 7, a size <= 0, n_iter <= 0, a tensor of more than 2^31 - 1 elements).
 * grad_guidance (summed over C), grad_att and grad_x may each be NULL.  n_iter == 0: out = x, grad_x = grad_out, grad_guidance = 0.
 * Arguments, ranges, alignment (workspace 256 bytes; any tensor alignment is taken, 16-byte aligned tensors with W % 4 == 0 run the vector
 * kernels) and error codes as the kxk_absnorm entry points; att, grad_att and sparse take part in the aliasing checks.  B n (R+1) H W beyond
 * 2^31 - 1 is CSPN_E_UNSUPPORTED; the attention planes are addressed in size_t throughout. */
size_t cspn2d_kxk_dyn_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse, int keep_history);
int cspn2d_forward_kxk_dyn_f32(const float* guidance, const float* att, const float* x, const float* sparse, float* out, float* history,
                               size_t history_bytes, int B, int C, int H, int W, int K, int n_iter,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_kxk_dyn_workspace_bytes(int B, int C, int H, int W, int K, int n_iter, int has_sparse);
int cspn2d_backward_kxk_dyn_f32(const float* guidance, const float* att, const float* x, const float* sparse, const float* history,
                                size_t history_bytes, const float* grad_out, float* grad_guidance, float* grad_att, float* grad_x,
                                int B, int C, int H, int W, int K, int n_iter,
                                void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- line-scan propagation: the linear, three-way scan-line recurrence of SPN ("Learning Affinity via Spatial Propagation Networks"), the
 * contract "line scan, three-way".  IT WAS WRITTEN FROM THE PUBLISHED DESCRIPTION, NOT FROM A SOURCE: compare it with your model before you
 * port it.  Tensors are float32, contiguous NCHW.
 *   x     [B,C,H,W]
 *   dirs  a non-empty subset of {0: left->right, 1: right->left, 2: top->bottom, 3: bottom->top} as a 4-bit mask (bit c = direction c, 1 .. 15);
 *         D is its size, the directions are numbered d = 0 .. D-1 in ascending order of their code
 *   gates [B,D Cg 3,H,W]   channel (d Cg + j) 3 + k; Cg divides C and channel c uses group j = c / (C / Cg): Cg = 1 is shared gates, Cg = C is
 *                          SPN's per-channel gates.  Gates are used AS GIVEN (any sign, no normalisation in the engine)
 *   lam   [B,D C,H,W] or NULL        out [B,D C,H,W], channel d C + c
 * For one direction, t is the coordinate along the scan and i the coordinate along the line.  Directions 0 / 1: a line is a column, t is the
 * column index, ascending for 0 and descending for 1, and i is the row.  Directions 2 / 3: a line is a row, t is the row index, i the column.
 * L is the line length, t- the line visited just before t, k in {0,1,2} the connection to h(i + k - 1, t-):
 *     g^_k(i,t) = g_k(i,t)  if t is not the first line and 0 <= i + k - 1 < L,   else 0
 *     b(i,t)    = lam(i,t)  if lam is given,   else 1 - sum_k g^_k(i,t)
 *     h(i,t)    = b(i,t) x(i,t) + sum_k g^_k(i,t) h(i + k - 1, t-)                  (first line: h = b x)
 *
 *     A(i,t)    = grad_out(i,t) + sum_k g^_k(i - (k-1), t+) A(i - (k-1), t+)        (t+: the line visited after t; last line: A = grad_out)
 *     grad_x    = sum_d b A            grad_lam = A x (lam given)
 *     grad_g_k  = sum_{c in group} A (h(i + k - 1, t-) - x(i,t))  without lam,   sum_{c in group} A h(i + k - 1, t-)  with lam;
 *                 exactly 0 wherever g^_k is the dropped 0
 * The backward reads x, gates, lam, out (the forward's own result is the only history) and grad_out.  Each of grad_x, grad_gates and grad_lam
 * may be NULL (grad_lam without lam is CSPN_E_BADARG).  Nothing is guarded: gates with sum |g| > 1 diverge as the formulas do.
 * One launch runs all directions, images, channels and steps of the forward; the backward is one launch plus at most one fixed-order reduction
 * launch.  No atomics: forward and backward are run-to-run bitwise.
 * A line (H for directions 0 / 1, W for 2 / 3) has at most 2048 pixels: beyond that, and for a tensor of more than 2^31 - 1 elements, the calls
 * return CSPN_E_UNSUPPORTED and the byte queries 0.  The scan itself may be of any length.
 * Workspaces: pure host arithmetic, multiples of 256, 0 wherever the arguments are rejected (Cg not dividing C, dirs outside 1 .. 15, a size
 * <= 0, the limits above) and >= 256 otherwise.  The forward's holds no tensor (256 bytes); the backward's holds grad_x of the directions
 * d >= 1 ((D - 1) B C H W floats) and grad_gates of the channels beyond a group's first ((C / Cg - 1) B D Cg 3 H W floats).
 * Arguments, ranges, alignment (workspace 256 bytes; any tensor alignment and any H, W >= 1 is taken) and error codes as the kxk_dyn entry
 * points: out / the gradients must not alias an input, each other or the workspace. */
size_t cspn2d_scan_workspace_bytes(int B, int C, int Cg, int H, int W, int dirs, int has_lam);
int cspn2d_forward_scan_f32(const float* x, const float* gates, const float* lam, float* out, int B, int C, int Cg, int H, int W, int dirs,
                            void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_scan_workspace_bytes(int B, int C, int Cg, int H, int W, int dirs, int has_lam);
int cspn2d_backward_scan_f32(const float* x, const float* gates, const float* lam, const float* out, const float* grad_out, float* grad_x,
                             float* grad_gates, float* grad_lam, int B, int C, int Cg, int H, int W, int dirs,
                             void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the steps right next to the path, on the device ----
 * cspn_metrics_f32: reference cspn_pytorch/utils.py:19-47 (evaluate_error) and loss.py:16-23 (Wighted_L1_Loss = MAE
 * over gt > 1e-4) as one fused masked reduction over n elements.  out12 (device, 12 floats):
 *   [0] n_valid  [1] MSE  [2] RMSE  [3] ABS_REL  [4] LG10 (the reference never fills it: 0)  [5] MAE
 *   [6..11] DELTA1.02, 1.05, 1.10, 1.25, 1.25^2, 1.25^3.   All zero when no element is valid (utils.py:23-26).
 * cspn_l1_backward_f32: d(Wighted_L1_Loss)/d(pred) = grad_scale[0] * sign(pred - label) / n_valid on label > 1e-4;
 *   stats12 = the out12 of cspn_metrics_f32(label, pred), grad_scale = 1 device float.
 * cspn_unpool_f32: reference models/torch_resnet_cspn_nyu.py:41-54 (Unpool: conv_transpose2d with a one-hot
 *   stride x stride kernel): out[nc][y*stride][x*stride] = x[nc][y][x], zeros elsewhere; x [NC,H,W] -> out [NC,H*s,W*s]. */
size_t cspn_metrics_workspace_bytes(size_t n);
int cspn_metrics_f32(const float* gt, const float* pred, size_t n, float* out12, void* workspace, size_t workspace_bytes,
                     cspn_stream_t stream);
int cspn_l1_backward_f32(const float* pred, const float* label, const float* stats12, const float* grad_scale,
                         float* grad_pred, size_t n, cspn_stream_t stream);
int cspn_unpool_f32(const float* x, float* out, size_t NC, int H, int W, int stride, cspn_stream_t stream);
int cspn_unpool_backward_f32(const float* grad_out, float* grad_x, size_t NC, int H, int W, int stride, cspn_stream_t stream);

/* cspn_sparse_sample_f32: reference createSparseDepthImage on the device -- sparse = depth * bernoulli(p), p = n_sample /
 * (pixels per image) for mode 0 (cspn_pytorch/nyu_dataset_loader.py:135-144) or n_sample / (pixels of that image with
 * depth > 1e-4) for mode 1 (cspn_pytorch/kitti_dataset_loader.py:138-148).  depth, sparse_out: [n_images][hw] floats.
 * Counter-based generator keyed by (seed, image, pixel): reproducible, independent of launch geometry; NOT the bit stream
 * of torch.bernoulli.  workspace: cspn_sparse_sample_workspace_bytes(n_images) (only used by mode 1). */
size_t cspn_sparse_sample_workspace_bytes(size_t n_images);
int cspn_sparse_sample_f32(const float* depth, float* sparse_out, size_t n_images, size_t hw, int n_sample, int mode,
                           unsigned long long seed, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the producer of the path's inputs (producer half): the two heads Simple_Gudi_UpConv_Block_Last_Layer of the reference backbone
 * (cspn_pytorch/models/torch_resnet_cspn_nyu.py:187-206; gud_up_proj_layer6 64 -> 8 = guidance and gud_up_proj_layer5 64 -> 1 = blur depth, :318-319,
 * called :372-373) as ONE kernel: Unpool (:41-54, narrowed to H x W :196-201) + 3x3 conv, padding 1, no bias (:190) -- the three quarters of the
 * unpooled taps that are structurally zero are never multiplied.
 *   x [B,C,h,w];  w_guidance [8,C,3,3];  w_blur [1,C,3,3] or NULL;  guidance_out [B,8,H,W];  blur_out [B,1,H,W] or NULL;  H <= 2h, W <= 2w (the reference: exactly 2x).
 *   norm_type CSPN_NORM_NONE: guidance_out = the raw guidance, what gud_up_proj_layer6 returns (feed it to cspn2d_forward_f32 with '8sum' / '8sum_abs');
 *   CSPN_NORM_8SUM / CSPN_NORM_8SUM_ABS: guidance_out = gate_wb = affinity_normalization (cspn.py:85-144) of that guidance, fused behind the conv (IEEE
 *   division: 0 / 0 = NaN as in the reference) -- the input contract of cspn2d_forward_f32 with CSPN_NORM_PRENORM; no stand-alone normalisation pass.
 * workspace: cspn_guidance_head_workspace_bytes(C) (the packed weights). */
size_t cspn_guidance_head_workspace_bytes(int C);
int cspn_guidance_head_f32(const float* x, const float* w_guidance, const float* w_blur, float* guidance_out, float* blur_out,
                           int B, int C, int h, int w, int H, int W, int norm_type,
                           void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- 2D, C channels on SHARED guidance (reference cspn.py:58-81 only multiplies and broadcasts: a blur_depth [B,C,H,W] is propagated
 * channel by channel on the same normalised affinities; the Paddle contract says the same, cspn_paddle/README.md:56).
 *   guidance [B,8,H,W] (or gate_wb for PRENORM), blur / out / grad_out / grad_blur [B,C,H,W],
 *   sparse NULL, [B,1,H,W] (sparse_channels 1: one mask for every channel) or [B,C,H,W] (sparse_channels C)
 *   grad_guidance [B,8,H,W] = the gradient SUMMED over the channels (what autograd accumulates into the shared tensor).
 * cspn2d_multi_supported() != 0 where the shared-gate fast path takes the call: ONE ring launch per pass over the B*C image-channels (image-channel
 * b*C + c reads guidance image b), so a short batch of several channels fills the device the way a longer batch does; a shared mask is widened
 * to [B,C,H,W] in the workspace first.  The backward's two sweeps run over the B*C image-channels as well; its final pass runs once per channel and
 * adds that channel's part of grad_guidance to the previous ones (channel order: deterministic).  Everywhere else (W < 256, W % 4 != 0,
 * other n_iter, the STEPWISE / FUSED_CXX / FUSED_PADDED algos, misaligned tensors) the library loops over the channels itself (each channel
 * gathered into the workspace, propagated by the single-channel entry point, scattered back; the guidance gradients summed by a HIP kernel):
 * the same results as a per-channel loop of the single-channel calls.  The history pair (training mode) only where the fast path holds
 * (cspn2d_history_bytes_multi() > 0).  `B*C*H*W` is bounded like `B*H*W` of the single-channel calls.  With C = 1 (and sparse_channels 1)
 * every entry point runs the single-channel one it mirrors. */
size_t cspn2d_workspace_bytes_multi(int B, int C, int H, int W, int n_iter);
int cspn2d_multi_supported(int B, int C, int H, int W, int n_iter);
int cspn2d_forward_multi_f32(const float* guidance, const float* blur, const float* sparse, float* out, int B, int C, int sparse_channels,
                             int H, int W, int n_iter, int norm_type, int algo, void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_history_bytes_multi(int B, int C, int H, int W, int n_iter);
int cspn2d_forward_history_multi_f32(const float* guidance, const float* blur, const float* sparse, float* out, void* history,
                                     size_t history_bytes, int B, int C, int sparse_channels, int H, int W, int n_iter, int norm_type,
                                     void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_multi_workspace_bytes(int B, int C, int H, int W, int n_iter);
int cspn2d_backward_multi_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out, float* grad_guidance,
                              float* grad_blur, int B, int C, int sparse_channels, int H, int W, int n_iter, int norm_type,
                              void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn2d_backward_history_multi_workspace_bytes(int B, int C, int H, int W, int n_iter);
int cspn2d_backward_history_multi_f32(const float* guidance, const float* blur, const float* sparse, const float* grad_out,
                                      const void* history, size_t history_bytes, float* grad_guidance, float* grad_blur, int B, int C,
                                      int sparse_channels, int H, int W, int n_iter, int norm_type, void* workspace, size_t workspace_bytes,
                                      cspn_stream_t stream);

/* The gradient of the raw heads (norm_type NONE above): what torch autograd computes through the two reference layers when the training loop back-propagates
 * through torch_resnet_cspn_nyu.py:372-373.  grad_guidance [B,8,H,W] and grad_blur [B,1,H,W] (with w_blur; both or neither) are dL/d(outputs);
 *   grad_x          [B,C,h,w]   dL/dx = sum_{o,ky,kx} W[o][c][ky][kx] g[o][2i + 1 - ky][2j + 1 - kx]   (inputs beyond the narrowed output: 0), or NULL to skip
 *   grad_w_guidance [8,C,3,3], grad_w_blur [1,C,3,3]   dL/dW = sum over the batch and all input pixels of x g -- on the matrix cores (fp32 MFMA), the waves'
 *                   partial sums added in a fixed order: deterministic; either or both may be NULL
 * workspace: cspn_guidance_head_backward_workspace_bytes(B, C, h, w) bytes, 256-byte aligned. */
size_t cspn_guidance_head_backward_workspace_bytes(int B, int C, int h, int w);
int cspn_guidance_head_backward_f32(const float* x, const float* w_guidance, const float* w_blur, const float* grad_guidance, const float* grad_blur,
                                    float* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w, int H, int W,
                                    void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the guidance heads for K x K propagation: Simple_Gudi_UpConv_Block_Last_Layer(C, K*K-1, ...) (the class takes the plane count as an argument) with the
 * 1-plane blur head riding along -- the producer of what cspn2d_forward_kxk_norm_f32 consumes.  Raw guidance only (the K x K contract normalises in its own fold).
 *   x [B,C,h,w];  w_guidance [K*K-1,C,3,3];  w_blur [1,C,3,3] or NULL;  guidance_out / grad_guidance [B,K*K-1,H,W];  blur_out / grad_blur [B,1,H,W] or NULL
 *   (with w_blur: both or neither);  H <= 2h, W <= 2w;  grad_x [B,C,h,w], grad_w_guidance [K*K-1,C,3,3], grad_w_blur [1,C,3,3]: each may be NULL (skipped).
 *   K = 5 or 7: three GEMMs on the matrix cores in exact fp32 (v_mfma_f32_32x32x2_f32); the weight gradients' partial sums are added in a fixed order (no
 *   atomics: deterministic).  K = 3 forwards to cspn_guidance_head_f32 (CSPN_NORM_NONE) / cspn_guidance_head_backward_f32: bitwise their results.
 *   Any other K, H > 2h, W > 2w or a w_blur without blur_out / grad_blur: CSPN_E_BADARG.
 * workspace: the matching *_workspace_bytes(B, C, h, w, K) bytes, 256-byte aligned; too small or misaligned: CSPN_E_WORKSPACE from both calls. */
size_t cspn_guidance_head_kxk_workspace_bytes(int B, int C, int h, int w, int K);
int cspn_guidance_head_kxk_f32(const float* x, const float* w_guidance, const float* w_blur, float* guidance_out, float* blur_out,
                               int B, int C, int h, int w, int H, int W, int K,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn_guidance_head_kxk_backward_workspace_bytes(int B, int C, int h, int w, int K);
int cspn_guidance_head_kxk_backward_f32(const float* x, const float* w_guidance, const float* w_blur, const float* grad_guidance, const float* grad_blur,
                                        float* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w, int H, int W, int K,
                                        void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the same heads on a 16-bit feature map (what a backbone under autocast hands over), dtype CSPN_DTYPE_F16 or CSPN_DTYPE_BF16 = DT, K = 5 or 7 only (the
 * 8-plane head of K = 3 has no 16-bit guidance, its ring has no 16-bit consumer: cspn_guidance_head_g16 below) -- the producer of what cspn2d_forward_kxk_norm_g16 consumes.
 *   x [B,C,h,w], guidance_out / grad_guidance [B,K*K-1,H,W] and grad_x [B,C,h,w] are DT;  w_guidance, w_blur (the master weights), blur_out / grad_blur
 *   [B,1,H,W] and grad_w_guidance / grad_w_blur are float32.
 *   The weights are rounded once to DT (to nearest even) in the per-call repack; every product is of two DT values, exact in float32; the sums accumulate in
 *   float32 on the matrix cores (v_mfma_f32_32x32x16_f16 / _bf16).  guidance_out is the accumulator rounded once to DT (to nearest even, overflow to +-inf as
 *   a cast); blur_out is the accumulator, unrounded.  grad_guidance arrives in DT (what cspn2d_backward_kxk_norm_g16 returns); grad_blur arrives in float32
 *   and is ROUNDED ONCE TO DT as it enters the GEMMs -- what a 16-bit convolution's backward would have received; grad_x is rounded once to DT; the weight
 *   gradients are the float32 accumulators, their partial sums added in a fixed order (no atomics: deterministic, every element written once).
 *   All checks of the _f32 twins apply; K = 3 or any other K, an unknown dtype or a 16-bit pointer that is not 2-byte aligned: CSPN_E_BADARG.
 * workspace: the matching *_g16_workspace_bytes(B, C, h, w, K) bytes, 256-byte aligned; too small or misaligned: CSPN_E_WORKSPACE. */
size_t cspn_guidance_head_kxk_g16_workspace_bytes(int B, int C, int h, int w, int K);
int cspn_guidance_head_kxk_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, void* guidance_out, float* blur_out,
                               int B, int C, int h, int w, int H, int W, int K,
                               void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn_guidance_head_kxk_backward_g16_workspace_bytes(int B, int C, int h, int w, int K);
int cspn_guidance_head_kxk_backward_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, const void* grad_guidance,
                                        const float* grad_blur, void* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w,
                                        int H, int W, int K, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

/* ---- the 3 x 3 model's heads (8 guidance planes + the blur plane, raw) on a 16-bit feature map, dtype CSPN_DTYPE_F16 or CSPN_DTYPE_BF16 = DT, feeding the
 * float32 rings: the producer of what cspn2d_forward_f32 / Affinity_Propagate consume, with no widening pass on either side.
 *   x [B,C,h,w] and grad_x [B,C,h,w] are DT;  w_guidance [8,C,3,3], w_blur [1,C,3,3] (the master weights), guidance_out / grad_guidance [B,8,H,W], blur_out /
 *   grad_blur [B,1,H,W] and grad_w_guidance / grad_w_blur are float32.
 *   The weights are rounded once to DT (to nearest even) in the per-call repack; every product is of two DT values, exact in float32; the sums accumulate in
 *   float32 on the matrix cores (v_mfma_f32_16x16x32_f16 / _bf16 forward, v_mfma_f32_32x32x16 backward).  guidance_out and blur_out are the accumulators,
 *   UNROUNDED.  grad_guidance and grad_blur arrive in float32 (what cspn2d_backward_f32 returns) and are ROUNDED ONCE TO DT as they enter the GEMMs -- what a
 *   16-bit convolution's backward would have received; grad_x is the float32 accumulator rounded once to DT at its single store; the weight gradients are the
 *   float32 accumulators, their partial sums added in a fixed order (no atomics: deterministic, every element written once).
 *   No loss scaling happens inside: fp16 underflow of small gradients is the caller's GradScaler, as for any 16-bit convolution.
 *   w_blur / blur_out (grad_blur) come together or are both null; grad_x, grad_w_guidance, grad_w_blur may each be null.  An unknown dtype, a 16-bit pointer
 *   that is not 2-byte aligned, a null required pointer or a bad shape (H > 2 h, W > 2 w): CSPN_E_BADARG.  B = 0: nothing to do, 0.
 * workspace: the matching *_g16_workspace_bytes(B, C, h, w) bytes, 256-byte aligned; too small or misaligned: CSPN_E_WORKSPACE. */
size_t cspn_guidance_head_g16_workspace_bytes(int B, int C, int h, int w);
int cspn_guidance_head_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, float* guidance_out, float* blur_out,
                           int B, int C, int h, int w, int H, int W,
                           void* workspace, size_t workspace_bytes, cspn_stream_t stream);
size_t cspn_guidance_head_backward_g16_workspace_bytes(int B, int C, int h, int w);
int cspn_guidance_head_backward_g16(const void* x, int dtype, const float* w_guidance, const float* w_blur, const float* grad_guidance,
                                    const float* grad_blur, void* grad_x, float* grad_w_guidance, float* grad_w_blur, int B, int C, int h, int w,
                                    int H, int W, void* workspace, size_t workspace_bytes, cspn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_AMD_H */
