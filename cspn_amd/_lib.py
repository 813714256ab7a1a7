"""ctypes binding of libcspn_amd.so (the C ABI in include/cspn_amd.h).

There is NO CPU fallback and no PyTorch re-implementation behind this module:
if the HIP library is missing or a call fails, it raises."""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CSPN_AMD_LIB") or os.path.join(_HERE, "libcspn_amd.so")
CSRC = os.path.join(_HERE, "csrc")

NORM_TYPES = {"8sum": 0, "8sum_abs": 1, "none": 2, "prenorm": 3}
ALGOS = {"auto": 0, "stepwise": 1, "fused": 2, "fused_cxx": 3, "fused_padded": 4}
ALGOS_3D = {"auto": 0, "stepwise": 1, "persistent": 2}
ABI_VERSION = 5
DTYPES = {"float16": 1, "bfloat16": 2}   # CSPN_DTYPE_F16 / CSPN_DTYPE_BF16: the gate storage types of the *_g16 entry points

HOOKS_PATH = os.path.join(os.path.dirname(LIB_PATH), "libcspn_amd_hooks.so")

_lib = None
_hooks = None


class CspnError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into cspn_amd/libcspn_amd.so (in-tree)."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    if not verbose:
        args.append("-s")
    subprocess.check_call(args)
    return LIB_PATH


c_int, c_size_t, vp = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p
_WS = [vp, c_size_t, vp]   # workspace, its bytes, stream: the tail of the entry points that take a workspace

# every entry point the binding calls: name -> (restype, argtypes).  First ABI 5 as it was released: load() binds these, so a library
# without one of them fails to load
_SYMBOLS = {
    "cspn2d_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn2d_auto_algo": (c_int, [c_int] * 4),
    "cspn2d_forward_f32": (c_int, [vp] * 4 + [c_int] * 5 + _WS),
    "cspn2d_forward_f32_algo": (c_int, [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_normalize_f32": (c_int, [vp] * 2 + [c_int] * 4 + [vp]),
    "cspn2d_forward_prenorm_f32": (c_int, [vp] * 4 + [c_int] * 4 + _WS),
    "cspn2d_backward_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn2d_backward_f32": (c_int, [vp] * 6 + [c_int] * 5 + _WS),
    "cspn2d_history_bytes": (c_size_t, [c_int] * 4),
    "cspn2d_forward_history_f32": (c_int, [vp] * 5 + [c_size_t] + [c_int] * 5 + _WS),
    "cspn2d_backward_history_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn2d_backward_history_f32": (c_int, [vp] * 5 + [c_size_t, vp, vp] + [c_int] * 5 + _WS),
    "cspn_metrics_workspace_bytes": (c_size_t, [c_size_t]),
    "cspn_metrics_f32": (c_int, [vp, vp, c_size_t, vp, vp, c_size_t, vp]),
    "cspn_l1_backward_f32": (c_int, [vp, vp, vp, vp, vp, c_size_t, vp]),
    "cspn3d_backward_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn3d_backward_f32": (c_int, [vp] * 5 + [c_int] * 6 + _WS),
    "cspn_unpool_f32": (c_int, [vp, vp, c_size_t, c_int, c_int, c_int, vp]),
    "cspn_guidance_head_workspace_bytes": (c_size_t, [c_int]),
    "cspn_guidance_head_f32": (c_int, [vp] * 5 + [c_int] * 7 + _WS),
    "cspn_guidance_head_backward_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn_guidance_head_backward_f32": (c_int, [vp] * 8 + [c_int] * 6 + _WS),
    "cspn_unpool_backward_f32": (c_int, [vp, vp, c_size_t, c_int, c_int, c_int, vp]),
    "cspn_sparse_sample_workspace_bytes": (c_size_t, [c_size_t]),
    "cspn_sparse_sample_f32": (c_int, [vp, vp, c_size_t, c_size_t, c_int, c_int, ctypes.c_ulonglong, vp, c_size_t, vp]),
    "cspn3d_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn3d_forward_f32": (c_int, [vp] * 4 + [c_int] * 6 + _WS),
    "cspn3d_workspace_bytes_ex": (c_size_t, [c_int] * 7),
    "cspn3d_forward_f32_algo": (c_int, [vp] * 4 + [c_int] * 7 + _WS),
    "cspn3d_multi_supported": (c_int, [c_int] * 6),
    "cspn3d_forward_multi_f32": (c_int, [vp] * 3 + [c_int] * 6 + _WS),
    "cspn3d_backward_multi_workspace_bytes": (c_size_t, [c_int] * 6),
    "cspn3d_backward_multi_f32": (c_int, [vp] * 5 + [c_int] * 6 + _WS),
    "cspn3d_check_status": (c_int, [vp]),
}
_BOUND_AT_LOAD = tuple(_SYMBOLS)
# exports added to ABI 5 after its release (purely additive, the version stayed): looked up on first use, so that a library built before
# them still loads and serves everything else, and a call of a missing one says to rebuild instead of raising AttributeError
_SYMBOLS.update({
    "cspn2d_normalize_backward_f32": (c_int, [vp] * 3 + [c_int] * 4 + [vp]),
    # C channels on shared 2D guidance
    "cspn2d_workspace_bytes_multi": (c_size_t, [c_int] * 5),
    "cspn2d_multi_supported": (c_int, [c_int] * 5),
    "cspn2d_forward_multi_f32": (c_int, [vp] * 4 + [c_int] * 8 + _WS),
    "cspn2d_history_bytes_multi": (c_size_t, [c_int] * 5),
    "cspn2d_forward_history_multi_f32": (c_int, [vp] * 5 + [c_size_t] + [c_int] * 7 + _WS),
    "cspn2d_backward_multi_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn2d_backward_multi_f32": (c_int, [vp] * 6 + [c_int] * 7 + _WS),
    "cspn2d_backward_history_multi_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn2d_backward_history_multi_f32": (c_int, [vp] * 5 + [c_size_t, vp, vp] + [c_int] * 7 + _WS),
    # the demo's gate normalisation (reference cspn_paddle/demo.py:24,34-36,47-49) and the 3D module on raw gates
    "cspn_gate_absnorm_f32": (c_int, [vp] * 2 + [c_int] * 2 + [c_size_t, vp]),
    "cspn_gate_absnorm_backward_f32": (c_int, [vp] * 3 + [c_int] * 2 + [c_size_t, vp]),
    "cspn3d_forward_absnorm_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn3d_forward_absnorm_f32": (c_int, [vp] * 3 + [c_int] * 6 + _WS),
    # the 2D NONE op over a K x K neighbourhood, K = 5 or 7 (fluid.layers.affinity_propagate's kernel_size)
    "cspn2d_kxk_workspace_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_kxk_history_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_forward_kxk_f32": (c_int, [vp] * 4 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_kxk_workspace_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_backward_kxk_f32": (c_int, [vp] * 3 + [c_size_t] + [vp] * 3 + [c_int] * 6 + _WS),
    # the depth-completion contract (Affinity_Propagate's normalisation, siting, blur term and pinning) over K x K, K = 3, 5 or 7
    "cspn2d_kxk_norm_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_kxk_norm_history_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_forward_kxk_norm_f32": (c_int, [vp] * 5 + [c_size_t] + [c_int] * 8 + _WS),
    "cspn2d_backward_kxk_norm_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_backward_kxk_norm_f32": (c_int, [vp] * 4 + [c_size_t] + [vp] * 3 + [c_int] * 8 + _WS),
    # the same four on fp16 / bf16 gates or guidance (gate_dtype DTYPES[...]); values, workspace and history stay float32
    "cspn2d_forward_kxk_g16": (c_int, [vp, c_int] + [vp] * 3 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_kxk_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_size_t] + [vp] * 3 + [c_int] * 6 + _WS),
    "cspn2d_forward_kxk_norm_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_size_t] + [c_int] * 8 + _WS),
    "cspn2d_backward_kxk_norm_g16": (c_int, [vp, c_int] + [vp] * 3 + [c_size_t] + [vp] * 3 + [c_int] * 8 + _WS),
    # assembling K x K levels per pixel (out = sum_j conf_j H_{s_j}): the kxk_norm arguments with conf, steps (host ints) and T behind sparse; the
    # backward also takes grad_conf behind grad_blur
    "cspn2d_kxk_assemble_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_kxk_assemble_history_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_backward_kxk_assemble_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_forward_kxk_assemble_f32": (c_int, [vp] * 5 + [c_int] + [vp] * 2 + [c_size_t] + [c_int] * 8 + _WS),
    "cspn2d_forward_kxk_assemble_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] + [vp] * 2 + [c_size_t] + [c_int] * 8 + _WS),
    "cspn2d_backward_kxk_assemble_f32": (c_int, [vp] * 5 + [c_int, vp, c_size_t] + [vp] * 4 + [c_int] * 8 + _WS),
    "cspn2d_backward_kxk_assemble_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int, vp, c_size_t] + [vp] * 4 + [c_int] * 8 + _WS),
    # dilated K x K propagation: the _g16 argument lists with dilation behind K (gate_dtype 0: float32 guidance); the byte queries above apply
    "cspn2d_forward_kxk_norm_dil": (c_int, [vp, c_int] + [vp] * 4 + [c_size_t] + [c_int] * 9 + _WS),
    "cspn2d_backward_kxk_norm_dil": (c_int, [vp, c_int] + [vp] * 3 + [c_size_t] + [vp] * 3 + [c_int] * 9 + _WS),
    "cspn2d_forward_kxk_assemble_dil": (c_int, [vp, c_int] + [vp] * 4 + [c_int] + [vp] * 2 + [c_size_t] + [c_int] * 9 + _WS),
    "cspn2d_backward_kxk_assemble_dil": (c_int, [vp, c_int] + [vp] * 4 + [c_int, vp, c_size_t] + [vp] * 4 + [c_int] * 9 + _WS),
    # K x K propagation pinned to the measured depth with a confidence: the _dil argument lists with pin_conf behind sparse and, in the backwards,
    # grad_sparse and grad_pin behind the other gradients; the byte queries above apply
    "cspn2d_forward_kxk_norm_pin": (c_int, [vp, c_int] + [vp] * 5 + [c_size_t] + [c_int] * 9 + _WS),
    "cspn2d_backward_kxk_norm_pin": (c_int, [vp, c_int] + [vp] * 4 + [c_size_t] + [vp] * 5 + [c_int] * 9 + _WS),
    "cspn2d_forward_kxk_assemble_pin": (c_int, [vp, c_int] + [vp] * 5 + [c_int] + [vp] * 2 + [c_size_t] + [c_int] * 9 + _WS),
    "cspn2d_backward_kxk_assemble_pin": (c_int, [vp, c_int] + [vp] * 5 + [c_int, vp, c_size_t] + [vp] * 6 + [c_int] * 9 + _WS),
    # non-local propagation with learned offsets (K = 3): aff, offset, x, sparse (or NULL) in front; the sampling operator on its own
    "cspn2d_nl_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_nl_history_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_forward_nl_f32": (c_int, [vp] * 6 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_nl_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_backward_nl_f32": (c_int, [vp] * 5 + [c_size_t] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_nl_sample_f32": (c_int, [vp] * 3 + [c_int] * 4 + [vp]),
    "cspn2d_nl_sample_backward_f32": (c_int, [vp] * 5 + [c_int] * 4 + [vp]),
    # their run-to-run bitwise twins (cspn2d_nl_det.hip): the same arguments; the sampling backward takes a workspace here
    "cspn2d_backward_nl_det_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_backward_nl_det_f32": (c_int, [vp] * 5 + [c_size_t] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_nl_sample_backward_det_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn2d_nl_sample_backward_det_f32": (c_int, [vp] * 5 + [c_int] * 4 + _WS),
    # the six on fp16 / bf16 affinities and offsets: a dtype code behind aff and behind offset, the twins' arguments otherwise
    "cspn2d_forward_nl_g16": (c_int, [vp, c_int, vp, c_int] + [vp] * 4 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_nl_g16": (c_int, [vp, c_int, vp, c_int] + [vp] * 3 + [c_size_t] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_backward_nl_det_g16": (c_int, [vp, c_int, vp, c_int] + [vp] * 3 + [c_size_t] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_nl_sample_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_int] * 4 + [vp]),
    "cspn2d_nl_sample_backward_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 4 + [vp]),
    "cspn2d_nl_sample_backward_det_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 4 + _WS),
    # the demo module's contract inside the K x K engine: the raw guide in the gates' place, argument lists as the four kxk entry points
    "cspn2d_forward_kxk_absnorm_f32": (c_int, [vp] * 4 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_forward_kxk_absnorm_g16": (c_int, [vp, c_int] + [vp] * 3 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_kxk_absnorm_workspace_bytes": (c_size_t, [c_int] * 6),
    "cspn2d_backward_kxk_absnorm_f32": (c_int, [vp] * 3 + [c_size_t] + [vp] * 3 + [c_int] * 6 + _WS),
    "cspn2d_backward_kxk_absnorm_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_size_t] + [vp] * 3 + [c_int] * 6 + _WS),
    # K x K propagation with per-step attention (K = 3, 5 or 7): guidance, att, x, sparse (or NULL) in front
    "cspn2d_kxk_dyn_workspace_bytes": (c_size_t, [c_int] * 8),
    "cspn2d_forward_kxk_dyn_f32": (c_int, [vp] * 6 + [c_size_t] + [c_int] * 6 + _WS),
    "cspn2d_backward_kxk_dyn_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_backward_kxk_dyn_f32": (c_int, [vp] * 5 + [c_size_t] + [vp] * 4 + [c_int] * 6 + _WS),
    # line-scan propagation, SPN's three-way recurrence (cspn2d_scan.hip): x, gates, lam (or NULL) in front; B, C, Cg, H, W, dirs (a 4-bit mask)
    "cspn2d_scan_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_forward_scan_f32": (c_int, [vp] * 4 + [c_int] * 6 + _WS),
    "cspn2d_backward_scan_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn2d_backward_scan_f32": (c_int, [vp] * 8 + [c_int] * 6 + _WS),
    # the guidance heads for K x K propagation (K*K-1 guidance planes + the blur plane), K = 3 (the 8-plane head), 5 or 7
    "cspn_guidance_head_kxk_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn_guidance_head_kxk_f32": (c_int, [vp] * 5 + [c_int] * 7 + _WS),
    "cspn_guidance_head_kxk_backward_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn_guidance_head_kxk_backward_f32": (c_int, [vp] * 8 + [c_int] * 7 + _WS),
    # the same heads on an fp16 / bf16 feature map (dtype DTYPES[...] after x), K = 5 or 7: 16-bit x, guidance, dL/dguidance, dL/dx; float32 weights, blur, dL/dW
    "cspn_guidance_head_kxk_g16_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn_guidance_head_kxk_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 7 + _WS),
    "cspn_guidance_head_kxk_backward_g16_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn_guidance_head_kxk_backward_g16": (c_int, [vp, c_int] + [vp] * 7 + [c_int] * 7 + _WS),
    # the 8-plane head + the blur head on an fp16 / bf16 feature map, feeding the float32 rings: 16-bit x and dL/dx; float32 guidance, blur, their gradients, dL/dW
    "cspn_guidance_head_g16_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn_guidance_head_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn_guidance_head_backward_g16_workspace_bytes": (c_size_t, [c_int] * 4),
    "cspn_guidance_head_backward_g16": (c_int, [vp, c_int] + [vp] * 7 + [c_int] * 6 + _WS),
    # the 3D entry points of the Paddle contract on fp16 / bf16 gates or guides (gate_dtype DTYPES[...] after the gate pointer): values, levels,
    # workspaces float32; the gate / guide gradient in the gate's type
    "cspn3d_forward_g16_algo": (c_int, [vp, c_int] + [vp] * 3 + [c_int] * 7 + _WS),
    "cspn3d_forward_multi_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_int] * 6 + _WS),
    "cspn3d_forward_absnorm_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_int] * 6 + _WS),
    "cspn3d_backward_g16_workspace_bytes": (c_size_t, [c_int] * 5),
    "cspn3d_backward_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn3d_backward_multi_g16_workspace_bytes": (c_size_t, [c_int] * 6),
    "cspn3d_backward_multi_g16": (c_int, [vp, c_int] + [vp] * 4 + [c_int] * 6 + _WS),
    "cspn_gate_absnorm_g16": (c_int, [vp, c_int, vp] + [c_int] * 2 + [c_size_t, vp]),
    "cspn_gate_absnorm_backward_g16": (c_int, [vp, c_int] + [vp] * 2 + [c_int] * 2 + [c_size_t, vp]),
    # the backward of the 3D normalising / masked modes (raw guidance, optional mask)
    "cspn3d_backward_norm_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn3d_backward_norm_f32": (c_int, [vp] * 6 + [c_int] * 7 + _WS),
    # the 3D normalising / masked modes on fp16 / bf16 guidance (gate_dtype after the guidance pointer): read where it is used, its gradient in
    # its type; everything else float32
    "cspn3d_forward_norm_g16": (c_int, [vp, c_int] + [vp] * 3 + [c_int] * 7 + _WS),
    "cspn3d_backward_norm_g16_workspace_bytes": (c_size_t, [c_int] * 7),
    "cspn3d_backward_norm_g16": (c_int, [vp, c_int] + [vp] * 5 + [c_int] * 7 + _WS),
    # the same modes for C value channels on shared guidance (feat / grad_out [B,C,D,H,W], sparse None or [B,1,D,H,W]); one backward workspace
    # query for both guidance types
    "cspn3d_forward_norm_multi_workspace_bytes": (c_size_t, [c_int] * 8),
    "cspn3d_forward_norm_multi_f32": (c_int, [vp] * 4 + [c_int] * 8 + _WS),
    "cspn3d_forward_norm_multi_g16": (c_int, [vp, c_int] + [vp] * 3 + [c_int] * 8 + _WS),
    "cspn3d_backward_norm_multi_workspace_bytes": (c_size_t, [c_int] * 8),
    "cspn3d_backward_norm_multi_f32": (c_int, [vp] * 6 + [c_int] * 8 + _WS),
    "cspn3d_backward_norm_multi_g16": (c_int, [vp, c_int] + [vp] * 5 + [c_int] * 8 + _WS),
})
_LATE_SYMBOLS = _SYMBOLS   # (the table's name while it held the later exports only)


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CspnError(
            "cspn_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C cspn_amd/csrc`). There is no fallback path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    lib.cspn_abi_version.restype = c_int
    v = lib.cspn_abi_version()
    if v != ABI_VERSION:   # (before any symbol lookup: a stale library must fail with this message, not an AttributeError)
        raise CspnError("cspn_amd: ABI version mismatch: library %d, binding %d -- rebuild with `make -C cspn_amd/csrc`" % (v, ABI_VERSION))
    lib.cspn_last_error.restype = ctypes.c_char_p
    for name in _BOUND_AT_LOAD:
        f = getattr(lib, name)
        f.restype, f.argtypes = _SYMBOLS[name]
    _lib = lib
    return lib


_bound = {}


def symbol(name):
    """the entry point `name` of the loaded library with its types set: what every wrapper calls"""
    f = _bound.get(name)
    if f is not None:
        return f
    lib = load()
    try:
        f = getattr(lib, name)
    except AttributeError:
        raise CspnError("cspn_amd: %s does not export %s (a library built before it was added) -- rebuild with `make -C cspn_amd/csrc`"
                        % (LIB_PATH, name)) from None
    f.restype, f.argtypes = _SYMBOLS[name]
    _bound[name] = f
    return f


late_symbol = symbol


def load_hooks():
    """libcspn_amd_hooks.so: what tests and measuring tools need beyond the ABI (plan dumps, plan A/B, the muted-workgroup launch
    of the persistent 3D kernel ...).  It links against libcspn_amd.so and calls the same code with the test's choice as an
    argument; the product library itself exports no cspn_debug_* symbol and keeps no test state."""
    global _hooks
    if _hooks is not None:
        return _hooks
    load()   # the product library first (the hooks library resolves its symbols against it)
    if not os.path.exists(HOOKS_PATH):
        raise CspnError("cspn_amd: %s not found -- `make -C cspn_amd/csrc` builds it next to the product library" % HOOKS_PATH)
    h = ctypes.CDLL(HOOKS_PATH)
    ip = ctypes.POINTER(c_int)
    h.cspn_debug_tsw_plan_geo.restype = c_int
    h.cspn_debug_tsw_plan_geo.argtypes = [c_int] * 5 + [ip]
    h.cspn_debug_tsw_plan_cuts.restype = c_int
    h.cspn_debug_tsw_plan_cuts.argtypes = [c_int] * 5 + [ip, ip, ip]
    h.cspn_debug_tsw_dump_plan.restype = c_int
    h.cspn_debug_tsw_dump_plan.argtypes = [c_int] * 5 + [vp, vp, vp]
    h.cspn_debug_forward2d_plan.restype = c_int
    h.cspn_debug_forward2d_plan.argtypes = [vp] * 4 + [c_int] * 6 + [vp, vp]
    h.cspn_debug_3d_geo.restype = c_int
    h.cspn_debug_3d_geo.argtypes = [c_int] * 5 + [ip]
    h.cspn_debug_3d_persistent_error.restype = c_int
    h.cspn_debug_3d_persistent_error.argtypes = [vp] + [c_int] * 4
    h.cspn_debug_3d_persistent_forward.restype = c_int
    h.cspn_debug_3d_persistent_forward.argtypes = [vp] * 3 + [c_int] * 7 + [vp, vp]
    h.cspn_debug_3d_backward_stepwise.restype = c_int
    h.cspn_debug_3d_backward_stepwise.argtypes = [vp] * 5 + [c_int] * 5 + [vp, vp]
    h.cspn_debug_sited8_supported.restype = c_int
    h.cspn_debug_sited8_supported.argtypes = [c_int] * 4
    h.cspn_debug_guidance_to_sited8.restype = c_int
    h.cspn_debug_guidance_to_sited8.argtypes = [vp, vp] + [c_int] * 4 + [vp]
    h.cspn_debug_forward_sited8.restype = c_int
    h.cspn_debug_forward_sited8.argtypes = [vp, vp, vp, vp] + [c_int] * 5 + [vp]
    _hooks = h
    return h


def check(rc, what):
    if rc != 0:
        msg = load().cspn_last_error().decode("utf-8", "replace")
        raise CspnError("%s failed (code %d): %s" % (what, rc, msg))
