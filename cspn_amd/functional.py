"""Functional front-end over the C ABI: tensors in, tensor out, work enqueued on
torch's current HIP stream.  PyTorch is plumbing here (device memory + streams);
all arithmetic happens in libcspn_amd.so."""
import collections
import ctypes

import torch

from . import _lib


def _prep(t, name, shape=None, dtype=torch.float32):
    """a tensor of the engine: on the GPU, of `dtype` (another than float32: the 16-bit dtype of the heads' x), of `shape` if given -> contiguous"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.CspnError(
            "cspn_amd: %s is on %s; the engine is GPU-only (hand-written HIP for gfx950) and has no CPU path"
            % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, "float32" if dtype == torch.float32 else "%s as x" % dtype, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t.contiguous()


_GATE16 = {torch.float16: _lib.DTYPES["float16"], torch.bfloat16: _lib.DTYPES["bfloat16"]}


def _prep_gate(t, name):
    """a gate / guidance tensor of the K x K engine or of the 3D Paddle contract: float32, or float16 / bfloat16 as it is (the *_g16 entry
    points widen it exactly where it is used) -> (tensor, gate_dtype code or None for float32)"""
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in _GATE16:
        return t.contiguous(), _GATE16[t.dtype]
    return _prep(t, name), None


def _prep_value(t, name, shape=None):
    """a value tensor of the K x K engine or of the 3D Paddle contract (one plane per channel): float32; float16 / bfloat16 is widened with
    one torch cast"""
    if isinstance(t, torch.Tensor) and t.dtype in _GATE16:
        t = t.float()
    return _prep(t, name, shape)


def widen16(*tensors):
    """float16 / bfloat16 tensors widened with a differentiable .float() (autograd carries the gradient back through the cast), everything
    else as it is: what the modules and mirrors do with value tensors, and in front of the paths that have no 16-bit kernel (3 x 3 in 2D: the
    ring; the gate_absnorm tensor op).  Every 3D path takes a 16-bit gate, guide or guidance as it is (cspn3d_*_g16): the Paddle contract, the
    demo module, and the normalising / masked modes (cspn3d_forward_norm, cspn3d_backward_norm, Affinity_Propagate3d)"""
    out = tuple(t.float() if isinstance(t, torch.Tensor) and t.dtype in _GATE16 else t for t in tensors)
    return out[0] if len(out) == 1 else out


def _workspace(nbytes, device):
    # torch's caching allocator: stream-ordered reuse is safe, base is >=512-B aligned
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _history(query, device, *args):
    """the history a forward writes its levels to, sized by the query `query`(*args) -> (a float32 tensor of at least one element, its bytes as
    the engine is told them)"""
    with torch.cuda.device(device):
        hb = _lib.symbol(query)(*args)
    return torch.empty(max(hb // 4, 1), dtype=torch.float32, device=device), hb


def _history_bytes(history):
    return history.numel() * history.element_size() if history is not None else 0


def _launch(name, device, args, ws_query=None, what=None):
    """One engine call on `device` and its current stream: name(*args, [workspace, its bytes,] stream), then _lib.check under `what` (default:
    name).  ws_query = (a size query's name, *its arguments): the workspace is allocated here and passed behind args.  -> the workspace"""
    ws = None
    with torch.cuda.device(device):
        if ws_query is not None:
            ws_bytes = _lib.symbol(ws_query[0])(*ws_query[1:])
            ws = _workspace(ws_bytes, device)
            args = (*args, ws.data_ptr(), ws_bytes)
        rc = _lib.symbol(name)(*args, torch.cuda.current_stream(device).cuda_stream)
    _lib.check(rc, what or name)
    return ws


def _normalize(guidance, norm_type):
    if guidance.dim() != 4 or guidance.shape[1] != 8:
        raise ValueError("guidance must be [B,8,H,W], got %s" % (tuple(guidance.shape),))
    g = _prep(guidance, "guidance")
    B, _, H, W = g.shape
    out = torch.empty_like(g)
    if B == 0:
        return out
    _launch("cspn2d_normalize_f32", g.device, (_ptr(g), _ptr(out), B, H, W, _lib.NORM_TYPES[norm_type]))
    return out


def cspn2d_normalize_backward(guidance, grad_wb, norm_type="8sum"):
    """The adjoint of cspn2d_normalize (cspn2d_normalize_backward_f32): guidance [B,8,H,W] (raw, as cspn2d_normalize takes it) and
    grad_wb = dL/dgate_wb [B,8,H,W] (consumer-sited: what cspn2d_backward(..., 'prenorm') returns for its guidance) -> dL/dguidance
    [B,8,H,W], the gradient torch autograd computes through the reference's affinity_normalization (cspn.py:85-144).  Elements no pixel
    reads get 0; NaN where a pixel's neighbourhood sums to 0 (as the forward)."""
    if norm_type not in ("8sum", "8sum_abs"):
        raise ValueError("norm_type must be '8sum' or '8sum_abs' (got %r)" % (norm_type,))
    if guidance.dim() != 4 or guidance.shape[1] != 8:
        raise ValueError("guidance must be [B,8,H,W], got %s" % (tuple(guidance.shape),))
    B, _, H, W = guidance.shape
    g = _prep(guidance, "guidance")
    r = _prep(grad_wb, "grad_wb", (B, 8, H, W))
    if r.device != g.device:
        raise ValueError("all tensors must live on the same device")
    out = torch.empty_like(g)
    if out.numel() == 0:
        return out
    _launch("cspn2d_normalize_backward_f32", g.device, (_ptr(g), _ptr(r), _ptr(out), B, H, W, _lib.NORM_TYPES[norm_type]))
    return out


class _NormalizeFunction(torch.autograd.Function):
    """cspn2d_normalize under autograd: keeps the raw guidance, the backward is one cspn2d_normalize_backward_f32 launch"""

    @staticmethod
    def forward(ctx, guidance, norm_type):
        ctx.norm_type = norm_type
        ctx.save_for_backward(guidance)
        return _normalize(guidance, norm_type)

    @staticmethod
    def backward(ctx, grad_wb):
        guidance, = ctx.saved_tensors
        return cspn2d_normalize_backward(guidance, grad_wb, ctx.norm_type), None


def cspn2d_normalize(guidance, norm_type="8sum"):
    """reference affinity_normalization (cspn_pytorch/models/cspn.py:85-144) as a stand-alone HIP kernel: guidance [B,8,H,W] ->
    gate_wb [B,8,H,W] (normalised, consumer-sited): what a producer head with a fused epilogue would emit, and what
    cspn2d_forward(..., norm_type="prenorm") takes in place of the raw guidance.  Differentiable w.r.t. guidance
    (cspn2d_normalize_backward) when grad mode is on and guidance requires grad; otherwise the plain forward kernel, no graph."""
    if torch.is_grad_enabled() and isinstance(guidance, torch.Tensor) and guidance.requires_grad:
        return _NormalizeFunction.apply(guidance, norm_type)
    return _normalize(guidance, norm_type)


def guidance_to_sited8(guidance, norm_type="8sum"):
    """(closed experiment, experiment builds only: libcspn_amd_hooks.so) [B,8,H,W] -> the pre-sited pair-interleaved layout
    [B,H,W/2,8,2] of DESIGN.md 3.6"""
    hooks = _lib.load_hooks()
    g = _prep(guidance, "guidance")
    B, _, H, W = g.shape
    out = torch.empty(B, H, W // 2, 8, 2, dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        rc = hooks.cspn_debug_guidance_to_sited8(g.data_ptr(), out.data_ptr(), B, H, W, _lib.NORM_TYPES[norm_type],
                                                 torch.cuda.current_stream(g.device).cuda_stream)
    if rc != 0:
        raise _lib.CspnError("cspn_debug_guidance_to_sited8 failed (code %d): the sited8 experiment is only in experiment builds "
                             "(make -C cspn_amd/csrc EXPERIMENTS=1)" % rc)
    return out


def cspn2d_forward_sited8(guidance_s8, blur_depth, sparse_depth=None, n_iter=24, norm_type="8sum"):
    """(closed experiment, experiment builds only) cspn2d_forward with the guidance in the sited8 layout (24 iterations, W >= 256)."""
    hooks = _lib.load_hooks()
    B, H, W2 = guidance_s8.shape[:3]
    W = 2 * W2
    g = _prep(guidance_s8, "guidance_s8", (B, H, W2, 8, 2))
    h = _prep(blur_depth, "blur_depth", (B, 1, H, W))
    s = _prep(sparse_depth, "sparse_depth", (B, 1, H, W)) if sparse_depth is not None else None
    out = torch.empty_like(h)
    with torch.cuda.device(g.device):
        rc = hooks.cspn_debug_forward_sited8(g.data_ptr(), h.data_ptr(), _ptr(s), out.data_ptr(),
                                             B, H, W, int(n_iter), _lib.NORM_TYPES[norm_type],
                                             torch.cuda.current_stream(g.device).cuda_stream)
    if rc != 0:
        raise _lib.CspnError("cspn_debug_forward_sited8 failed (code %d): experiment builds only, passes of exactly 24 iterations, "
                             "W >= 256, W %% 4 == 0" % rc)
    return out


# ---- the 3 x 3 engine in 2D: one body per operation; variant "" is one channel (cspn2d_*_f32, blur_depth [B,1,H,W]), "_multi" C >= 1 channels on shared
# guidance (cspn2d_*_multi_f32: reference cspn.py:58-81 broadcasts the affinities over blur_depth's channels) ----
def _args2d(variant, guidance, blur_depth, sparse_depth, extra=()):
    """-> (g, h, s, the shape arguments of the variant's size queries, those of its entry points, *extra): checked, contiguous, on one device"""
    if guidance.dim() != 4 or guidance.shape[1] != 8:
        raise ValueError("guidance must be [B,8,H,W], got %s" % (tuple(guidance.shape),))
    B, _, H, W = guidance.shape
    s, C, sc = None, 1, 1
    if not variant:
        g = _prep(guidance, "guidance")
        h = _prep(blur_depth, "blur_depth", (B, 1, H, W))
        if sparse_depth is not None:
            s = _prep(sparse_depth, "sparse_depth", (B, 1, H, W))
    else:
        if blur_depth.dim() != 4 or tuple(blur_depth.shape[:1]) + tuple(blur_depth.shape[2:]) != (B, H, W) or blur_depth.shape[1] < 1:
            raise ValueError("blur_depth has shape %s, expected (B,C,H,W) = (%d,C,%d,%d)" % (tuple(blur_depth.shape), B, H, W))
        C = blur_depth.shape[1]
        g = _prep(guidance, "guidance")
        h = _prep(blur_depth, "blur_depth", (B, C, H, W))
        if sparse_depth is not None:
            if sparse_depth.dim() != 4 or sparse_depth.shape[1] not in (1, C):
                raise ValueError("sparse_depth has shape %s, expected (B,1,H,W) or (B,C,H,W) = (%d,%d,%d,%d)"
                                 % (tuple(sparse_depth.shape), B, C, H, W))
            sc = sparse_depth.shape[1]
            s = _prep(sparse_depth, "sparse_depth", (B, sc, H, W))
    rest = [_prep(t, name, (B, C, H, W)) for t, name in extra]
    if any(t.device != g.device for t in [h] + ([s] if s is not None else []) + rest):
        raise ValueError("all tensors must live on the same device")
    return (g, h, s) + (((B, C, H, W), (B, C, sc, H, W)) if variant else ((B, H, W), (B, H, W))) + tuple(rest)


def _forward2d(variant, guidance, blur_depth, sparse_depth, n_iter, norm_type, algo):
    g, h, s, q, d = _args2d(variant, guidance, blur_depth, sparse_depth)
    out = torch.empty_like(h)
    if q[0] == 0:
        return out
    _launch("cspn2d_forward%s_f32%s" % (variant, "" if variant else "_algo"), g.device,
            (_ptr(g), _ptr(h), _ptr(s), _ptr(out), *d, int(n_iter), _lib.NORM_TYPES[norm_type], _lib.ALGOS[algo]),
            ("cspn2d_workspace_bytes" + variant, *q, int(n_iter)), "cspn2d_forward%s_f32" % variant)
    return out


def _forward2d_with_history(variant, guidance, blur_depth, sparse_depth, n_iter, norm_type):
    g, h, s, q, d = _args2d(variant, guidance, blur_depth, sparse_depth)
    out = torch.empty_like(h)
    with torch.cuda.device(g.device):
        hb = _lib.symbol("cspn2d_history_bytes" + variant)(*q, int(n_iter))
    if hb == 0:
        raise _lib.CspnError("cspn_amd: no history mode for B=%d C=%d H=%d W=%d, n_iter %d" % (*q, n_iter) if variant else
                             "cspn_amd: no history mode for shape %s, n_iter %d" % (tuple(guidance.shape), n_iter))
    hist = torch.empty(hb, dtype=torch.uint8, device=g.device)
    _launch("cspn2d_forward_history%s_f32" % variant, g.device,
            (_ptr(g), _ptr(h), _ptr(s), _ptr(out), _ptr(hist), hb, *d, int(n_iter), _lib.NORM_TYPES[norm_type]),
            ("cspn2d_workspace_bytes" + variant, *q, int(n_iter)))
    return out, hist


def _backward2d(variant, guidance, blur_depth, sparse_depth, grad_out, history, n_iter, norm_type, need_guidance, need_blur):
    """cspn2d_backward<variant>_f32 (history None: the levels are recomputed), or cspn2d_backward_history<variant>_f32 from what a training-mode
    forward kept"""
    g, h, s, q, d, go = _args2d(variant, guidance, blur_depth, sparse_depth, ((grad_out, "grad_out"),))
    gg = torch.empty_like(g) if need_guidance else None
    gh = torch.empty_like(h) if need_blur else None
    if (history is None and q[0] == 0) or not (need_guidance or need_blur):
        return gg, gh
    kind, hist = ("backward", ()) if history is None else ("backward_history", (history.data_ptr(), history.numel()))
    _launch("cspn2d_%s%s_f32" % (kind, variant), g.device,
            (_ptr(g), _ptr(h), _ptr(s), _ptr(go), *hist, _ptr(gg), _ptr(gh), *d, int(n_iter), _lib.NORM_TYPES[norm_type]),
            ("cspn2d_%s%s_workspace_bytes" % (kind, variant), *q, int(n_iter)))
    return gg, gh


def cspn2d_forward(guidance, blur_depth, sparse_depth=None, n_iter=24, norm_type="8sum", algo="auto"):
    """All n_iter steps of reference cspn_pytorch/models/cspn.py:42-83 in the HIP engine.

    guidance [B,8,H,W], blur_depth [B,1,H,W], sparse_depth [B,1,H,W] or None -> [B,1,H,W]."""
    return _forward2d("", guidance, blur_depth, sparse_depth, n_iter, norm_type, algo)


def cspn2d_backward(guidance, blur_depth, sparse_depth, grad_out, n_iter=24, norm_type="8sum",
                    need_guidance=True, need_blur=True):
    """Gradient of cspn2d_forward w.r.t. guidance and blur_depth (what autograd computes through reference
    cspn_pytorch/models/cspn.py:42-83, back-propagated by reference train.py:196-198) in the HIP engine.
    -> (grad_guidance [B,8,H,W] or None, grad_blur [B,1,H,W] or None)"""
    return _backward2d("", guidance, blur_depth, sparse_depth, grad_out, None, n_iter, norm_type, need_guidance, need_blur)


def cspn2d_history_bytes(B, H, W, n_iter):
    """bytes of what the training-mode forward keeps for its backward: every fourth level + the folded coefficients (0: not available for this shape)"""
    return int(_lib.symbol("cspn2d_history_bytes")(int(B), int(H), int(W), int(n_iter)))


def cspn2d_forward_with_history(guidance, blur_depth, sparse_depth=None, n_iter=24, norm_type="8sum"):
    """Training-mode forward: same output as cspn2d_forward, plus an opaque `history` tensor for cspn2d_backward_from_history:
    the checkpoints H_4, H_8 .. H_20 (every fourth level, register order per 4-column group) followed by the 8 folded coefficient
    planes -- 13 planes of B*H*W floats (the backward recomputes the levels in between; a tensor in the round-2 format, all 23
    levels, is NOT accepted: its size differs and the size is checked).  Only where cspn2d_history_bytes(...) > 0."""
    return _forward2d_with_history("", guidance, blur_depth, sparse_depth, n_iter, norm_type)


def cspn2d_backward_from_history(guidance, blur_depth, sparse_depth, grad_out, history, n_iter=24, norm_type="8sum",
                                 need_guidance=True, need_blur=True):
    """Gradients as cspn2d_backward, starting from the history a training-mode forward kept."""
    return _backward2d("", guidance, blur_depth, sparse_depth, grad_out, history, n_iter, norm_type, need_guidance, need_blur)


def cspn2d_multi_supported(B, C, H, W, n_iter):
    """True where C channels on shared guidance take the fast path (one ring launch per pass over the B*C image-channels)"""
    return bool(_lib.symbol("cspn2d_multi_supported")(int(B), int(C), int(H), int(W), int(n_iter)))


def cspn2d_forward_multi(guidance, blur_depth, sparse_depth=None, n_iter=24, norm_type="8sum", algo="auto"):
    """guidance [B,8,H,W], blur_depth [B,C,H,W], sparse_depth None, [B,1,H,W] (one mask for every channel) or [B,C,H,W] -> [B,C,H,W]:
    the C channels propagated on the same affinities (reference cspn.py:58-81), one engine call (cspn2d_forward_multi_f32)."""
    return _forward2d("_multi", guidance, blur_depth, sparse_depth, n_iter, norm_type, algo)


def cspn2d_backward_multi(guidance, blur_depth, sparse_depth, grad_out, n_iter=24, norm_type="8sum", need_guidance=True, need_blur=True):
    """Gradient of cspn2d_forward_multi: -> (grad_guidance [B,8,H,W] summed over the C channels or None, grad_blur [B,C,H,W] or None);
    one engine call (cspn2d_backward_multi_f32)."""
    return _backward2d("_multi", guidance, blur_depth, sparse_depth, grad_out, None, n_iter, norm_type, need_guidance, need_blur)


def cspn2d_history_bytes_multi(B, C, H, W, n_iter):
    """bytes of the training-mode history of C channels on shared guidance (0: not available for this shape)"""
    return int(_lib.symbol("cspn2d_history_bytes_multi")(int(B), int(C), int(H), int(W), int(n_iter)))


def cspn2d_forward_with_history_multi(guidance, blur_depth, sparse_depth=None, n_iter=24, norm_type="8sum"):
    """Training-mode cspn2d_forward_multi: (out [B,C,H,W], history) -- checkpoints and folded planes per image-channel."""
    return _forward2d_with_history("_multi", guidance, blur_depth, sparse_depth, n_iter, norm_type)


def cspn2d_backward_from_history_multi(guidance, blur_depth, sparse_depth, grad_out, history, n_iter=24, norm_type="8sum",
                                       need_guidance=True, need_blur=True):
    """Gradients as cspn2d_backward_multi, starting from the history cspn2d_forward_with_history_multi kept."""
    return _backward2d("_multi", guidance, blur_depth, sparse_depth, grad_out, history, n_iter, norm_type, need_guidance, need_blur)


def cspn3d_forward(gate, feat, sparse=None, n_iter=12, norm_type="8sum_abs", algo="auto", _return_ws=False):
    """gate [B,26,D,H,W], feat [B,1,D,H,W] -> [B,1,D,H,W]; n_iter 3x3x3 propagation steps.  algo: 'auto' | 'stepwise'
    (one launch per step) | 'persistent' (gates resident in registers across the steps; norm_type 'none' without a mask).
    With norm_type 'none' and no mask (the Paddle contract) gate may be float16 / bfloat16 (cspn3d_forward_g16_algo: widened exactly where
    it is read, out is float32 and bitwise the float32 call on gate.float() on the same path); a 16-bit feat is widened with one cast.  The
    normalising and masked modes take float32 gates only here: cspn3d_forward_norm takes them in 16 bits."""
    if gate.dim() != 5 or gate.shape[1] != 26:
        raise ValueError("gate must be [B,26,D,H,W], got %s" % (tuple(gate.shape),))
    B, _, D, H, W = gate.shape
    paddle = norm_type == "none" and sparse is None
    g, dt = _prep_gate(gate, "gate") if paddle else (_prep(gate, "gate"), None)
    h = _prep_value(feat, "feat", (B, 1, D, H, W)) if paddle else _prep(feat, "feat", (B, 1, D, H, W))
    s = _prep(sparse, "sparse", (B, 1, D, H, W)) if sparse is not None else None
    out, ws = _forward3d("cspn3d_forward_f32_algo" if dt is None else "cspn3d_forward_g16_algo", "cspn3d_forward_f32" if dt is None else "cspn3d_forward_g16",
                         g, dt, h, s, n_iter, norm_type, algo)
    return (out, ws) if _return_ws and B else out


def _forward3d(name, what, g, dt, h, s, n_iter, norm_type, algo):
    """one 3D forward call on prepared tensors (g of gate_dtype dt, None: float32) -> (out, the workspace)"""
    B, _, D, H, W = g.shape
    out = torch.empty_like(h)
    if B == 0:
        return out, None
    if g.data_ptr() % (16 if dt is None else 8) or any(t.data_ptr() % 16 for t in (h, out)):   # misaligned views take the folding path: the full workspace
        ws_query = ("cspn3d_workspace_bytes", B, D, H, W, int(n_iter))
    else:
        ws_query = ("cspn3d_workspace_bytes_ex", B, D, H, W, int(n_iter), _lib.NORM_TYPES[norm_type], int(s is not None))
    ws = _launch(name, g.device,
                 (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(s), _ptr(out), B, D, H, W, int(n_iter), _lib.NORM_TYPES[norm_type],
                  _lib.ALGOS_3D[algo]),
                 ws_query, what)
    return out, ws


def cspn3d_forward_norm(guidance, feat, sparse=None, n_iter=12, norm_type="8sum_abs", algo="auto"):
    """cspn3d_forward on a guidance that may be float16 / bfloat16 in EVERY mode ('8sum', '8sum_abs', 'none' with or without a mask): what a
    head under torch.autocast emits goes to the engine as it is (cspn3d_forward_norm_g16: each gate is widened exactly where the fold reads
    it, no float32 copy is made); out is float32 and bitwise cspn3d_forward(guidance.float(), ...) with the same algo.  feat and sparse are
    float32.  A float32 guidance is exactly cspn3d_forward.
    feat may be [B,C,D,H,W] with C > 1: the channels share the guidance and the mask (sparse None or [B,1,D,H,W]) -> [B,C,D,H,W], one engine
    call (cspn3d_forward_norm_multi_f32 / _g16: the fold runs once, w' and coef are read once per step for all channels, and stay resident
    across steps and channels where the persistent kernel takes the call).  Its channels are close to, not bitwise, the single-channel
    calls': the constant term is formed as coef H_0."""
    if guidance.dim() != 5 or guidance.shape[1] != 26:
        raise ValueError("guidance must be [B,26,D,H,W], got %s" % (tuple(guidance.shape),))
    B, _, D, H, W = guidance.shape
    g, dt = _prep_gate(guidance, "guidance")
    if isinstance(feat, torch.Tensor) and feat.dim() == 5 and feat.shape[1] > 1:
        C = feat.shape[1]
        h = _prep(feat, "feat", (B, C, D, H, W))
        s = _prep(sparse, "sparse", (B, 1, D, H, W)) if sparse is not None else None
        if any(t is not None and t.device != g.device for t in (h, s)):
            raise ValueError("all tensors must live on the same device")
        out = torch.empty_like(h)
        if B == 0:
            return out
        norm = _lib.NORM_TYPES[norm_type]
        _launch("cspn3d_forward_norm_multi_f32" if dt is None else "cspn3d_forward_norm_multi_g16", g.device,
                (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(s), _ptr(out), B, C, D, H, W, int(n_iter), norm, _lib.ALGOS_3D[algo]),
                ("cspn3d_forward_norm_multi_workspace_bytes", B, C, D, H, W, int(n_iter), norm, int(s is not None)))
        return out
    if dt is None:
        return cspn3d_forward(guidance, feat, sparse, n_iter, norm_type, algo)
    h = _prep(feat, "feat", (B, 1, D, H, W))
    s = _prep(sparse, "sparse", (B, 1, D, H, W)) if sparse is not None else None
    return _forward3d("cspn3d_forward_norm_g16", "cspn3d_forward_norm_g16", g, dt, h, s, n_iter, norm_type, algo)[0]


def cspn3d_forward_multi(gate, feat, n_iter=12):
    """gate [B,26,D,H,W] (used as given: the Paddle contract), feat [B,C,D,H,W] -> [B,C,D,H,W]: the C channels share the gates
    (reference cspn_paddle/README.md:56), which are read once per forward and stay in the registers while the n_iter steps run for
    one channel after the other.  Raises CspnError where the persistent kernel does not take the call (see cspn3d_multi_supported).
    gate may be float16 / bfloat16 (cspn3d_forward_multi_g16; out float32, bitwise the float32 call on gate.float())."""
    if gate.dim() != 5 or gate.shape[1] != 26:
        raise ValueError("gate must be [B,26,D,H,W], got %s" % (tuple(gate.shape),))
    B, _, D, H, W = gate.shape
    C = feat.shape[1]
    g, dt = _prep_gate(gate, "gate")
    h = _prep_value(feat, "feat", (B, C, D, H, W))
    if h.device != g.device:
        raise ValueError("all tensors must live on the same device")
    out = torch.empty_like(h)
    if B == 0:
        return out
    _launch("cspn3d_forward_multi_f32" if dt is None else "cspn3d_forward_multi_g16", g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(out), B, C, D, H, W, int(n_iter)),
            ("cspn3d_workspace_bytes_ex", B, D, H, W, int(n_iter), _lib.NORM_TYPES["none"], 0))
    return out


def cspn3d_check_status(device=None):
    """Synchronises the current stream of `device` and raises CspnError if a persistent 3D launch gave up on it (its outputs are
    NaN-filled): the failure the C ABI can only report after the call has returned.  Every later cspn3d_* call raises it too
    (once) without a synchronisation; call this where a result is about to be trusted without another 3D call in between."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    _launch("cspn3d_check_status", dev, ())


def _backward3d(variant, gate, feat, grad_out, n_iter, need_gate, need_feat):
    """cspn3d_backward<variant>_f32 / _g16: variant "" takes feat [B,1,D,H,W], "_multi" [B,C,D,H,W] on shared gates"""
    if gate.dim() != 5 or gate.shape[1] != 26:
        raise ValueError("gate must be [B,26,D,H,W], got %s" % (tuple(gate.shape),))
    B, _, D, H, W = gate.shape
    C = feat.shape[1] if variant else 1
    g, dt = _prep_gate(gate, "gate")
    h = _prep_value(feat, "feat", (B, C, D, H, W))
    go = _prep_value(grad_out, "grad_out", (B, C, D, H, W))
    if h.device != g.device or go.device != g.device:
        raise ValueError("all tensors must live on the same device")
    gg = torch.empty_like(g) if need_gate else None
    gf = torch.empty_like(h) if need_feat else None
    if B == 0 or not (need_gate or need_feat):
        return gg, gf
    dims = (B, C, D, H, W) if variant else (B, D, H, W)
    _launch("cspn3d_backward%s_%s" % (variant, "f32" if dt is None else "g16"), g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(go), _ptr(gg), _ptr(gf), *dims, int(n_iter),
             *(() if variant else (_lib.NORM_TYPES["none"],))),
            ("cspn3d_backward%s%s_workspace_bytes" % (variant, "" if dt is None else "_g16"), *dims, int(n_iter)))
    return gg, gf


def cspn3d_backward(gate, feat, grad_out, n_iter=1, need_gate=True, need_feat=True):
    """Gradient of cspn3d_forward(gate, feat, None, n_iter, 'none') -- the Paddle contract, the op the reference demo's
    optimiser differentiates (cspn_paddle/demo.py:65-75) -- w.r.t. gate and feat, in the HIP engine.
    -> (grad_gate [B,26,D,H,W] or None, grad_feat [B,1,D,H,W] or None).  A float16 / bfloat16 gate (cspn3d_backward_g16): grad_feat is
    float32 and bitwise the float32 call's on gate.float(), grad_gate comes back in the gate's dtype, the float32 sum rounded once."""
    return _backward3d("", gate, feat, grad_out, n_iter, need_gate, need_feat)


def cspn3d_backward_multi(gate, feat, grad_out, n_iter=1, need_gate=True, need_feat=True):
    """Gradient of the n_iter-step 3D propagation of C channels on SHARED gates (feat, grad_out [B,C,D,H,W]; reference
    cspn_paddle/README.md:56, differentiated at demo.py:65-75) -> (grad_gate [B,26,D,H,W] summed over the channels or None,
    grad_feat [B,C,D,H,W] or None); one call of the HIP engine (cspn3d_backward_multi_f32; cspn3d_backward_multi_g16 for a float16 /
    bfloat16 gate, whose gradient comes back in its dtype)."""
    return _backward3d("_multi", gate, feat, grad_out, n_iter, need_gate, need_feat)


def cspn3d_backward_norm(guidance, feat, sparse, grad_out, n_iter=12, norm_type="8sum_abs", algo="auto", need_guidance=True, need_feat=True):
    """Gradient of cspn3d_forward(guidance, feat, sparse, n_iter, norm_type) in its normalising / masked modes ('8sum', '8sum_abs', or
    'none' with a mask; 'none' without one is cspn3d_backward) w.r.t. the raw guidance and feat, in the HIP engine
    (cspn3d_backward_norm_f32: the fold is recomputed, one launch per step).  sparse gets no gradient (only its sign is used).
    -> (grad_guidance [B,26,D,H,W] or None, grad_feat [B,1,D,H,W] or None).  A float16 / bfloat16 guidance goes to the engine as it is
    (cspn3d_backward_norm_g16: read where it is used, no float32 copy of it or of its gradient): grad_feat is float32 and bitwise the float32
    call's on guidance.float(), grad_guidance comes back in the guidance's dtype, the float32 value rounded once.  The other tensors are float32.
    feat and grad_out may be [B,C,D,H,W] with C > 1 on the shared guidance and mask (sparse None or [B,1,D,H,W]; 'none' without a mask
    included): one engine call (cspn3d_backward_norm_multi_f32 / _g16), grad_feat [B,C,D,H,W], grad_guidance summed over the channels inside
    the engine -- written once per element, no atomics, bitwise reproducible."""
    if guidance.dim() != 5 or guidance.shape[1] != 26:
        raise ValueError("guidance must be [B,26,D,H,W], got %s" % (tuple(guidance.shape),))
    B, _, D, H, W = guidance.shape
    C = feat.shape[1] if isinstance(feat, torch.Tensor) and feat.dim() == 5 and feat.shape[1] > 1 else 1
    g, dt = _prep_gate(guidance, "guidance")
    h = _prep(feat, "feat", (B, C, D, H, W))
    s = _prep(sparse, "sparse", (B, 1, D, H, W)) if sparse is not None else None
    go = _prep(grad_out, "grad_out", (B, C, D, H, W))
    if any(t is not None and t.device != g.device for t in (h, s, go)):
        raise ValueError("all tensors must live on the same device")
    gg = torch.empty_like(g) if need_guidance else None
    gf = torch.empty_like(h) if need_feat else None
    if B == 0 or not (need_guidance or need_feat):
        return gg, gf
    norm = _lib.NORM_TYPES[norm_type]
    if C > 1:
        _launch("cspn3d_backward_norm_multi_f32" if dt is None else "cspn3d_backward_norm_multi_g16", g.device,
                (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(s), _ptr(go), _ptr(gg), _ptr(gf), B, C, D, H, W, int(n_iter), norm,
                 _lib.ALGOS_3D[algo]),
                ("cspn3d_backward_norm_multi_workspace_bytes", B, C, D, H, W, int(n_iter), norm, int(s is not None)))
        return gg, gf
    _launch("cspn3d_backward_norm_f32" if dt is None else "cspn3d_backward_norm_g16", g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(s), _ptr(go), _ptr(gg), _ptr(gf), B, D, H, W, int(n_iter), norm, _lib.ALGOS_3D[algo]),
            ("cspn3d_backward_norm%s_workspace_bytes" % ("" if dt is None else "_g16"), B, D, H, W, int(n_iter), norm, int(s is not None)))
    return gg, gf


class _AffinityPropagateFunction(torch.autograd.Function):
    """n_iter chained 3 x 3 (x 3) propagation steps of C >= 1 input channels on shared gates, differentiable w.r.t. both arguments: one engine call
    each way for all channels (the gate gradient summed in the engine), but for the 3D forward where the persistent kernel does not take them"""

    @staticmethod
    def forward(ctx, x, gate_weight, n_iter):
        ctx.n_iter = int(n_iter)
        ctx.save_for_backward(x, gate_weight)
        C = x.shape[1]
        if x.dim() == 4:
            return (cspn2d_forward if C == 1 else cspn2d_forward_multi)(gate_weight, x, None, n_iter, "none")
        if C == 1:
            return cspn3d_forward(gate_weight, x, None, n_iter, "none")
        if _lib.symbol("cspn3d_multi_supported")(x.shape[0], C, *x.shape[2:], int(n_iter)) and x.data_ptr() % 16 == 0 \
                and gate_weight.data_ptr() % (8 if gate_weight.dtype in _GATE16 else 16) == 0:
            return cspn3d_forward_multi(gate_weight, x, n_iter)
        return torch.cat([cspn3d_forward(gate_weight, x[:, c:c + 1].contiguous(), None, n_iter, "none") for c in range(C)], 1)

    @staticmethod
    def backward(ctx, grad_out):
        x, gate_weight = ctx.saved_tensors
        need_x, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if x.dim() == 4:
            gg, gx = (cspn2d_backward if x.shape[1] == 1 else cspn2d_backward_multi)(gate_weight, x, None, grad_out, ctx.n_iter, "none", need_g, need_x)
        else:
            gg, gx = (cspn3d_backward if x.shape[1] == 1 else cspn3d_backward_multi)(gate_weight, x, grad_out, ctx.n_iter, need_g, need_x)
        return gx, gg, None


# ---- the 2D NONE op over a K x K neighbourhood, K = 5 or 7 (cspn2d_kxk.hip): gate channel k is the k-th pair (t, l) in raster order over
# {0..K-1}^2 without the centre, neighbour offset (K//2 - t, K//2 - l) ----
def _kxk_shape(gate, x, kernel_size, extra=()):
    K = _check_kernel_size(kernel_size, x.dim() if isinstance(x, torch.Tensor) else 4)
    if K == 3:
        raise ValueError("the K x K engine takes kernel_size 5 or 7; 3 x 3 is cspn2d_forward / affinity_propagate")
    if gate.dim() != 4 or gate.shape[1] != K * K - 1:
        raise ValueError("gate must be [N,%d,H,W] for kernel_size %d, got %s" % (K * K - 1, K, tuple(gate.shape)))
    N, _, H, W = gate.shape
    if x.dim() != 4 or x.shape[0] != N or tuple(x.shape[2:]) != (H, W) or x.shape[1] < 1:
        raise ValueError("x has shape %s, expected (N,C,H,W) = (%d,C,%d,%d)" % (tuple(x.shape), N, H, W))
    C = x.shape[1]
    for t, name in extra:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, C, H, W):
            raise ValueError("%s must be a tensor of shape %s" % (name, (N, C, H, W)))
    return K, N, C, H, W


def _kxk_args(gate, x, kernel_size, extra=(), gate_name="gate"):
    K, N, C, H, W = _kxk_shape(gate, x, kernel_size, extra)
    g, dt = _prep_gate(gate, gate_name)
    h = _prep_value(x, "x")
    rest = [_prep_value(t, name, (N, C, H, W)) for t, name in extra]
    if any(t.device != g.device for t in [h] + rest):
        raise ValueError("all tensors must live on the same device")
    return (g, dt, h, K, N, C, H, W) + tuple(rest)


def _check_kernel_size(kernel_size, dim):
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, int):
        raise ValueError("kernel_size must be an int, got %r" % (kernel_size,))
    if kernel_size < 3 or kernel_size > 7 or kernel_size % 2 == 0:
        raise ValueError("kernel_size must be 3, 5 or 7 (odd, 3 <= K <= 7), got %d" % kernel_size)
    if kernel_size != 3 and dim != 4:
        raise ValueError("kernel_size %d is 2D only (input [N,C,H,W]); 3D takes the 3 x 3 x 3 neighbourhood" % kernel_size)
    return kernel_size


def cspn2d_forward_kxk(gate, x, kernel_size, n_iter, return_history=False):
    """gate [N,K*K-1,H,W] used as given (centre-sited, no centre term, any sign), x [N,C,H,W] -> H_n [N,C,H,W] with
    H_{t+1}(p) = sum_k gate_k(p) H_t(p + off_k), zero outside, the C channels on the shared gates (cspn2d_forward_kxk_f32).
    K = kernel_size in {5, 7}.  return_history: (out, history) with H_1 .. H_{n-1} for cspn2d_backward_kxk.  n_iter == 0 returns x.
    gate may be float16 / bfloat16 (cspn2d_forward_kxk_g16: widened exactly where used, out is float32 and bitwise the float32 call on
    gate.float()); a 16-bit x is widened with one cast."""
    return _kxk_forward(gate, x, kernel_size, n_iter, return_history, "")


def _kxk_forward(gate, x, kernel_size, n_iter, return_history, contract):
    """cspn2d_forward_kxk<contract>_f32 / _g16: contract "" (gates as given) or "_absnorm" (the raw guide in their place)"""
    _kxk_shape(gate, x, kernel_size)
    n = int(n_iter)
    if n < 0:
        raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
    if n == 0:
        return (x, None) if return_history else x
    g, dt, h, K, N, C, H, W = _kxk_args(gate, x, kernel_size, gate_name="guide" if contract else "gate")
    out = torch.empty_like(h)
    if out.numel() == 0:
        return (out, None) if return_history else out
    # with a history the levels go there: no workspace
    hist, hb = _history("cspn2d_kxk_history_bytes", g.device, N, C, H, W, K, n) if return_history else (None, 0)
    args = (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(out), _ptr(hist), hb, N, C, H, W, K, n)
    _launch("cspn2d_forward_kxk%s_%s" % (contract, "f32" if dt is None else "g16"), g.device, args + ((None, 0) if return_history else ()),
            None if return_history else ("cspn2d_kxk_workspace_bytes", N, C, H, W, K, n))
    return (out, hist) if return_history else out


def cspn2d_backward_kxk(gate, x, grad_out, kernel_size, n_iter, history=None, need_gate=True, need_x=True):
    """Gradient of cspn2d_forward_kxk -> (dL/dgate [N,K*K-1,H,W] summed over the C channels or None, dL/dx [N,C,H,W] or None);
    cspn2d_backward_kxk_f32.  history: what cspn2d_forward_kxk(..., return_history=True) returned; None runs that forward first
    where the gate gradient needs it.  A float16 / bfloat16 gate (cspn2d_backward_kxk_g16): dL/dx is float32 and bitwise the float32 call's,
    dL/dgate comes back in the gate's dtype, the float32 sum rounded once."""
    return _kxk_backward(gate, x, grad_out, kernel_size, n_iter, history, need_gate, need_x, "")


def _kxk_backward(gate, x, grad_out, kernel_size, n_iter, history, need_gate, need_x, contract):
    """cspn2d_backward_kxk<contract>_f32 / _g16, contract as _kxk_forward"""
    g, dt, h, K, N, C, H, W, go = _kxk_args(gate, x, kernel_size, ((grad_out, "grad_out"),), "guide" if contract else "gate")
    n = int(n_iter)
    if n < 0:
        raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
    gg = torch.empty_like(g) if need_gate else None
    gx = torch.empty_like(h) if need_x else None
    if not (need_gate or need_x):
        return gg, gx
    if h.numel() == 0:
        return (gg.zero_() if gg is not None else None), gx
    if need_gate and n >= 2 and history is None:
        _, history = _kxk_forward(g, h, K, n, True, contract)
    _launch("cspn2d_backward_kxk%s_%s" % (contract, "f32" if dt is None else "g16"), g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(history), _history_bytes(history), _ptr(go), _ptr(gg), _ptr(gx), N, C, H, W, K, n),
            ("cspn2d_backward_kxk%s_workspace_bytes" % contract, N, C, H, W, K, n))
    return gg, gx


def cspn2d_forward_kxk_absnorm(guide, x, kernel_size, n_iter, return_history=False):
    """The demo module's step inside the K x K engine (cspn2d_forward_kxk_absnorm_f32): guide [N,K*K-1,H,W] raw, any sign, in the gate
    channel order of cspn2d_forward_kxk; x [N,C,H,W], the C channels on the shared guide -> H_n [N,C,H,W] with
    H_{t+1}(p) = (sum_k |guide_k(p)| H_t(p + off_k)) / S(p), S(p) = sum_k |guide_k(p)|: what cspn2d_forward_kxk(gate_absnorm(guide, K*K-1),
    x, ...) computes up to rounding (the scale is applied once, after the sum), with no normalised gate stored.  NaN where a pixel's
    gates are all zero.  K = kernel_size in {5, 7}; return_history: (out, history) with H_1 .. H_{n-1} for cspn2d_backward_kxk_absnorm;
    n_iter == 0 returns x.  guide may be float16 / bfloat16 (cspn2d_forward_kxk_absnorm_g16: widened exactly where used, out is float32 and
    bitwise the float32 call on guide.float()); a 16-bit x is widened with one cast."""
    return _kxk_forward(guide, x, kernel_size, n_iter, return_history, "_absnorm")


def cspn2d_backward_kxk_absnorm(guide, x, grad_out, kernel_size, n_iter, history=None, need_guide=True, need_x=True):
    """Gradient of cspn2d_forward_kxk_absnorm -> (dL/dguide [N,K*K-1,H,W] summed over the C channels or None, dL/dx [N,C,H,W] or None);
    cspn2d_backward_kxk_absnorm_f32.  The adjoint steps read 1 / S from one float32 plane, the gate-gradient pass keeps its K*K-1 sums in
    registers and chains them through the normalisation as it writes: no dL/dw tensor exists.  history: what
    cspn2d_forward_kxk_absnorm(..., return_history=True) returned; None runs that forward first where the guide gradient needs it.
    A float16 / bfloat16 guide (cspn2d_backward_kxk_absnorm_g16): dL/dx is float32 and bitwise the float32 call's, dL/dguide comes back in
    the guide's dtype, the float32 value rounded once."""
    return _kxk_backward(guide, x, grad_out, kernel_size, n_iter, history, need_guide, need_x, "_absnorm")


# ---- K x K propagation with per-step attention, K = 3, 5 or 7 (cspn2d_kxk_dyn.hip) ----
def _dyn_args(guidance, att, x, sparse, kernel_size, n_iter, extra=()):
    """shapes and dtypes of the cspn2d_*_kxk_dyn calls -> (g, a, h, s, K, B, C, H, W, n) + the extra tensors, prepared.  float32 only: any other
    dtype is a TypeError"""
    K = _check_kernel_size(kernel_size, 4)
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or n_iter < 0:
        raise ValueError("n_iter must be an int >= 0 (got %r)" % (n_iter,))
    n, R = int(n_iter), K // 2
    named = [(guidance, "guidance"), (att, "att"), (x, "x")] + ([(sparse, "sparse")] if sparse is not None else []) + list(extra)
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32 (got %s): the per-step attention contract has no 16-bit kernels" % (name, t.dtype))
    if guidance.dim() != 4 or guidance.shape[1] != K * K - 1:
        raise ValueError("guidance must be [B,%d,H,W] for kernel_size %d, got %s" % (K * K - 1, K, tuple(guidance.shape)))
    B, _, H, W = guidance.shape
    if tuple(att.shape) != (B, n * (R + 1), H, W):
        raise ValueError("att must be [B,n_iter*(K//2+1),H,W] = %s, got %s" % ((B, n * (R + 1), H, W), tuple(att.shape)))
    if x.dim() != 4 or x.shape[0] != B or tuple(x.shape[2:]) != (H, W) or x.shape[1] < 1:
        raise ValueError("x has shape %s, expected (B,C,H,W) = (%d,C,%d,%d)" % (tuple(x.shape), B, H, W))
    C = x.shape[1]
    if sparse is not None and tuple(sparse.shape) != (B, 1, H, W):
        raise ValueError("sparse must be [B,1,H,W] = %s, got %s" % ((B, 1, H, W), tuple(sparse.shape)))
    for t, name in extra:
        if tuple(t.shape) != (B, C, H, W):
            raise ValueError("%s must be a tensor of shape %s" % (name, (B, C, H, W)))
    ts = [t if n == 0 and not extra else _prep(t, name) for t, name in named]   # (a forward of no step returns x, wherever it lives)
    if any(t.device != ts[0].device for t in ts):
        raise ValueError("all tensors must live on the same device")
    g, a, h = ts[:3]
    s = ts[3] if sparse is not None else None
    return (g, a, h, s, K, B, C, H, W, n) + tuple(ts[4 if sparse is not None else 3:])


def _dyn_history_query(K):
    """H~_1 .. H~_{n-1}: cspn2d_kxk_history_bytes, which knows K = 5 and 7; for K = 3 the same count from the query that does"""
    return "cspn2d_kxk_history_bytes" if K != 3 else "cspn2d_kxk_norm_history_bytes"


def cspn2d_forward_kxk_dyn(guidance, att, x, kernel_size, n_iter, sparse=None, return_history=False):
    """K x K propagation with per-step attention (cspn2d_forward_kxk_dyn_f32), K = kernel_size in {3, 5, 7}, R = K // 2: guidance [B,K*K-1,H,W] raw,
    any sign, read at the pixel, in the gate channel order of cspn2d_forward_kxk; att [B,n_iter*(R+1),H,W] used as given, channel t*(R+1) + r:
    r = 0 the pixel's own term of step t (it only enters the divisor), r >= 1 ring r = max(|dy|, |dx|) of step t; x [B,C,H,W], the C channels share
    guidance and att; sparse [B,1,H,W] or None, pinned where > 0 before every step (the result is not pinned):
        w^_k = att[t, ring(k)] * g_k      D = att[t, 0] + sum_k |w^_k|      w_k = w^_k / D      c = 1 - sum_k w_k
        H <- c * Ht + sum_k w_k * Ht(p + off_k),   Ht = sparse where sparse > 0 else H,   H_0 = x, n_iter times; zero outside the image
    No modulated or normalised gate is stored.  D = 0 gives the statement's non-finite pattern.  return_history: (out, history) with the pinned
    levels 1 .. n-1 for cspn2d_backward_kxk_dyn.  n_iter == 0 returns x.  float32 only: any other dtype is a TypeError.  Bitwise reproducible."""
    g, a, h, s, K, B, C, H, W, n = _dyn_args(guidance, att, x, sparse, kernel_size, n_iter)
    if n == 0:
        return (x, None) if return_history else x
    out = torch.empty_like(h)
    if out.numel() == 0:
        return (out, None) if return_history else out
    # with a history the levels go there; the workspace keeps the pinned H_0 alone
    hist, hb = _history(_dyn_history_query(K), g.device, B, C, H, W, K, n) if return_history else (None, 0)
    _launch("cspn2d_forward_kxk_dyn_f32", g.device, (_ptr(g), _ptr(a), _ptr(h), _ptr(s), _ptr(out), _ptr(hist), hb, B, C, H, W, K, n),
            ("cspn2d_kxk_dyn_workspace_bytes", B, C, H, W, K, n, int(s is not None), int(return_history)))
    return (out, hist) if return_history else out


def cspn2d_backward_kxk_dyn(guidance, att, x, grad_out, kernel_size, n_iter, sparse=None, history=None, need_guidance=True, need_att=True, need_x=True):
    """Gradient of cspn2d_forward_kxk_dyn -> (dL/dguidance [B,K*K-1,H,W] and dL/datt [B,n_iter*(R+1),H,W], each summed over the C channels, dL/dx
    [B,C,H,W]), None where not asked for; cspn2d_backward_kxk_dyn_f32.  sparse has no gradient.  The adjoint steps read att_r A / D from one staged
    tile per ring, the gradient pass keeps the raw gates and their K*K-1 sums in registers over all steps and writes every element once: no
    dL/dw tensor exists.  history: what cspn2d_forward_kxk_dyn(..., return_history=True) returned; None runs that forward first where dL/dguidance
    or dL/datt needs it (n_iter >= 2).  No atomics: run-to-run bitwise."""
    g, a, h, s, K, B, C, H, W, n, go = _dyn_args(guidance, att, x, sparse, kernel_size, n_iter, ((grad_out, "grad_out"),))
    gg = torch.empty_like(g) if need_guidance else None
    ga = torch.empty_like(a) if need_att else None
    gx = torch.empty_like(h) if need_x else None
    if not (need_guidance or need_att or need_x) or h.numel() == 0:
        return (gg.zero_() if gg is not None else None), ga, gx
    if (need_guidance or need_att) and n >= 2 and history is None:
        _, history = cspn2d_forward_kxk_dyn(g, a, h, K, n, s, return_history=True)
    _launch("cspn2d_backward_kxk_dyn_f32", g.device,
            (_ptr(g), _ptr(a), _ptr(h), _ptr(s), _ptr(history), _history_bytes(history), _ptr(go), _ptr(gg), _ptr(ga), _ptr(gx), B, C, H, W, K, n),
            ("cspn2d_backward_kxk_dyn_workspace_bytes", B, C, H, W, K, n, int(s is not None)))
    return gg, ga, gx


# ---- line-scan propagation, SPN's three-way recurrence (cspn2d_scan.hip) ----
def _scan_mask(dirs):
    """dirs: a non-empty collection of distinct direction codes 0 .. 3 -> (the 4-bit mask, D).  The engine numbers the directions in ascending
    order of their code, whatever the order they are given in"""
    try:
        codes = list(dirs)
    except TypeError:
        raise ValueError("dirs must be a non-empty tuple of distinct directions out of 0, 1, 2, 3 (got %r)" % (dirs,)) from None
    if not codes or len(set(codes)) != len(codes) or any(isinstance(d, bool) or not isinstance(d, int) or not 0 <= d <= 3 for d in codes):
        raise ValueError("dirs must be a non-empty tuple of distinct directions out of 0, 1, 2, 3 (got %r)" % (dirs,))
    return sum(1 << d for d in codes), len(codes)


def _scan_args(x, gates, dirs, lam, extra=()):
    """shapes and dtypes of the cspn2d_*_scan calls -> (x, gates, lam, mask, B, C, Cg, D, H, W) + the extra tensors ([B,D*C,H,W] each), prepared.
    float32 only: any other dtype is a TypeError"""
    mask, D = _scan_mask(dirs)
    named = [(x, "x"), (gates, "gates")] + ([(lam, "lam")] if lam is not None else []) + list(extra)
    for t, name in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32 (got %s): line-scan propagation has no 16-bit kernels" % (name, t.dtype))
    if x.dim() != 4 or x.shape[1] < 1:
        raise ValueError("x must be [B,C,H,W] with C >= 1, got %s" % (tuple(x.shape),))
    B, C, H, W = x.shape
    if gates.dim() != 4 or gates.shape[0] != B or tuple(gates.shape[2:]) != (H, W) or gates.shape[1] < 1 or gates.shape[1] % (3 * D):
        raise ValueError("gates must be [B,D*Cg*3,H,W] = (%d, %d*Cg*3, %d, %d), got %s" % (B, D, H, W, tuple(gates.shape)))
    Cg = gates.shape[1] // (3 * D)
    if C % Cg:
        raise ValueError("the %d gate groups (gates has %d = %d*Cg*3 channels) must divide the %d channels of x" % (Cg, gates.shape[1], D, C))
    for t, name in named[2:]:
        if tuple(t.shape) != (B, D * C, H, W):
            raise ValueError("%s must be [B,D*C,H,W] = %s, got %s" % (name, (B, D * C, H, W), tuple(t.shape)))
    ts = [_prep(t, name) for t, name in named]
    if any(t.device != ts[0].device for t in ts):
        raise ValueError("all tensors must live on the same device")
    n = 3 if lam is not None else 2
    return (ts[0], ts[1], ts[2] if lam is not None else None, mask, B, C, Cg, D, H, W) + tuple(ts[n:])


def cspn2d_forward_scan(x, gates, dirs=(0, 1, 2, 3), lam=None):
    """Line-scan propagation, the linear three-way recurrence of SPN (cspn2d_forward_scan_f32): x [B,C,H,W]; dirs a non-empty subset of
    {0: left->right, 1: right->left, 2: top->bottom, 3: bottom->top}, D its size, the directions numbered d = 0 .. D-1 in ascending order of their
    code; gates [B,D*Cg*3,H,W], channel (d*Cg + j)*3 + k, used as given (any sign, no normalisation), Cg divides C and channel c uses group
    j = c // (C // Cg); lam [B,D*C,H,W] or None -> out [B,D*C,H,W], channel d*C + c.  With t the coordinate along the scan, i along the line
    (directions 0 / 1: a line is a column, t the column index; 2 / 3: a line is a row), L the line length, t- the line visited just before t:
        g^_k(i,t) = g_k(i,t) if t is not the first line and 0 <= i + k - 1 < L, else 0
        b(i,t)    = lam(i,t) if lam is given, else 1 - sum_k g^_k(i,t)
        h(i,t)    = b(i,t) x(i,t) + sum_k g^_k(i,t) h(i + k - 1, t-)
    Written from the published description of the method, not from a source: compare it with your model.  One launch for all
    directions and steps.  A line has at most 2048 pixels.  float32 only: any other dtype is a TypeError.  Bitwise reproducible."""
    x, g, lm, mask, B, C, Cg, D, H, W = _scan_args(x, gates, dirs, lam)
    out = torch.empty((B, D * C, H, W), dtype=torch.float32, device=x.device)
    if out.numel() == 0:
        return out
    _launch("cspn2d_forward_scan_f32", x.device, (_ptr(x), _ptr(g), _ptr(lm), _ptr(out), B, C, Cg, H, W, mask),
            ("cspn2d_scan_workspace_bytes", B, C, Cg, H, W, mask, int(lm is not None)))
    return out


def cspn2d_backward_scan(x, gates, out, grad_out, dirs=(0, 1, 2, 3), lam=None, need_x=True, need_gates=True, need_lam=True):
    """Gradient of cspn2d_forward_scan -> (dL/dx [B,C,H,W] summed over the directions, dL/dgates [B,D*Cg*3,H,W] summed over a group's channels,
    dL/dlam [B,D*C,H,W]), None where not asked for or (dL/dlam) where lam is None; cspn2d_backward_scan_f32.  out: what the forward returned,
    the only history.  A(i,t) = grad_out(i,t) + sum_k g^_k(i - (k-1), t+) A(i - (k-1), t+); dL/dx = sum_d b A; dL/dlam = A x;
    dL/dg_k = sum_c A (h(i + k - 1, t-) - x) without lam, sum_c A h(i + k - 1, t-) with it, exactly 0 where the gate is dropped (first line,
    line ends).  One launch and at most one fixed-order reduction; no atomics: run-to-run bitwise."""
    x, g, lm, mask, B, C, Cg, D, H, W, o, go = _scan_args(x, gates, dirs, lam, ((out, "out"), (grad_out, "grad_out")))
    gx = torch.empty_like(x) if need_x else None
    gg = torch.empty_like(g) if need_gates else None
    gl = torch.empty_like(lm) if need_lam and lm is not None else None
    if (gx is None and gg is None and gl is None) or o.numel() == 0:
        return gx, gg, gl
    _launch("cspn2d_backward_scan_f32", x.device, (_ptr(x), _ptr(g), _ptr(lm), _ptr(o), _ptr(go), _ptr(gx), _ptr(gg), _ptr(gl), B, C, Cg, H, W, mask),
            ("cspn2d_backward_scan_workspace_bytes", B, C, Cg, H, W, mask, int(lm is not None)))
    return gx, gg, gl


class _AffinityPropagateKxKFunction(torch.autograd.Function):
    """2D K x K, any C on shared gates: the forward keeps H_1 .. H_{n-1}, the backward is one cspn2d_backward_kxk_f32 call"""

    @staticmethod
    def forward(ctx, x, gate_weight, kernel_size, n_iter):
        ctx.kernel_size, ctx.n_iter = kernel_size, n_iter
        out, hist = cspn2d_forward_kxk(gate_weight, x, kernel_size, n_iter, return_history=True)
        ctx.save_for_backward(x, gate_weight, hist)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gate_weight, hist = ctx.saved_tensors
        gg, gx = cspn2d_backward_kxk(gate_weight, x, grad_out, ctx.kernel_size, ctx.n_iter, hist, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        return gx, gg, None, None


def affinity_propagate(input, gate_weight, kernel_size=3, n_iter=1):
    """Mirror of fluid.layers.affinity_propagate (reference cspn_paddle/demo.py:41-43,50-52;
    contract cspn_paddle/README.md:54-56): input [N,C,...], gate_weight [N,kernel_size**d-1,...] already
    normalised over the channel dim by the caller, shared across the C input channels.
    d = 2 or 3; kernel_size 3, or 5 / 7 in 2D (the K x K engine, cspn2d_forward_kxk).  n_iter > 1 fuses that many chained calls
    (demo.py:39,50).  Differentiable w.r.t. input and gate_weight like the reference op (the demo trains through it, demo.py:65-75).
    float16 / bfloat16 (a head under torch.autocast): with kernel_size 5 / 7 the gates go to the engine as they are (widened exactly where
    used; the gate gradient comes back in their dtype) and a 16-bit input is widened with one cast; so it is with kernel_size 3 in 3D (the
    16-bit instances of the 3D kernels, cspn3d_*_g16); with kernel_size 3 in 2D (the ring: no 16-bit kernel) both are widened with a
    differentiable .float().  The result is float32 either way."""
    if kernel_size != 3:
        if not isinstance(input, torch.Tensor) or not isinstance(gate_weight, torch.Tensor):
            raise TypeError("input and gate_weight must be torch.Tensor")
        K = _check_kernel_size(kernel_size, input.dim())
        if gate_weight.dim() != 4 or gate_weight.shape[1] != K * K - 1:
            raise ValueError("gate_weight must have %d channels for kernel_size %d, got %s" % (K * K - 1, K, tuple(gate_weight.shape)))
        if int(n_iter) == 0:
            return input
        input = widen16(input)
        if torch.is_grad_enabled() and (input.requires_grad or gate_weight.requires_grad):
            return _AffinityPropagateKxKFunction.apply(input, gate_weight, K, int(n_iter))
        return cspn2d_forward_kxk(gate_weight, input, K, n_iter)
    input = widen16(input)
    d = input.dim() - 2
    if d not in (2, 3):
        raise ValueError("input must be [N,C,H,W] or [N,C,D,H,W]")
    if d == 2:
        gate_weight = widen16(gate_weight)
    if gate_weight.shape[1] != 3 ** d - 1:
        raise ValueError("gate_weight must have %d channels" % (3 ** d - 1))
    N, C = input.shape[:2]
    needs_grad = torch.is_grad_enabled() and (input.requires_grad or gate_weight.requires_grad)
    if input.device != gate_weight.device:
        raise ValueError("all tensors must live on the same device")
    if d == 3 and C > 1 and not needs_grad and input.is_cuda and _lib.symbol("cspn3d_multi_supported")(N, C, *input.shape[2:], int(n_iter)) \
            and input.is_contiguous() and gate_weight.is_contiguous() and input.data_ptr() % 16 == 0 \
            and gate_weight.data_ptr() % (8 if gate_weight.dtype in _GATE16 else 16) == 0:
        return cspn3d_forward_multi(gate_weight, input, n_iter)   # the gates are read once for all C channels
    if d == 3 and C > 1 and needs_grad and input.is_cuda:
        # training through C channels on shared gates (demo.py:65-75): one forward and one backward call for all of them
        return _AffinityPropagateFunction.apply(input.contiguous(), gate_weight.contiguous(), n_iter)
    if d == 2 and C > 1:
        # C channels on shared gates (README.md:56): one forward and one backward engine call for all of them
        if needs_grad:
            return _AffinityPropagateFunction.apply(input, gate_weight, n_iter)
        return cspn2d_forward_multi(gate_weight, input, None, n_iter, "none")
    outs = []
    for c in range(C):  # gates shared across channels (README.md:56)
        x = input[:, c:c + 1].contiguous()
        if torch.is_grad_enabled() and (x.requires_grad or gate_weight.requires_grad):
            outs.append(_AffinityPropagateFunction.apply(x, gate_weight, n_iter))
        elif d == 2:
            outs.append(cspn2d_forward(gate_weight, x, None, n_iter, "none"))
        else:
            outs.append(cspn3d_forward(gate_weight, x, None, n_iter, "none"))
    return outs[0] if C == 1 else torch.cat(outs, 1)


# ---- the depth-completion contract of Affinity_Propagate (reference cspn.py:42-144) over a K x K neighbourhood, K = 3, 5 or 7
# (cspn2d_*_kxk_norm_f32): guidance [B,K*K-1,H,W] raw in the K x K op's channel order, normalised, each gate sited at its neighbour, a
# (1 - gate_sum) blur term and sparse depth pinned ----
def _kxk_norm_shape(guidance, blur_depth, sparse_depth, kernel_size, norm_type, n_iter):
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, int) or kernel_size not in (3, 5, 7):
        raise ValueError("kernel_size must be 3, 5 or 7, got %r" % (kernel_size,))
    if norm_type not in ("8sum", "8sum_abs"):
        raise ValueError("norm_type must be '8sum' or '8sum_abs', got %r" % (norm_type,))
    if int(n_iter) < 0:
        raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
    for t, name in ((guidance, "guidance"), (blur_depth, "blur_depth")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    K = kernel_size
    if guidance.dim() != 4 or guidance.shape[1] != K * K - 1:
        raise ValueError("guidance must be [B,%d,H,W] for kernel_size %d, got %s" % (K * K - 1, K, tuple(guidance.shape)))
    B, _, H, W = guidance.shape
    if blur_depth.dim() != 4 or blur_depth.shape[0] != B or tuple(blur_depth.shape[2:]) != (H, W) or blur_depth.shape[1] < 1:
        raise ValueError("blur_depth has shape %s, expected (B,C,H,W) = (%d,C,%d,%d)" % (tuple(blur_depth.shape), B, H, W))
    C = blur_depth.shape[1]
    sc = 0
    if sparse_depth is not None:
        if not isinstance(sparse_depth, torch.Tensor) or sparse_depth.dim() != 4 or sparse_depth.shape[1] not in (1, C) \
                or sparse_depth.shape[0] != B or tuple(sparse_depth.shape[2:]) != (H, W):
            raise ValueError("sparse_depth must be None, (B,1,H,W) or (B,C,H,W) = (%d,%d,%d,%d), got %s"
                             % (B, C, H, W, tuple(getattr(sparse_depth, "shape", ()))))
        sc = sparse_depth.shape[1]
    return K, B, C, H, W, sc


KXK_DILATIONS = (1, 2)   # what the engine instantiates (cspn2d_kxk_impl.h: Dilations, and 1)


def check_dilation(dilation):
    if isinstance(dilation, bool) or not isinstance(dilation, int) or dilation not in KXK_DILATIONS:
        raise ValueError("dilation must be one of %r, got %r" % (KXK_DILATIONS, dilation))
    return dilation


def _kxk_entry(stem, dt, dilation):
    """the entry point of a folded / assembling call and what it takes around the tensors: (name, the dtype argument(s), the dilation
    argument(s)).  dilation 1 is the _f32 / _g16 entry point used before there was a dilation; any other the _dil one (gate_dtype 0: float32)"""
    check_dilation(dilation)
    if dilation == 1:
        return stem + ("_f32" if dt is None else "_g16"), (() if dt is None else (dt,)), ()
    return stem + "_dil", (0 if dt is None else dt,), (dilation,)


def _pin_entry(stem, dt, dilation):
    """the pinned entry point of a folded / assembling call: one for every guidance dtype (gate_dtype 0: float32) and every dilation"""
    check_dilation(dilation)
    return stem + "_pin", (0 if dt is None else dt,), (dilation,)


def _pin_check(sparse_depth, pin_conf):
    """sparse_depth and pin_conf: both given, the same shape, [B,1,H,W] or [B,C,H,W] (sparse_depth's shape itself is checked by _kxk_norm_shape)"""
    if sparse_depth is None or pin_conf is None:
        raise ValueError("the pinned contract needs a sparse_depth and a pin_conf (a pin_conf without a sparse_depth pins nothing)")
    if not isinstance(pin_conf, torch.Tensor) or not isinstance(sparse_depth, torch.Tensor) or tuple(pin_conf.shape) != tuple(sparse_depth.shape):
        raise ValueError("pin_conf must be a tensor of sparse_depth's shape %s ([B,1,H,W] or [B,C,H,W]), got %s"
                         % (tuple(getattr(sparse_depth, "shape", ())), tuple(getattr(pin_conf, "shape", ()))))


def _assemble_steps(steps, n_iter):
    """steps: ints, strictly increasing, steps[0] >= 0, steps[-1] == n_iter >= 1 -> the ctypes array the engine reads"""
    try:
        st = tuple(steps)
    except TypeError:
        raise ValueError("steps must be a sequence of ints, got %r" % (steps,)) from None
    if not st or any(isinstance(s, bool) or not isinstance(s, int) for s in st):
        raise ValueError("steps must be a non-empty sequence of ints, got %r" % (steps,))
    n = int(n_iter)
    if n < 1:
        raise ValueError("n_iter must be >= 1 for the assembling call (got %r)" % (n_iter,))
    if st[0] < 0 or any(b <= a for a, b in zip(st, st[1:])) or st[-1] != n:
        raise ValueError("steps must be strictly increasing, start at >= 0 and end at n_iter = %d, got %r" % (n, st))
    return (ctypes.c_int * len(st))(*st)


# The one host path of the eight public calls below: the folded contract (cspn2d_*_kxk_norm) and the assembling one (cspn2d_*_kxk_assemble), each
# with and without a pin.  A call is described by three things: `pinned` (pin_conf exists; None is then an error, not the unpinned call), `assemble`
# (None, or the pair (conf, steps)) and the dilation.  What they decide, and nothing else differs between the eight:
#   * the names: cspn2d_{forward,backward}_kxk_<kind> through _kxk_entry (unpinned: _f32 / _g16 / _dil) or _pin_entry, and the size queries
#     cspn2d_kxk_<kind>_{history,workspace}_bytes and cspn2d_backward_kxk_<kind>_workspace_bytes, <kind> = norm or assemble (_FOLD_NAMES);
#   * the engine's arguments (include/cspn_amd.h): pin_conf directly behind sparse, then conf, steps, T; in the backward grad_conf, then
#     grad_sparse and grad_pin, behind grad_blur;
#   * n_iter == 0: the folded forward returns blur_depth itself, wherever it lives; the assembling calls refuse it (_assemble_steps);
#   * a backward without a history runs the forward first where dL/dguidance or dL/dpin_conf (n_iter >= 2: both read the gradient of the folded
#     gates) or dL/dconf (always: it reads the collected levels) is asked for.
_FoldNames = collections.namedtuple("_FoldNames", "forward backward history_bytes forward_workspace_bytes backward_workspace_bytes")
_FOLD_NAMES = {   # by `assemble is not None`: the stems of the entry points (_kxk_entry / _pin_entry add the suffix) and the size queries
    False: _FoldNames("cspn2d_forward_kxk_norm", "cspn2d_backward_kxk_norm", "cspn2d_kxk_norm_history_bytes",
                      "cspn2d_kxk_norm_workspace_bytes", "cspn2d_backward_kxk_norm_workspace_bytes"),
    True: _FoldNames("cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble", "cspn2d_kxk_assemble_history_bytes",
                     "cspn2d_kxk_assemble_workspace_bytes", "cspn2d_backward_kxk_assemble_workspace_bytes"),
}


def _fold_checks(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, dilation):
    """what every one of the eight calls checks first, in one order: kernel_size, norm_type, n_iter and the shapes; the pin; conf and steps; the
    dilation (a backward goes on with grad_out; the device comes last, in _fold_tensors) -> K, B, C, H, W, sparse_depth's planes, the steps as the
    engine reads them (None: the folded contract)"""
    K, B, C, H, W, sc = _kxk_norm_shape(guidance, blur_depth, sparse_depth, kernel_size, norm_type, n_iter)
    if pinned:
        _pin_check(sparse_depth, pin_conf)
    c_steps = None
    if assemble is not None:
        conf, steps = assemble
        c_steps = _assemble_steps(steps, n_iter)
        if not isinstance(conf, torch.Tensor):
            raise TypeError("conf must be a torch.Tensor")
        if tuple(conf.shape) != (B, len(c_steps), H, W):
            raise ValueError("conf has shape %s, expected (B,len(steps),H,W) = %s" % (tuple(conf.shape), (B, len(c_steps), H, W)))
    check_dilation(dilation)
    return K, B, C, H, W, sc, c_steps


def _fold_tensors(guidance, blur_depth, *others):
    """one device for all, then every tensor as the engine takes it: the guidance in its dtype, the values float32 (a 16-bit one widened with one
    cast) -> guidance, its dtype code, blur_depth, *others (None stays None)"""
    if any(isinstance(t, torch.Tensor) and t.device != guidance.device for t in (blur_depth,) + tuple(t for t, _ in others)):
        raise ValueError("all tensors must live on the same device")
    g, dt = _prep_gate(guidance, "guidance")
    return (g, dt, _prep_value(blur_depth, "blur_depth")) + tuple(None if t is None else _prep_value(t, name) for t, name in others)


def _fold_forward(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, return_history, dilation):
    """cspn2d_forward_kxk_{norm,assemble}[_pin] -> out, or (out, history) with return_history"""
    K, B, C, H, W, sc, c_steps = _fold_checks(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, dilation)
    n = int(n_iter)
    if n == 0:   # (the folded contract alone gets here)
        return (blur_depth, None) if return_history else blur_depth
    g, dt, h, s, p, cf = _fold_tensors(guidance, blur_depth, (sparse_depth, "sparse_depth"), (pin_conf if pinned else None, "pin_conf"),
                                       (assemble[0] if assemble else None, "conf"))
    out = torch.empty_like(h)
    if out.numel() == 0:
        return (out, None) if return_history else out
    names = _FOLD_NAMES[assemble is not None]
    # with a history the levels go there and the workspace holds only the fold (the query's n_iter = 1 size)
    hist, hb = _history(names.history_bytes, g.device, B, C, H, W, K, n) if return_history else (None, 0)
    name, dta, dil = (_pin_entry if pinned else _kxk_entry)(names.forward, dt, dilation)
    _launch(name, g.device,
            (_ptr(g), *dta, _ptr(h), _ptr(s), *((_ptr(p),) if pinned else ()), *((_ptr(cf), c_steps, len(c_steps)) if assemble else ()),
             _ptr(out), _ptr(hist), hb, B, C, sc, H, W, K, *dil, n, _lib.NORM_TYPES[norm_type]),
            (names.forward_workspace_bytes, B, C, sc, H, W, K, 1 if return_history else n))
    return (out, hist) if return_history else out


def _fold_backward(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, grad_out, kernel_size, n_iter, norm_type, history, dilation,
                   need_guidance, need_blur, need_conf=False, need_sparse=False, need_pin=False):
    """cspn2d_backward_kxk_{norm,assemble}[_pin] -> (dL/dguidance, dL/dblur_depth, dL/dconf, dL/dsparse_depth, dL/dpin_conf), None for what the
    contract does not have or the caller does not need"""
    K, B, C, H, W, sc, c_steps = _fold_checks(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, dilation)
    if not isinstance(grad_out, torch.Tensor) or tuple(grad_out.shape) != tuple(blur_depth.shape):
        raise ValueError("grad_out must be a tensor of shape %s" % (tuple(blur_depth.shape),))
    g, dt, h, s, p, cf, go = _fold_tensors(guidance, blur_depth, (sparse_depth, "sparse_depth"), (pin_conf if pinned else None, "pin_conf"),
                                           (assemble[0] if assemble else None, "conf"), (grad_out, "grad_out"))
    n = int(n_iter)
    need = (need_guidance, need_blur, need_conf and assemble is not None, need_sparse and pinned, need_pin and pinned)
    grads = [torch.empty_like(t) if wanted else None for t, wanted in zip((g, h, cf, s, p), need)]
    if not any(need):
        return tuple(grads)
    if h.numel() == 0:
        if grads[0] is not None:
            grads[0].zero_()
        return tuple(grads)
    if history is None and (((need[0] or need[4]) and n >= 2) or need[2]):
        _, history = _fold_forward(g, h, s, p, pinned, (cf, assemble[1]) if assemble else None, K, n, norm_type, True, dilation)
    names = _FOLD_NAMES[assemble is not None]
    name, dta, dil = (_pin_entry if pinned else _kxk_entry)(names.backward, dt, dilation)
    gg, gh, gc, gs, gp = (_ptr(t) for t in grads)
    _launch(name, g.device,
            (_ptr(g), *dta, _ptr(h), _ptr(s), *((_ptr(p),) if pinned else ()), *((_ptr(cf), c_steps, len(c_steps)) if assemble else ()),
             _ptr(history), _history_bytes(history), _ptr(go), gg, gh, *((gc,) if assemble else ()), *((gs, gp) if pinned else ()),
             B, C, sc, H, W, K, *dil, n, _lib.NORM_TYPES[norm_type]),
            (names.backward_workspace_bytes, B, C, sc, H, W, K, n))
    return tuple(grads)


def cspn2d_forward_kxk_norm(guidance, blur_depth, sparse_depth=None, kernel_size=5, n_iter=24, norm_type="8sum", return_history=False, dilation=1):
    """Affinity_Propagate's forward (reference cspn.py:42-144) over a kernel_size x kernel_size neighbourhood: guidance [B,K*K-1,H,W] raw
    (channel k = the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre, its gate sited at the neighbour
    (K//2 - t, K//2 - l)), blur_depth [B,C,H,W] on the shared guidance, sparse_depth None, [B,1,H,W] or [B,C,H,W] -> [B,C,H,W]
    (cspn2d_forward_kxk_norm_f32).  return_history: (out, history) with H_1 .. H_{n-1} for cspn2d_backward_kxk_norm.  n_iter == 0
    returns blur_depth itself.  guidance may be float16 / bfloat16 (cspn2d_forward_kxk_norm_g16, K = 3 included: the fold widens it exactly,
    w' stays float32; out is float32 and bitwise the float32 call on guidance.float()); 16-bit blur_depth / sparse_depth are widened with
    one cast.  dilation 1 or 2: the neighbour of gate (t, l) is dilation * (K//2 - t, K//2 - l) (dilated CSPN++; cspn2d_forward_kxk_norm_dil)."""
    return _fold_forward(guidance, blur_depth, sparse_depth, None, False, None, kernel_size, n_iter, norm_type, return_history, dilation)


def cspn2d_backward_kxk_norm(guidance, blur_depth, sparse_depth, grad_out, kernel_size=5, n_iter=24, norm_type="8sum", history=None,
                             need_guidance=True, need_blur=True, dilation=1):
    """Gradient of cspn2d_forward_kxk_norm -> (dL/dguidance [B,K*K-1,H,W] summed over the C channels or None, dL/dblur_depth [B,C,H,W]
    or None); sparse_depth gets none (cspn.py uses its sign only).  cspn2d_backward_kxk_norm_f32.  history: what
    cspn2d_forward_kxk_norm(..., return_history=True) returned; None runs that forward first where the guidance gradient needs it.
    A float16 / bfloat16 guidance (cspn2d_backward_kxk_norm_g16): dL/dblur_depth is float32 and bitwise the float32 call's, dL/dguidance comes
    back in the guidance's dtype, the float32 value rounded once.  dilation: that of the forward (cspn2d_backward_kxk_norm_dil)."""
    return _fold_backward(guidance, blur_depth, sparse_depth, None, False, None, grad_out, kernel_size, n_iter, norm_type, history, dilation,
                          need_guidance, need_blur)[:2]


# ---- assembling K x K levels per pixel (CSPN++): out = sum_j conf_j H_{s_j} over the levels H_t of cspn2d_forward_kxk_norm, H_0 = blur_depth
# (cspn2d_*_kxk_assemble_f32 / _g16) ----
def cspn2d_forward_kxk_assemble(guidance, blur_depth, sparse_depth, conf, steps, kernel_size=5, n_iter=24, norm_type="8sum", return_history=False,
                                dilation=1):
    """out [B,C,H,W] = sum_j conf[:, j] * H_{steps[j]}: the levels H_t of cspn2d_forward_kxk_norm (H_0 = blur_depth) assembled per pixel
    inside the engine, one call (cspn2d_forward_kxk_assemble_f32).  conf [B,len(steps),H,W], shared by the C channels and used as given
    (no softmax); steps strictly increasing ints, steps[0] >= 0, steps[-1] == n_iter >= 1.  return_history: (out, history) with the n levels
    H_1 .. H_n for cspn2d_backward_kxk_assemble.  guidance may be float16 / bfloat16 and is taken as it is (out is float32 and bitwise the
    float32 call on guidance.float()); a 16-bit conf, blur_depth or sparse_depth is widened with one cast.  dilation 1 or 2: the levels are
    those of cspn2d_forward_kxk_norm at that dilation (cspn2d_forward_kxk_assemble_dil)."""
    return _fold_forward(guidance, blur_depth, sparse_depth, None, False, (conf, steps), kernel_size, n_iter, norm_type, return_history, dilation)


def cspn2d_backward_kxk_assemble(guidance, blur_depth, sparse_depth, conf, steps, grad_out, kernel_size=5, n_iter=24, norm_type="8sum", history=None,
                                 need_guidance=True, need_blur=True, need_conf=True, dilation=1):
    """Gradient of cspn2d_forward_kxk_assemble -> (dL/dguidance [B,K*K-1,H,W] in the guidance's dtype, rounded once, dL/dblur_depth [B,C,H,W],
    dL/dconf [B,len(steps),H,W]), None where not asked for; one engine call (cspn2d_backward_kxk_assemble_f32): the adjoint sweep of
    cspn2d_backward_kxk_norm with conf_j grad_out injected at every collected level, and dL/dconf_j = sum_c grad_out H_{steps[j]}.  history: what
    cspn2d_forward_kxk_assemble(..., return_history=True) returned; None runs that forward first where dL/dguidance or dL/dconf needs it.
    dilation: that of the forward (cspn2d_backward_kxk_assemble_dil)."""
    return _fold_backward(guidance, blur_depth, sparse_depth, None, False, (conf, steps), grad_out, kernel_size, n_iter, norm_type, history, dilation,
                          need_guidance, need_blur, need_conf)[:3]


# ---- the two contracts above pinned to the measured depth with a per-pixel confidence (CSPN++ / PENet; cspn2d_*_kxk_{norm,assemble}_pin): after
# every step H = (1 - m) step(H) + m sparse_depth with m = sign(sparse_depth) * pin_conf.  Functions of their own: the four above keep their
# parameter lists ----
def cspn2d_forward_kxk_norm_pin(guidance, blur_depth, sparse_depth=None, pin_conf=None, kernel_size=5, n_iter=24, norm_type="8sum", return_history=False,
                                dilation=1):
    """cspn2d_forward_kxk_norm pinned to the measured depth with a per-pixel confidence: after every step
        H <- (1 - m) * step(H) + m * sparse_depth,      m = sign(sparse_depth) * pin_conf,      H_0 = blur_depth,
    one engine call (cspn2d_forward_kxk_norm_pin).  sparse_depth enters by its value as well as its sign; pin_conf has sparse_depth's shape
    ([B,1,H,W]: one mask for the C channels, or [B,C,H,W]) and is used as given (no sigmoid, no clamp).  With pin_conf = 1, sparse_depth >= 0
    and blur_depth = sparse_depth where it is measured the result is bitwise cspn2d_forward_kxk_norm's; with pin_conf = 0 bitwise that of the
    call without a mask.  Everything else (guidance dtypes, return_history, n_iter == 0 returns blur_depth itself, dilation) as there; a 16-bit
    sparse_depth or pin_conf is widened with one cast."""
    return _fold_forward(guidance, blur_depth, sparse_depth, pin_conf, True, None, kernel_size, n_iter, norm_type, return_history, dilation)


def cspn2d_backward_kxk_norm_pin(guidance, blur_depth, sparse_depth, pin_conf, grad_out, kernel_size=5, n_iter=24, norm_type="8sum", history=None,
                                 need_guidance=True, need_blur=True, need_sparse=True, need_pin=True, dilation=1):
    """Gradient of cspn2d_forward_kxk_norm_pin -> (dL/dguidance in the guidance's dtype, dL/dblur_depth, dL/dsparse_depth, dL/dpin_conf), None
    where not asked for; one engine call (cspn2d_backward_kxk_norm_pin).  dL/dsparse_depth goes through the value (the sign has no
    derivative); dL/dpin_conf is exactly 0 where sparse_depth == 0.  Both are float32 with sparse_depth's shape.  history: what
    cspn2d_forward_kxk_norm_pin(..., return_history=True) returned; None runs that forward first where dL/dguidance or dL/dpin_conf needs it
    (n_iter >= 2: both read the gradient of the folded gates)."""
    gg, gh, _, gs, gp = _fold_backward(guidance, blur_depth, sparse_depth, pin_conf, True, None, grad_out, kernel_size, n_iter, norm_type, history, dilation,
                                       need_guidance, need_blur, False, need_sparse, need_pin)
    return gg, gh, gs, gp


def cspn2d_forward_kxk_assemble_pin(guidance, blur_depth, sparse_depth, pin_conf, conf, steps, kernel_size=5, n_iter=24, norm_type="8sum",
                                    return_history=False, dilation=1):
    """cspn2d_forward_kxk_assemble over the levels of cspn2d_forward_kxk_norm_pin: out = sum_j conf[:, j] * H_{steps[j]}, one engine call
    (cspn2d_forward_kxk_assemble_pin).  pin_conf as there; everything else as the unpinned call."""
    return _fold_forward(guidance, blur_depth, sparse_depth, pin_conf, True, (conf, steps), kernel_size, n_iter, norm_type, return_history, dilation)


def cspn2d_backward_kxk_assemble_pin(guidance, blur_depth, sparse_depth, pin_conf, conf, steps, grad_out, kernel_size=5, n_iter=24, norm_type="8sum",
                                     history=None, need_guidance=True, need_blur=True, need_conf=True, need_sparse=True, need_pin=True, dilation=1):
    """Gradient of cspn2d_forward_kxk_assemble_pin -> (dL/dguidance, dL/dblur_depth, dL/dconf, dL/dsparse_depth, dL/dpin_conf), None where not
    asked for; one engine call (cspn2d_backward_kxk_assemble_pin).  history: what cspn2d_forward_kxk_assemble_pin(..., return_history=True)
    returned; None runs that forward first where dL/dguidance, dL/dpin_conf (n_iter >= 2) or dL/dconf needs it."""
    return _fold_backward(guidance, blur_depth, sparse_depth, pin_conf, True, (conf, steps), grad_out, kernel_size, n_iter, norm_type, history, dilation,
                          need_guidance, need_blur, need_conf, need_sparse, need_pin)


# ---- non-local propagation with learned offsets (NLSPN's refinement step; cspn2d_nl.hip): every pixel reads its K*K - 1 neighbours by bilinear
# interpolation at p + base_k + offset_k(p).  Neighbour k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre and its base is
# (t - K//2, l - K//2): the deformable convolution's sign, THE OPPOSITE of the K x K engine's (K//2 - t, K//2 - l) above.  The six functions are
# float32 only; their *_g16 twins below them take aff and offset in float16 / bfloat16 as well ----
def _nl_kernel_size(kernel_size):
    K = _check_kernel_size(kernel_size, 4)
    if K != 3:
        raise ValueError("non-local propagation is built for kernel_size 3 only (5 and 7 are not), got %d" % K)
    return K


def _nl_tensor(t, name, shape=None, channels=None, g16=False):
    """float32 and nothing else (g16, for aff and offset of the *_g16 functions: float16 and bfloat16 as well), checked before the device;
    [B, channels, H, W] or exactly `shape`"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if g16 and t.dtype != torch.float32 and t.dtype not in _GATE16:
        raise TypeError("%s must be float32, float16 or bfloat16 (got %s)" % (name, t.dtype))
    if not g16 and t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s): the non-local entry points take no other dtype%s"
                        % (name, t.dtype, " (16-bit aff and offset: the *_g16 functions)" if name in ("aff", "offset") else ""))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    if shape is None and (t.dim() != 4 or (channels is not None and t.shape[1] != channels)):
        raise ValueError("%s must be [B,%s,H,W], got %s" % (name, "C" if channels is None else channels, tuple(t.shape)))


def _nl_offset(offset, K, g16=False):
    _nl_tensor(offset, "offset", channels=2 * (K * K - 1), g16=g16)
    return offset.shape[0], offset.shape[2], offset.shape[3]


def _nl_pair(aff, offset):
    """the *_g16 functions' pairs (aff, offset): (float32, float32), (float32, T) and (T, T), T float16 or bfloat16; anything else is a TypeError"""
    if aff.dtype != offset.dtype and aff.dtype != torch.float32:
        raise TypeError("aff %s with offset %s is not built: float32 or the offset's dtype with a 16-bit offset, float32 with a float32 one"
                        % (aff.dtype, offset.dtype))


def _nl_args(aff, offset, x, sparse_depth, kernel_size, n_iter, extra=(), g16=False):
    """-> K, B, C, H, W, n and the tensors on the GPU, contiguous: aff, offset, x, sparse_depth (or None), *extra (each of x's shape)"""
    K = _nl_kernel_size(kernel_size)
    B, H, W = _nl_offset(offset, K, g16)
    _nl_tensor(aff, "aff", (B, K * K - 1, H, W), g16=g16)
    if g16:
        _nl_pair(aff, offset)
    _nl_tensor(x, "x", channels=None)
    if x.shape[0] != B or tuple(x.shape[2:]) != (H, W) or x.shape[1] < 1:
        raise ValueError("x has shape %s, expected (B,C,H,W) = (%d,C,%d,%d)" % (tuple(x.shape), B, H, W))
    C = x.shape[1]
    if sparse_depth is not None:
        _nl_tensor(sparse_depth, "sparse_depth", (B, 1, H, W))
    for t, name in extra:
        _nl_tensor(t, name, (B, C, H, W))
    if isinstance(n_iter, bool) or int(n_iter) != n_iter or n_iter < 0:
        raise ValueError("n_iter must be an int >= 0 (got %r)" % (n_iter,))
    return K, B, C, H, W, int(n_iter)


def _nl_prep(*named):
    """on the GPU, contiguous, in the dtype _nl_tensor has let through"""
    ts = [None if t is None else _prep(t, name, dtype=t.dtype) for t, name in named]
    if any(t is not None and t.device != ts[0].device for t in ts):
        raise ValueError("all tensors must live on the same device")
    return ts


def _nl_typed(t):
    """a pointer of a *_g16 entry point with the dtype code behind it"""
    return _ptr(t), _GATE16.get(t.dtype, 0)


def _nl_forward(g16, aff, offset, x, sparse_depth, n_iter, kernel_size, return_history):
    K, B, C, H, W, n = _nl_args(aff, offset, x, sparse_depth, kernel_size, n_iter, g16=g16)
    if n == 0:
        return (x, None) if return_history else x
    a, o, h, s = _nl_prep((aff, "aff"), (offset, "offset"), (x, "x"), (sparse_depth, "sparse_depth"))
    out = torch.empty_like(h)
    if out.numel() == 0:
        return (out, None) if return_history else out
    # with a history the levels go there; the workspace keeps the pinned H_0 alone
    hist, hb = _history("cspn2d_nl_history_bytes", a.device, B, C, H, W, K, n) if return_history else (None, 0)
    gates = (*_nl_typed(a), *_nl_typed(o)) if g16 else (_ptr(a), _ptr(o))
    _launch("cspn2d_forward_nl_g16" if g16 else "cspn2d_forward_nl_f32", a.device, (*gates, _ptr(h), _ptr(s), _ptr(out), _ptr(hist), hb, B, C, H, W, K, n),
            ("cspn2d_nl_workspace_bytes", B, C, H, W, K, 1 if return_history else n, int(s is not None)))
    return (out, hist) if return_history else out


def cspn2d_forward_nl(aff, offset, x, sparse_depth, n_iter, kernel_size=3, return_history=False):
    """Non-local propagation, affinities as given (cspn2d_forward_nl_f32): aff [B,8,H,W] any sign, normalised by the caller; offset [B,16,H,W],
    channel 2k is dy_k and 2k+1 is dx_k; x [B,C,H,W], the C channels share aff and offset; sparse_depth [B,1,H,W] or None, pinned where > 0:
        Ht = sparse_depth where sparse_depth > 0 else H       (before every step)
        H <- (1 - sum_k aff_k) * Ht + sum_k aff_k * bil(Ht, p + base_k + offset_k(p)),      H_0 = x, n_iter times; the result is not pinned
    base_k = (t - 1, l - 1) for the k-th (t, l) of the 3 x 3 raster without the centre: the deformable convolution's sign, the opposite of the
    K x K functions'.  bil takes its fractions from the offset (offset - floor(offset)), a corner outside the image contributes 0, every finite
    offset is valid.  return_history: (out, history) for cspn2d_backward_nl.  n_iter == 0 returns x.  float32 only: any other dtype is a
    TypeError (cspn2d_forward_nl_g16 takes 16-bit aff and offset).  Bitwise reproducible."""
    return _nl_forward(False, aff, offset, x, sparse_depth, n_iter, kernel_size, return_history)


def _nl_backward(stem, aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size, history, need_aff, need_offset, need_x, g16=False):
    """cspn2d_backward_nl and its deterministic twin: stem + "_f32" (g16: "_g16") is the entry point, stem + "_workspace_bytes" its size query"""
    K, B, C, H, W, n = _nl_args(aff, offset, x, sparse_depth, kernel_size, n_iter, ((grad_out, "grad_out"),), g16)
    a, o, h, s, go = _nl_prep((aff, "aff"), (offset, "offset"), (x, "x"), (sparse_depth, "sparse_depth"), (grad_out, "grad_out"))
    ga = torch.empty_like(a) if need_aff else None
    gd = torch.empty_like(o) if need_offset else None
    gx = torch.empty_like(h) if need_x else None
    if not (need_aff or need_offset or need_x) or h.numel() == 0:
        return ga, gd, gx
    if (need_aff or need_offset) and n >= 2 and history is None:
        _, history = (cspn2d_forward_nl_g16 if g16 else cspn2d_forward_nl)(a, o, h, s, n, K, return_history=True)
    gates = (*_nl_typed(a), *_nl_typed(o)) if g16 else (_ptr(a), _ptr(o))
    _launch(stem + ("_g16" if g16 else "_f32"), a.device,
            (*gates, _ptr(h), _ptr(s), _ptr(history), _history_bytes(history), _ptr(go), _ptr(ga), _ptr(gd), _ptr(gx), B, C, H, W, K, n),
            (stem + "_workspace_bytes", B, C, H, W, K, n, int(s is not None)))
    return ga, gd, gx


def cspn2d_backward_nl(aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size=3, history=None, need_aff=True, need_offset=True, need_x=True):
    """Gradient of cspn2d_forward_nl -> (dL/daff [B,8,H,W] and dL/doffset [B,16,H,W], each summed over the C channels, dL/dx [B,C,H,W]), None where
    not asked for; cspn2d_backward_nl_f32.  sparse_depth has no gradient; floor has none either, so dL/doffset is the derivative of the bilinear
    fractions.  history: what cspn2d_forward_nl(..., return_history=True) returned; None runs that forward first where dL/daff or dL/doffset needs it
    (n_iter >= 2).  NOT run-to-run bitwise: the adjoint scatters with float atomics, whose sums depend on arrival order in their last bits
    (cspn2d_backward_nl_det is)."""
    return _nl_backward("cspn2d_backward_nl", aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size, history, need_aff, need_offset, need_x)


def cspn2d_backward_nl_det(aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size=3, history=None, need_aff=True, need_offset=True, need_x=True):
    """cspn2d_backward_nl as a deterministic function of its inputs (cspn2d_backward_nl_det_f32): RUN-TO-RUN BITWISE in all three gradients.  The
    adjoint gathers through an inverted index of the operator, built once per call, and sums each destination's terms in an order-independent way
    (quantised to a common exponent, added in int64; include/cspn_amd.h); no float atomics.  The same arguments and return convention; the results
    agree with cspn2d_backward_nl's within rounding, not bit for bit.  The index costs about 270 bytes a pixel of workspace (B H W pixels)."""
    return _nl_backward("cspn2d_backward_nl_det", aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size, history, need_aff, need_offset, need_x)


def _nl_sample(g16, offset, f, kernel_size):
    K = _nl_kernel_size(kernel_size)
    B, H, W = _nl_offset(offset, K, g16)
    _nl_tensor(f, "f", (B, 1, H, W))
    o, v = _nl_prep((offset, "offset"), (f, "f"))
    out = torch.empty((B, K * K - 1, H, W), dtype=torch.float32, device=o.device)
    if out.numel():
        if g16:
            _launch("cspn2d_nl_sample_g16", o.device, (*_nl_typed(o), _ptr(v), _ptr(out), B, H, W, K))
        else:
            _launch("cspn2d_nl_sample_f32", o.device, (_ptr(o), _ptr(v), _ptr(out), B, H, W, K))
    return out


def cspn2d_nl_sample(offset, f, kernel_size=3):
    """The sampling operator of cspn2d_forward_nl on its own: out[:, k](p) = bil(f, p + base_k + offset_k(p)), f [B,1,H,W] -> [B,8,H,W]
    (cspn2d_nl_sample_f32).  Bitwise reproducible."""
    return _nl_sample(False, offset, f, kernel_size)


def _nl_sample_backward(det, offset, f, grad_out, kernel_size, need_f, need_offset, g16=False):
    K = _nl_kernel_size(kernel_size)
    B, H, W = _nl_offset(offset, K, g16)
    _nl_tensor(f, "f", (B, 1, H, W))
    _nl_tensor(grad_out, "grad_out", (B, K * K - 1, H, W))
    o, v, go = _nl_prep((offset, "offset"), (f, "f"), (grad_out, "grad_out"))
    gf = torch.empty_like(v) if need_f else None
    gd = torch.empty_like(o) if need_offset else None
    if (need_f or need_offset) and v.numel():
        args = ((*_nl_typed(o),) if g16 else (_ptr(o),)) + (_ptr(v), _ptr(go), _ptr(gf), _ptr(gd), B, H, W, K)
        tail = "_g16" if g16 else "_f32"
        if det:
            _launch("cspn2d_nl_sample_backward_det" + tail, o.device, args, ("cspn2d_nl_sample_backward_det_workspace_bytes", B, H, W, K))
        else:
            _launch("cspn2d_nl_sample_backward" + tail, o.device, args)
    return gf, gd


def cspn2d_nl_sample_backward(offset, f, grad_out, kernel_size=3, need_f=True, need_offset=True):
    """Gradient of cspn2d_nl_sample -> (dL/df [B,1,H,W], dL/doffset [B,16,H,W]), None where not asked for (cspn2d_nl_sample_backward_f32).  dL/df is
    scattered with float atomics: not run-to-run bitwise (cspn2d_nl_sample_backward_det is); dL/doffset is written once."""
    return _nl_sample_backward(False, offset, f, grad_out, kernel_size, need_f, need_offset)


def cspn2d_nl_sample_backward_det(offset, f, grad_out, kernel_size=3, need_f=True, need_offset=True):
    """cspn2d_nl_sample_backward as a deterministic function of its inputs (cspn2d_nl_sample_backward_det_f32): RUN-TO-RUN BITWISE.  dL/df is
    gathered through the inverted index of the sampling operator and summed in an order-independent way, as in cspn2d_backward_nl_det; about 260
    bytes a pixel of workspace."""
    return _nl_sample_backward(True, offset, f, grad_out, kernel_size, need_f, need_offset)


# ---- the same six on float16 / bfloat16 affinities and offsets (the cspn2d_*_nl*_g16 entry points): what a head under torch.autocast emits, taken
# as it is.  aff / offset come in the pairs (float32, float32), (float32, T), (T, T), T float16 or bfloat16; any other pair, or float64, is a
# TypeError raised before the device.  Everything else is float32.  A 16-bit value is widened exactly where the kernels read it, so every result
# is bitwise the float32 function's on aff.float(), offset.float(); dL/daff and dL/doffset come back in the dtype of aff and of offset, the float32
# value rounded once.  Signatures, workspaces and histories are the twins' ----
def cspn2d_forward_nl_g16(aff, offset, x, sparse_depth, n_iter, kernel_size=3, return_history=False):
    """cspn2d_forward_nl on aff / offset in float32, float16 or bfloat16 (cspn2d_forward_nl_g16): out and the history are float32 and bitwise
    cspn2d_forward_nl(aff.float(), offset.float(), ...); no widened copy is made."""
    return _nl_forward(True, aff, offset, x, sparse_depth, n_iter, kernel_size, return_history)


def cspn2d_backward_nl_g16(aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size=3, history=None, need_aff=True, need_offset=True, need_x=True):
    """cspn2d_backward_nl on aff / offset in float32, float16 or bfloat16 (cspn2d_backward_nl_g16): dL/daff in aff's dtype, dL/doffset in offset's
    (the float32 sums rounded once, to nearest even), dL/dx float32.  Not run-to-run bitwise, as its twin."""
    return _nl_backward("cspn2d_backward_nl", aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size, history, need_aff, need_offset, need_x, True)


def cspn2d_backward_nl_det_g16(aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size=3, history=None, need_aff=True, need_offset=True, need_x=True):
    """cspn2d_backward_nl_det on aff / offset in float32, float16 or bfloat16 (cspn2d_backward_nl_det_g16), RUN-TO-RUN BITWISE: dL/dx is bitwise
    cspn2d_backward_nl_det's on the widened tensors, dL/daff and dL/doffset are bitwise its results cast to aff's and offset's dtype."""
    return _nl_backward("cspn2d_backward_nl_det", aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size, history, need_aff, need_offset, need_x, True)


def cspn2d_nl_sample_g16(offset, f, kernel_size=3):
    """cspn2d_nl_sample on an offset in float32, float16 or bfloat16 (cspn2d_nl_sample_g16): bitwise cspn2d_nl_sample(offset.float(), f)."""
    return _nl_sample(True, offset, f, kernel_size)


def cspn2d_nl_sample_backward_g16(offset, f, grad_out, kernel_size=3, need_f=True, need_offset=True):
    """cspn2d_nl_sample_backward on an offset in float32, float16 or bfloat16 (cspn2d_nl_sample_backward_g16): dL/doffset in the offset's dtype."""
    return _nl_sample_backward(False, offset, f, grad_out, kernel_size, need_f, need_offset, True)


def cspn2d_nl_sample_backward_det_g16(offset, f, grad_out, kernel_size=3, need_f=True, need_offset=True):
    """cspn2d_nl_sample_backward_det on an offset in float32, float16 or bfloat16 (cspn2d_nl_sample_backward_det_g16): RUN-TO-RUN BITWISE."""
    return _nl_sample_backward(True, offset, f, grad_out, kernel_size, need_f, need_offset, True)


def assemble_conf(iter_conf, kernel_conf, k, T, like):
    """the confidences one kernel size of Affinity_PropagateAssemble hands to the engine: iter_conf [B,T,H,W] (None: ones) times
    kernel_conf[:, k:k+1] (None: no such factor), one differentiable torch op; like: blur_depth (batch, image size, device)"""
    B, _, H, W = like.shape
    if iter_conf is None and kernel_conf is None:
        return torch.ones((B, T, H, W), dtype=torch.float32, device=like.device)
    if kernel_conf is None:
        return iter_conf
    a = kernel_conf[:, k:k + 1]
    return a.expand(B, T, H, W) if iter_conf is None else iter_conf * a


# ---- the demo's module (reference cspn_paddle/demo.py:20-54): abs (:24), each channel's slice of K = 3^d - 1 gates divided by its own
# channel sum (:25,31-36,47-49), prop_step chained propagations (:40-43,50-52) ----
def _absnorm_flat(guide, K):
    """guide [N, M, *S] with M % K == 0 -> the flat (N M / K, V) the C ABI takes"""
    if not isinstance(guide, torch.Tensor):
        raise TypeError("guide must be a torch.Tensor")
    if K not in (8, 26, 24, 48):
        raise ValueError("K must be 8 (2D), 26 (3D), 24 or 48 (2D 5 x 5 / 7 x 7), got %r" % (K,))
    if guide.dim() < 3 or guide.shape[1] % K != 0 or guide.shape[1] == 0:
        raise ValueError("guide must be [N, C*%d, *S], got %s" % (K, tuple(guide.shape)))
    V = 1
    for s in guide.shape[2:]:
        V *= int(s)
    return guide.shape[0] * (guide.shape[1] // K), V


def _gate_absnorm(guide, K, allow16=False):
    """allow16 (the 3D module's backward, K = 26): a float16 / bfloat16 guide as it is -> float32 gates (cspn_gate_absnorm_g16)"""
    S, V = _absnorm_flat(guide, K)
    g, dt = _prep_gate(guide, "guide") if allow16 and K == 26 else (_prep(guide, "guide"), None)
    out = torch.empty_like(g, dtype=torch.float32)
    if out.numel() == 0:
        return out
    _launch("cspn_gate_absnorm_f32" if dt is None else "cspn_gate_absnorm_g16", g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(out), S, K, V))
    return out


def _gate_absnorm_backward26(guide, grad_gate):
    """the 3D module's chain through the normalisation: guide float32, float16 or bfloat16, grad_gate = dL/dw float32 -> dL/dguide in the
    guide's dtype (cspn_gate_absnorm_backward_f32 / _g16: the float32 value, rounded once at its store)"""
    S, V = _absnorm_flat(guide, 26)
    g, dt = _prep_gate(guide, "guide")
    r = _prep(grad_gate, "grad_gate", tuple(g.shape))
    out = torch.empty_like(g)
    if out.numel() == 0:
        return out
    _launch("cspn_gate_absnorm_backward_f32" if dt is None else "cspn_gate_absnorm_backward_g16", g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(r), _ptr(out), S, 26, V))
    return out


def gate_absnorm_backward(guide, grad_gate, K):
    """The adjoint of gate_absnorm (cspn_gate_absnorm_backward_f32): guide raw, grad_gate = dL/dw, both [N, C*K, *S] -> dL/dguide,
    sign(g_k) (dL/dw_k - sum_j w_j dL/dw_j) / sum_j |g_j| per slice (sign(0) = 0, torch's abs backward; NaN for an all-zero voxel)."""
    S, V = _absnorm_flat(guide, K)
    g = _prep(guide, "guide")
    r = _prep(grad_gate, "grad_gate", tuple(g.shape))
    if r.device != g.device:
        raise _lib.CspnError("cspn_amd: guide is on %s, grad_gate on %s: all tensors must live on the same device" % (g.device, r.device))
    out = torch.empty_like(g)
    if out.numel() == 0:
        return out
    _launch("cspn_gate_absnorm_backward_f32", g.device, (_ptr(g), _ptr(r), _ptr(out), S, K, V))
    return out


class _GateAbsnormFunction(torch.autograd.Function):
    """gate_absnorm under autograd: keeps the raw guide, the backward is one cspn_gate_absnorm_backward_f32 launch"""

    @staticmethod
    def forward(ctx, guide, K):
        ctx.K = K
        ctx.save_for_backward(guide)
        return _gate_absnorm(guide, K)

    @staticmethod
    def backward(ctx, grad_gate):
        guide, = ctx.saved_tensors
        return gate_absnorm_backward(guide, grad_gate, ctx.K), None


def gate_absnorm(guide, K):
    """The demo's gate normalisation (reference cspn_paddle/demo.py:24,34-36,47-49) as one HIP pass: guide [N, C*K, *S] -> w of the same
    shape, w_k = |g_k| / sum_j |g_j| per voxel over each channel's slice of K gates (K = 26 in 3D, 8 in 2D, 24 / 48 for the 2D 5 x 5 / 7 x 7
    neighbourhoods; the sum in channel order;
    NaN where a slice is all zero, as torch's 0 / 0).  Differentiable w.r.t. guide when grad mode is on and guide requires grad."""
    if torch.is_grad_enabled() and isinstance(guide, torch.Tensor) and guide.requires_grad:
        return _GateAbsnormFunction.apply(guide, K)
    return _gate_absnorm(guide, K)


def cspn3d_forward_absnorm(guide, feat, n_iter=12, algo="auto"):
    """guide [B,26,D,H,W] RAW, feat [B,1,D,H,W] -> [B,1,D,H,W]: gate_absnorm(guide, 26), then cspn3d_forward(..., 'none') -- one engine call
    (cspn3d_forward_absnorm_f32).  algo 'auto' normalises the resident gates inside the persistent kernel wherever the NONE op would take
    it; 'stepwise' normalises into the workspace and steps; 'persistent' raises CspnError where the kernel cannot take the call.
    guide may be float16 / bfloat16 (cspn3d_forward_absnorm_g16: widened exactly where it is read, out is float32 and bitwise the float32
    call on guide.float()); a 16-bit feat is widened with one cast."""
    if guide.dim() != 5 or guide.shape[1] != 26:
        raise ValueError("guide must be [B,26,D,H,W], got %s" % (tuple(guide.shape),))
    B, _, D, H, W = guide.shape
    g, dt = _prep_gate(guide, "guide")
    h = _prep_value(feat, "feat", (B, 1, D, H, W))
    if h.device != g.device:
        raise _lib.CspnError("cspn_amd: guide is on %s, feat on %s: all tensors must live on the same device" % (g.device, h.device))
    if h.data_ptr() % 16:
        h = h.clone()   # (an aligned copy: misaligned values would need the folding path's workspace)
    out = torch.empty_like(h)
    if B == 0:
        return out
    _launch("cspn3d_forward_absnorm_f32" if dt is None else "cspn3d_forward_absnorm_g16", g.device,
            (_ptr(g), *(() if dt is None else (dt,)), _ptr(h), _ptr(out), B, D, H, W, int(n_iter), _lib.ALGOS_3D[algo]),
            ("cspn3d_forward_absnorm_workspace_bytes", B, D, H, W, int(n_iter)))
    return out


def _absnorm_fold(guide, feat, kernel_size=3):
    """per-channel gates are batch folding: [N, C*K, *S] -> [N*C, K, *S] and [N, C, *S] -> [N*C, 1, *S] (views, no copy)"""
    N, C = feat.shape[:2]
    S = tuple(feat.shape[2:])
    K = kernel_size ** len(S) - 1
    return guide.view(N * C, K, *S), feat.view(N * C, 1, *S), K


def _absnorm_forward(guide, feat, n_iter, kernel_size=3, keep_history=False):
    """-> (out, history): history is the K x K forward's H_1 .. H_{n-1} where keep_history asks for it, else None"""
    g, x, K = _absnorm_fold(guide, feat, kernel_size)
    hist = None
    if K == 26:
        out = cspn3d_forward_absnorm(g, x, n_iter)
    elif K == 8:   # 2D: the normaliser, then the NONE op (the 2D loop is generated assembly: no fused normalisation there)
        out = cspn2d_forward(_gate_absnorm(g, 8), x, None, n_iter, "none")
    else:          # 2D K x K: the K x K engine normalises the resident gates in its step
        out = cspn2d_forward_kxk_absnorm(g, x, kernel_size, n_iter, return_history=keep_history)
        if keep_history:
            out, hist = out
    return out.view(feat.shape), hist


class _AbsnormPropagateFunction(torch.autograd.Function):
    """the demo's module under autograd.  3 x 3 (x 3): the backward recomputes w with the normaliser, runs the NONE op's backward on the
    folded N*C batch and chains the gate gradient through cspn_gate_absnorm_backward_f32 (3D: the guide may be float16 / bfloat16 -- w is
    recomputed in float32 from it and dL/dguide comes back in its dtype, cspn_gate_absnorm*_g16).  K x K: the forward keeps its levels where the
    guide gradient needs them, the backward is one cspn2d_backward_kxk_absnorm call on the raw guide (float32, float16 or bfloat16)"""

    @staticmethod
    def forward(ctx, guide, feat, n_iter, kernel_size):
        ctx.n_iter, ctx.kernel_size = n_iter, kernel_size
        out, hist = _absnorm_forward(guide, feat, n_iter, kernel_size, keep_history=kernel_size != 3 and ctx.needs_input_grad[0] and n_iter >= 2)
        ctx.save_for_backward(guide, feat, hist)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        guide, feat, hist = ctx.saved_tensors
        need_g, need_x = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g, x, K = _absnorm_fold(guide, feat, ctx.kernel_size)
        go = grad_out.contiguous().view(x.shape)
        if K not in (8, 26):
            gg, gx = cspn2d_backward_kxk_absnorm(g, x, go, ctx.kernel_size, ctx.n_iter, hist, need_g, need_x)
            return gg.view(guide.shape) if need_g else None, gx.view(feat.shape) if need_x else None, None, None
        w = _gate_absnorm(g, K, allow16=True)
        if K == 26:
            gw, gx = cspn3d_backward(w, x, go, ctx.n_iter, need_g, need_x)
            gg = _gate_absnorm_backward26(g, gw).view(guide.shape) if need_g else None
        else:
            gw, gx = cspn2d_backward(w, x, None, go, ctx.n_iter, "none", need_g, need_x)
            gg = gate_absnorm_backward(g, gw, K).view(guide.shape) if need_g else None
        return gg, gx.view(feat.shape) if need_x else None, None, None


def absnorm_propagate(guide, feat, n_iter, kernel_size=3):
    """The demo's CSPN.cspn (reference cspn_paddle/demo.py:20-54) as a function: feat [N,C,*S] (len(S) = 2 or 3), guide [N, C*K, *S] raw
    with K = kernel_size^len(S) - 1; channel c is propagated on its OWN slice guide[:, c*K:(c+1)*K], normalised by its abs-sum at every
    voxel, for n_iter chained steps.  One engine call for all channels (they fold into the batch).  3D: cspn3d_forward_absnorm_f32 (the
    normalisation inside the persistent kernel where it runs); 2D: gate_absnorm, then cspn2d_forward(..., 'none'); with kernel_size
    5 / 7 (2D only) cspn2d_forward_kxk_absnorm / cspn2d_backward_kxk_absnorm on the folded views, which normalise the gates inside the
    K x K step and store no normalised gate.  That route and the 3D one take a float16 / bfloat16 guide as it is (dL/dguide comes back in its
    dtype; 3D: cspn3d_forward_absnorm_g16, and in the backward the normaliser's 16-bit forms) and widen a 16-bit feat with one differentiable
    cast; the result is float32.  (2D 3 x 3 takes float32 only.)  Differentiable w.r.t. guide and feat.
    n_iter == 0 returns feat itself."""
    for t, name in ((guide, "guide"), (feat, "feat")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch.Tensor" % name)
    if feat.dim() not in (4, 5):
        raise ValueError("feat must be [N,C,H,W] or [N,C,D,H,W], got %s" % (tuple(feat.shape),))
    if kernel_size != 3:
        _check_kernel_size(kernel_size, feat.dim())
    K = kernel_size ** (feat.dim() - 2) - 1
    N, C = feat.shape[:2]
    if tuple(guide.shape) != (N, C * K) + tuple(feat.shape[2:]):
        raise ValueError("guide has shape %s, expected (N, C*%d, *S) = %s" % (tuple(guide.shape), K, (N, C * K) + tuple(feat.shape[2:])))
    if int(n_iter) < 0:
        raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
    if int(n_iter) == 0:
        return feat
    if kernel_size != 3 or feat.dim() == 5:
        g = _prep_gate(guide, "guide")[0]
        x = _prep(widen16(feat), "feat")
    else:
        g = _prep(guide, "guide")
        x = _prep(feat, "feat")
    if g.device != x.device:
        raise _lib.CspnError("cspn_amd: guide is on %s, feat on %s: all tensors must live on the same device" % (g.device, x.device))
    if torch.is_grad_enabled() and (guide.requires_grad or feat.requires_grad):
        return _AbsnormPropagateFunction.apply(g, x, int(n_iter), kernel_size)
    return _absnorm_forward(g, x, int(n_iter), kernel_size)[0]
