"""Device-side mirrors of the small steps next to the propagation path in the reference training / evaluation loops
(SURVEY.md §8f-3, §8f-4), same names and call signatures:

    reference                                                   here
    utils.evaluate_error(gt_depth, pred_depth)   utils.py:19-47   evaluate_error(gt_depth, pred_depth) -> same dict, one
                                                                  fused masked reduction on the GPU, one 48-byte copy back
    loss.Wighted_L1_Loss()(pred, label)          loss.py:16-23    Wighted_L1_Loss()(pred, label) -> 0-d tensor, differentiable
    Unpool(num_channels, stride=2)(x)            torch_resnet_cspn_nyu.py:41-54   Unpool(num_channels, stride)(x), differentiable

    createSparseDepthImage(depth_image, n_sample)                 createSparseDepthImage(depth, n_sample, mode='nyu'|'kitti',
      nyu_dataset_loader.py:135-144, kitti_dataset_loader.py:138-148   seed): the Bernoulli mask drawn on the GPU, batched
    gud_up_proj_layer6(x), gud_up_proj_layer5(x)                  guidance_heads(x, layer6.conv1.weight, layer5.conv1.weight, oheight, owidth
      torch_resnet_cspn_nyu.py:187-206, :318-319, :372-373          [, norm_type]): both Simple_Gudi_UpConv_Block_Last_Layer heads (Unpool + 3x3 conv) as
                                                                  ONE kernel; with norm_type the guidance comes back as gate_wb; differentiable

The reference moves every prediction to the host before reducing it (train.py:204-206, eval.py:146-150)."""
import collections

import torch
import torch.nn as nn

from . import _lib
from .functional import _GATE16, _launch, _prep, _ptr, cspn2d_normalize

_KEYS = ['MSE', 'RMSE', 'ABS_REL', 'LG10', 'MAE', 'DELTA1.02', 'DELTA1.05', 'DELTA1.10', 'DELTA1.25', 'DELTA1.25^2',
         'DELTA1.25^3']


def _metrics(gt, pred):
    """-> device float32[12]: n_valid, then the 11 values of _KEYS"""
    g = _prep(gt, "gt_depth")
    p = _prep(pred, "pred_depth", tuple(g.shape))
    out = torch.empty(12, dtype=torch.float32, device=g.device)
    n = g.numel()
    _launch("cspn_metrics_f32", g.device, (_ptr(g), _ptr(p), n, _ptr(out)), ("cspn_metrics_workspace_bytes", n))
    return out


def evaluate_error(gt_depth, pred_depth):
    """reference utils.py:19-47: dict of python floats (0 everywhere when no pixel has gt > 1e-4)"""
    v = _metrics(gt_depth, pred_depth).tolist()
    return {k: v[i + 1] for i, k in enumerate(_KEYS)}


class _L1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label):
        stats = _metrics(label, pred)
        ctx.save_for_backward(pred, label, stats)
        # MAE over label > 1e-4 == loss.py:18-22; nothing valid: loss.py:21-22 computes 0/0 = nan
        return torch.where(stats[0] > 0, stats[5], stats[5] + float("nan"))

    @staticmethod
    def backward(ctx, grad):
        pred, label, stats = ctx.saved_tensors
        p, l = pred.contiguous(), label.contiguous()
        gp = torch.empty_like(p)
        gs = grad.reshape(1).to(torch.float32).contiguous()
        _launch("cspn_l1_backward_f32", p.device, (_ptr(p), _ptr(l), _ptr(stats), _ptr(gs), _ptr(gp), p.numel()))
        return gp.view_as(pred), None


class Wighted_L1_Loss(nn.Module):
    """reference loss.py:12-23 (spelling as there)"""

    def forward(self, pred, label):
        return _L1.apply(pred, label)


class _Unpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride):
        xc = _prep(x, "x")
        N, C, H, W = xc.shape
        out = torch.empty(N, C, H * stride, W * stride, dtype=torch.float32, device=xc.device)
        ctx.shape, ctx.stride = (N, C, H, W), stride
        _launch("cspn_unpool_f32", xc.device, (_ptr(xc), _ptr(out), N * C, H, W, stride))
        return out

    @staticmethod
    def backward(ctx, go):
        N, C, H, W = ctx.shape
        g = go.contiguous()
        gx = torch.empty(N, C, H, W, dtype=torch.float32, device=g.device)
        _launch("cspn_unpool_backward_f32", g.device, (_ptr(g), _ptr(gx), N * C, H, W, ctx.stride))
        return gx, None


class Unpool(nn.Module):
    """reference torch_resnet_cspn_nyu.py:41-54: stride x stride unpooling with zero padding (no parameters)"""

    def __init__(self, num_channels, stride=2):
        super(Unpool, self).__init__()
        self.num_channels = num_channels
        self.stride = stride

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.num_channels:
            raise ValueError("expected [N,%d,H,W], got %s" % (self.num_channels, tuple(x.shape)))
        return _Unpool.apply(x, self.stride)


def createSparseDepthImage(depth_image, n_sample, mode="nyu", seed=0):
    """reference nyu_dataset_loader.py:135-144 (mode 'nyu': keep probability n_sample / n_pixels) and
    kitti_dataset_loader.py:138-148 (mode 'kitti': n_sample / n_valid_pixels, valid = depth > 1e-4), on the GPU:
    sparse_depth = depth_image * bernoulli(p), independently per pixel.  depth_image [..., H, W] on the device (any number
    of leading dims; every [H, W] slice is one image).  `seed` keys a counter-based generator (a fixed seed reproduces the
    mask; the reference draws from torch's global CPU generator)."""
    d = _prep(depth_image, "depth_image")
    if d.dim() < 2:
        raise ValueError("depth_image must be [..., H, W]")
    hw = d.shape[-1] * d.shape[-2]
    n_images = d.numel() // hw if hw else 0
    out = torch.empty_like(d)
    if d.numel() == 0:
        return out
    m = {"nyu": 0, "kitti": 1}[mode]
    _launch("cspn_sparse_sample_f32", d.device, (_ptr(d), _ptr(out), n_images, hw, int(n_sample), m, int(seed) & (2 ** 64 - 1)),
            ("cspn_sparse_sample_workspace_bytes", n_images))
    return out


_PLANES_TO_K = {8: 3, 24: 5, 48: 7}

# What differs between the four host paths of the heads.  fwd / bwd: the entry points (_lib.check reports under these names); *_ws: their workspace queries;
# *_ws_args: the queries' arguments, letters of B C h w K.  x16: x and dL/dx are float16 / bfloat16 and a dtype code follows x in both calls; guidance16: the
# guidance and its gradient are in x's dtype too (float32 otherwise; blur, its gradient and the weights are float32 on every path).  K: both calls end in K;
# norm: the forward call ends in a norm_type
_HeadPath = collections.namedtuple("_HeadPath", "fwd fwd_ws fwd_ws_args bwd bwd_ws bwd_ws_args x16 guidance16 K norm")
_HEAD_PATHS = {
    "f32": _HeadPath("cspn_guidance_head_f32", "cspn_guidance_head_workspace_bytes", "C",
                     "cspn_guidance_head_backward_f32", "cspn_guidance_head_backward_workspace_bytes", "BChw", False, False, False, True),
    "kxk_f32": _HeadPath("cspn_guidance_head_kxk_f32", "cspn_guidance_head_kxk_workspace_bytes", "BChwK",
                         "cspn_guidance_head_kxk_backward_f32", "cspn_guidance_head_kxk_backward_workspace_bytes", "BChwK", False, False, True, False),
    "kxk_g16": _HeadPath("cspn_guidance_head_kxk_g16", "cspn_guidance_head_kxk_g16_workspace_bytes", "BChwK",
                         "cspn_guidance_head_kxk_backward_g16", "cspn_guidance_head_kxk_backward_g16_workspace_bytes", "BChwK", True, True, True, False),
    "g16": _HeadPath("cspn_guidance_head_g16", "cspn_guidance_head_g16_workspace_bytes", "BChw",
                     "cspn_guidance_head_backward_g16", "cspn_guidance_head_backward_g16_workspace_bytes", "BChw", True, False, False, False),
}


def _head_planes(x, weight_guidance, *others):
    """the argument checks guidance_heads and guidance_heads_backward share -> the guidance head's plane count: 8, 24 or 48 (prop_kernel 3, 5 or 7)"""
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be [B,C,h,w], got %s" % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__,))
    if not isinstance(weight_guidance, torch.Tensor) or weight_guidance.dim() != 4 or int(weight_guidance.shape[0]) not in _PLANES_TO_K:
        raise ValueError("weight_guidance must be [8 | 24 | 48, C, 3, 3] (prop_kernel 3, 5 or 7: K*K-1 planes), got %s"
                         % (tuple(weight_guidance.shape) if isinstance(weight_guidance, torch.Tensor) else type(weight_guidance).__name__,))
    for t in (weight_guidance,) + others:
        if isinstance(t, torch.Tensor) and t.device != x.device:
            raise ValueError("all tensors must live on the same device")
    return int(weight_guidance.shape[0])


def _head_path(x, weight_guidance, weight_blur, P, guidance_dtype, norm_type=None):
    """-> the path of _HEAD_PATHS that the dtype of x, the plane count P and guidance_dtype select.  Raised before any device check: ValueError for a misused
    guidance_dtype and for a norm_type on any head but the float32 8-plane one, TypeError for a 16-bit x with 8-plane weights by default, and for 16-bit weights
    whose dtype differs from x's"""
    x16 = x.dtype in _GATE16
    if guidance_dtype is not None:
        if guidance_dtype is not torch.float32:
            raise ValueError("guidance_dtype must be None or torch.float32, got %r" % (guidance_dtype,))
        if P != 8:
            raise ValueError("guidance_dtype=torch.float32 is the 8-plane head's (prop_kernel 3); the %d-plane head of prop_kernel %d returns its guidance in the "
                             "dtype of x" % (P, _PLANES_TO_K[P]))
        if not x16:
            raise ValueError("guidance_dtype=torch.float32 is for a float16 / bfloat16 x; x is %s (a float32 x takes the default guidance_dtype=None)" % (x.dtype,))
        if norm_type is not None:
            raise ValueError("the 16-bit 8-plane head returns raw guidance only (norm_type=None): Affinity_Propagate(prop_time, 3, norm_type) normalises it")
    elif x16 and P == 8:
        raise TypeError("the 3 x 3 guidance head (weight_guidance [8, C, 3, 3]) is float32 only: its ring has no 16-bit consumer; x is %s -- pass x.float(), "
                        "or use the 24- / 48-plane heads of prop_kernel 5 / 7 (guidance_dtype=torch.float32, or cspn_amd.GuidanceHeads, runs the 16-bit head that emits "
                        "float32 guidance)" % (x.dtype,))
    if x16:
        for t, name in ((weight_guidance, "weight_guidance"), (weight_blur, "weight_blur")):
            if isinstance(t, torch.Tensor) and t.dtype in _GATE16 and t.dtype != x.dtype:
                raise TypeError("x is %s but %s is %s: 16-bit weights must have the dtype of x (or be the float32 master weights)" % (x.dtype, name, t.dtype))
    if P != 8 and norm_type is not None:
        raise ValueError("the %d-plane guidance head returns raw guidance only (norm_type=None): Affinity_PropagateKxK(prop_time, %d, norm_type) "
                         "normalises it" % (P, _PLANES_TO_K[P]))
    return _HEAD_PATHS[("g16" if P == 8 else "kxk_g16") if x16 else ("f32" if P == 8 else "kxk_f32")]


def _head_prep(path, x, weight_guidance, weight_blur, P):
    """-> x and the two weights (weight_blur may be None), checked and contiguous.  x: float32, or its own 16-bit dtype dt on the x16 paths; there a weight is
    the float32 master or a dt tensor, which stays dt here (the autograd Function saves it as given) and is widened with .float(), exactly, at the call"""
    dt = x.dtype if path.x16 else torch.float32
    xx = _prep(x, "x", None, dt)
    C = xx.shape[1]
    wg, wb = (_prep(t, name, (planes, C, 3, 3), dt if getattr(t, "dtype", None) == dt else torch.float32) if t is not None else None
              for t, name, planes in ((weight_guidance, "weight_guidance", P), (weight_blur, "weight_blur", 1)))
    return xx, wg, wb


def _head_prep_grads(path, xx, wb, P, grad_guidance, grad_blur):
    """-> dL/dguidance [B,P,H,W] in the path's guidance dtype and dL/dblur [B,1,H,W] float32 (None without a blur head), checked and contiguous"""
    if not isinstance(grad_guidance, torch.Tensor) or grad_guidance.dim() != 4:
        raise ValueError("grad_guidance must be [B,%d,H,W]" % P)
    B, H, W = xx.shape[0], int(grad_guidance.shape[2]), int(grad_guidance.shape[3])
    gg = _prep(grad_guidance, "grad_guidance", (B, P, H, W), xx.dtype if path.guidance16 else torch.float32)
    return gg, _prep(grad_blur, "grad_blur", (B, 1, H, W)) if wb is not None else None


def _head_out_size(xx, oheight, owidth):
    return (int(oheight), int(owidth)) if (oheight and owidth) else (2 * xx.shape[2], 2 * xx.shape[3])


def _head_call(path, backward, xx, wg, tensors, H, W, norm=()):
    """one head entry point of `path` on prepared tensors (float32 weights): x [, dtype code], the other tensors, the sizes [, K | norm_type], the workspace"""
    B, C, h, w = xx.shape
    dims = dict(B=B, C=C, h=h, w=w, K=_PLANES_TO_K[int(wg.shape[0])])
    name, ws, ws_args = (path.bwd, path.bwd_ws, path.bwd_ws_args) if backward else (path.fwd, path.fwd_ws, path.fwd_ws_args)
    _launch(name, xx.device, (_ptr(xx), *((_GATE16[xx.dtype],) if path.x16 else ()), _ptr(wg), *map(_ptr, tensors), B, C, h, w, H, W,
                              *((dims["K"],) if path.K else ()), *norm), (ws, *(dims[k] for k in ws_args)))


def _heads_forward(path, xx, wg, wb, H, W, norm_type=None):
    """path.fwd: both heads on xx, raw -- or, on the float32 8-plane path, normalised by norm_type behind the conv -> guidance (float32, or xx's dtype on the
    guidance16 path: the accumulator rounded once), blur float32 (None without a blur head).  On the x16 paths the engine rounds the float32 weights once to
    xx's dtype"""
    B, P = xx.shape[0], int(wg.shape[0])
    g = torch.empty(B, P, H, W, dtype=xx.dtype if path.guidance16 else torch.float32, device=xx.device)
    b = torch.empty(B, 1, H, W, dtype=torch.float32, device=xx.device) if wb is not None else None
    _head_call(path, False, xx, wg, (wb, g, b), H, W, (_lib.NORM_TYPES[norm_type or "none"],) if path.norm else ())
    return g, b


def _heads_backward(path, xx, wg, wb, gg, gb, need_x, need_w):
    """path.bwd -> dL/dx in xx's dtype (rounded once on the x16 paths, where the float32 gradients are rounded once to xx's dtype as they enter the GEMMs), the
    weight gradients float32; skipped outputs are None"""
    dx = torch.empty_like(xx) if need_x else None
    dwg = torch.empty_like(wg) if need_w else None
    dwb = torch.empty_like(wb) if (need_w and wb is not None) else None
    _head_call(path, True, xx, wg, (wb, gg, gb, dx, dwg, dwb), int(gg.shape[2]), int(gg.shape[3]))
    return dx, dwg, dwb


def _f32(t):
    return t.float() if t is not None else None


def guidance_heads_backward(x, weight_guidance, weight_blur, grad_guidance, grad_blur, need_x=True, need_w=True, guidance_dtype=None):
    """cspn_guidance_head_backward_f32: (dL/dx, dL/dweight_guidance, dL/dweight_blur) of the RAW heads -- what torch autograd computes through the two reference
    layers (torch_resnet_cspn_nyu.py:187-206) -- from dL/dguidance [B,8,H,W] and dL/dblur [B,1,H,W] (None without a blur head); skipped outputs are None.
    weight_guidance [24 | 48, C, 3, 3] with dL/dguidance [B, 24 | 48, H, W]: cspn_guidance_head_kxk_backward_f32, the heads of prop_kernel 5 / 7.
    With those weights x may be float16 / bfloat16 = dt (cspn_guidance_head_kxk_backward_g16): grad_guidance is dt (what cspn2d_backward_kxk_norm returns for a
    dt guidance), grad_blur is float32 and is ROUNDED ONCE TO dt as it enters the GEMMs (what a 16-bit convolution's backward would have received); dL/dx comes
    back in dt (rounded once), the weight gradients in float32 (the accumulators) -- or in dt, the float32 ones .to(dt), for weights that are dt themselves.
    guidance_dtype=torch.float32 with a dt x and the 8-plane weights (cspn_guidance_head_backward_g16): grad_guidance AND grad_blur are float32 (what
    cspn2d_backward returns) and are both rounded once to dt as they enter the GEMMs; the outputs as above.  Any other use of guidance_dtype: ValueError."""
    P = _head_planes(x, weight_guidance, weight_blur, grad_guidance, grad_blur)
    path = _head_path(x, weight_guidance, weight_blur, P, guidance_dtype)
    xx, wg, wb = _head_prep(path, x, weight_guidance, weight_blur, P)
    gg, gb = _head_prep_grads(path, xx, wb, P, grad_guidance, grad_blur)
    dx, dwg, dwb = _heads_backward(path, xx, _f32(wg), _f32(wb), gg, gb, need_x, need_w)
    return dx, dwg.to(wg.dtype) if dwg is not None else None, dwb.to(wb.dtype) if dwb is not None else None


class _GuidanceHeadsFunction(torch.autograd.Function):
    """both heads of one path of _HEAD_PATHS (ctx.path) and their backward.  wg / wb: float32 master weights, or on the x16 paths weights of x's dtype (widened
    exactly; their gradients are the float32 ones .to(dtype))"""

    @staticmethod
    def forward(ctx, path, x, wg, wb, H, W):
        ctx.path = path
        ctx.save_for_backward(x, wg, wb)
        return _heads_forward(path, x, _f32(wg), _f32(wb), H, W)

    @staticmethod
    def backward(ctx, grad_g, grad_b):
        path = ctx.path
        x, wg, wb = ctx.saved_tensors
        need_x, need_wg, need_wb = ctx.needs_input_grad[1], ctx.needs_input_grad[2], wb is not None and ctx.needs_input_grad[3]
        if grad_g is None:   # an output the loss does not use: zeros in the dtype the entry point takes
            grad_g = torch.zeros(x.shape[0], wg.shape[0], *(grad_b.shape[2:] if grad_b is not None else (2 * x.shape[2], 2 * x.shape[3])),
                                 dtype=x.dtype if path.guidance16 else torch.float32, device=x.device)
        if wb is not None and grad_b is None:
            grad_b = torch.zeros(x.shape[0], 1, grad_g.shape[2], grad_g.shape[3], dtype=torch.float32, device=x.device)
        dx, dwg, dwb = _heads_backward(path, x, _f32(wg), _f32(wb), (grad_g if path.guidance16 else grad_g.float()).contiguous(),
                                       grad_b.float().contiguous() if wb is not None else None, need_x, need_wg or need_wb)
        return None, dx, dwg.to(wg.dtype) if need_wg else None, dwb.to(wb.dtype) if need_wb else None, None, None


def _requires_grad(*tensors):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def guidance_heads(x, weight_guidance, weight_blur=None, oheight=0, owidth=0, norm_type=None, guidance_dtype=None):
    """The producer of the propagation's inputs: what the reference computes as
        guidance = self.gud_up_proj_layer6(x); x = self.gud_up_proj_layer5(x)          (torch_resnet_cspn_nyu.py:372-373)
    with both heads Simple_Gudi_UpConv_Block_Last_Layer (:187-206: Unpool + narrow to (oheight, owidth) + bias-free 3x3 conv), in ONE kernel that never
    multiplies the structurally zero taps.  x [B,C,h,w]; weight_guidance = layer6.conv1.weight [8,C,3,3]; weight_blur = layer5.conv1.weight [1,C,3,3] or None.
    norm_type None: -> (guidance [B,8,H,W], blur [B,1,H,W] | None), bit-compatible inputs of Affinity_Propagate(..., norm_type)(guidance, blur, sparse);
    differentiable w.r.t. x and both weights (cspn_guidance_head_backward_f32: the gradients torch autograd computes through the reference layers).
    norm_type '8sum' | '8sum_abs': the guidance comes back normalised -- gate_wb of affinity_normalization (cspn.py:85-144) -- for
    cspn2d_forward(gate_wb, blur, sparse, n_iter, 'prenorm') / cspn_amd.propagate_prenorm.  With grad off the normalisation runs fused behind the conv
    (one kernel); with grad on and any input requiring grad, the raw heads (_GuidanceHeadsFunction) then the differentiable cspn2d_normalize: autograd chains
    cspn2d_normalize_backward_f32 into cspn_guidance_head_backward_f32, so dL/dgate_wb from propagate_prenorm reaches x and both weights.
    weight_guidance [24 | 48, C, 3, 3] (Simple_Gudi_UpConv_Block_Last_Layer(C, 24 | 48, ...): prop_kernel 5 / 7): -> (guidance [B, 24 | 48, H, W], blur), the
    inputs of Affinity_PropagateKxK(prop_time, 5 | 7, norm_type)(guidance, blur, sparse); cspn_guidance_head_kxk_f32, three GEMMs on the matrix cores forward
    and backward (one autograd Function); raw only: a norm_type raises ValueError, the K x K contract normalises in its own fold.
    With the 24- / 48-plane weights x may be float16 / bfloat16 = dt, as a backbone under torch.autocast emits it (cspn_guidance_head_kxk_g16): the weights are
    the float32 master weights (rounded once to dt in the engine) or dt weights (passed as .float(), exact; their gradients come back .to(dt)); products of two
    dt values accumulate in float32 on the matrix cores; guidance comes back in dt (the accumulator rounded once) -- what Affinity_PropagateKxK takes as it is
    --, blur in float32 (the accumulator: the engine's value tensors are float32); dL/dx comes back in dt.  A dt that differs between x and 16-bit weights
    raises TypeError, and so does a 16-bit x with the 8-plane weights: the 3 x 3 head is float32 only -- by default.
    guidance_dtype=torch.float32 with a dt x and the 8-plane weights (cspn_guidance_head_g16; what cspn_amd.GuidanceHeads calls): the same contract for the
    weights and the sums, and guidance AND blur come back in float32, the unrounded accumulators -- what Affinity_Propagate(prop_time, 3, norm_type) takes as it
    is, with no x.float() before the head and no widening pass behind it; dL/dx comes back in dt.  Raw only.  Any other use of guidance_dtype (24 / 48 planes, a
    float32 x, another dtype, a norm_type) raises ValueError."""
    P = _head_planes(x, weight_guidance, weight_blur)
    path = _head_path(x, weight_guidance, weight_blur, P, guidance_dtype, norm_type)
    if norm_type is not None and _requires_grad(x, weight_guidance, weight_blur):
        return _guidance_heads_normalised(x, weight_guidance, weight_blur, oheight, owidth, norm_type)
    xx, wg, wb = _head_prep(path, x, weight_guidance, weight_blur, P)
    H, W = _head_out_size(xx, oheight, owidth)
    if norm_type not in (None, "8sum", "8sum_abs"):
        raise ValueError("norm_type must be None (raw guidance), '8sum' or '8sum_abs' (gate_wb)")
    if norm_type is None and _requires_grad(xx, wg, wb):
        return _GuidanceHeadsFunction.apply(path, xx, wg, wb, H, W)
    return _heads_forward(path, xx, _f32(wg), _f32(wb), H, W, norm_type)


def _guidance_heads_normalised(x, weight_guidance, weight_blur, oheight, owidth, norm_type):
    """guidance_heads with norm_type under autograd (the float32 8-plane path): the raw heads, then cspn2d_normalize (both differentiable).  Forward traffic: the
    raw guidance written (32 B/pixel) and normalised (36 B read + 32 B written) -- the fused mode writes 32 B and normalises in place in the same 32 + 32 B."""
    if norm_type not in ("8sum", "8sum_abs"):
        raise ValueError("norm_type must be None (raw guidance), '8sum' or '8sum_abs' (gate_wb)")
    path = _HEAD_PATHS["f32"]
    xx, wg, wb = _head_prep(path, x, weight_guidance, weight_blur, 8)
    g, b = _GuidanceHeadsFunction.apply(path, xx, wg, wb, *_head_out_size(xx, oheight, owidth))
    return cspn2d_normalize(g, norm_type), b


class GuidanceHeads(nn.Module):
    """Both Simple_Gudi_UpConv_Block_Last_Layer heads of the reference model (torch_resnet_cspn_nyu.py:187-206, :318-319: gud_up_proj_layer6 C -> K*K-1 and
    gud_up_proj_layer5 C -> 1) as one module that owns the two bias-free 3x3 weights: forward(x) -> (guidance, blur), the inputs of
    Affinity_Propagate(prop_time, 3, ...) / Affinity_PropagateKxK(prop_time, 5 | 7, ...).  weight_guidance [K*K-1, C, 3, 3] and weight_blur [1, C, 3, 3] (absent
    with blur=False) are float32 parameters initialised as nn.Conv2d initialises; the path is chosen by the dtype of x and the plane count:
        float32 x                      guidance_heads as it is                 -> float32 guidance, float32 blur
        float16 / bfloat16 x, K 5 | 7  the 16-bit 24- / 48-plane heads         -> guidance in x's dtype, float32 blur
        float16 / bfloat16 x, K 3      guidance_heads(guidance_dtype=float32)  -> float32 guidance, float32 blur (no x.float(), no widening pass)
    so a backbone under torch.autocast hands its feature map over as it is.  Differentiable w.r.t. x and both weights, one autograd Function per path."""

    def __init__(self, in_channels, prop_kernel=3, oheight=0, owidth=0, blur=True):
        super(GuidanceHeads, self).__init__()
        if prop_kernel not in (3, 5, 7):
            raise ValueError("prop_kernel must be 3, 5 or 7, got %r" % (prop_kernel,))
        self.in_channels, self.prop_kernel = int(in_channels), int(prop_kernel)
        self.oheight, self.owidth = int(oheight), int(owidth)
        # (what nn.Conv2d(C, planes, 3, bias=False).reset_parameters() does)
        self.weight_guidance = nn.Parameter(torch.empty(prop_kernel * prop_kernel - 1, self.in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight_guidance, a=5 ** 0.5)
        if blur:
            self.weight_blur = nn.Parameter(torch.empty(1, self.in_channels, 3, 3))
            nn.init.kaiming_uniform_(self.weight_blur, a=5 ** 0.5)
        else:
            self.register_parameter("weight_blur", None)

    @classmethod
    def from_reference(cls, layer_guidance, layer_blur=None):
        """from the reference model's two layers (anything with .conv1.weight, .oheight and .owidth): copies of their weights and their output size"""
        wg = layer_guidance.conv1.weight
        planes, C = int(wg.shape[0]), int(wg.shape[1])
        if planes not in _PLANES_TO_K or tuple(wg.shape[2:]) != (3, 3):
            raise ValueError("layer_guidance.conv1.weight must be [8 | 24 | 48, C, 3, 3], got %s" % (tuple(wg.shape),))
        if layer_blur is not None:
            if tuple(layer_blur.conv1.weight.shape) != (1, C, 3, 3):
                raise ValueError("layer_blur.conv1.weight must be [1, %d, 3, 3], got %s" % (C, tuple(layer_blur.conv1.weight.shape)))
            if (int(layer_blur.oheight), int(layer_blur.owidth)) != (int(layer_guidance.oheight), int(layer_guidance.owidth)):
                raise ValueError("the two layers narrow to different output sizes")
        m = cls(C, _PLANES_TO_K[planes], layer_guidance.oheight, layer_guidance.owidth, blur=layer_blur is not None)
        with torch.no_grad():
            m.weight_guidance.copy_(wg)
            if layer_blur is not None:
                m.weight_blur.copy_(layer_blur.conv1.weight)
        return m.to(wg.device)

    def forward(self, x):
        f32_guidance = isinstance(x, torch.Tensor) and x.dtype in _GATE16 and self.prop_kernel == 3
        return guidance_heads(x, self.weight_guidance, self.weight_blur, self.oheight, self.owidth,
                              guidance_dtype=torch.float32 if f32_guidance else None)

    def extra_repr(self):
        return "in_channels=%d, prop_kernel=%d, oheight=%d, owidth=%d, blur=%s" % (self.in_channels, self.prop_kernel, self.oheight, self.owidth,
                                                                                   self.weight_blur is not None)
