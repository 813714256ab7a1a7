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
import torch
import torch.nn as nn

from . import _lib
from .functional import _GATE16, _prep, _workspace, cspn2d_normalize

_KEYS = ['MSE', 'RMSE', 'ABS_REL', 'LG10', 'MAE', 'DELTA1.02', 'DELTA1.05', 'DELTA1.10', 'DELTA1.25', 'DELTA1.25^2',
         'DELTA1.25^3']


def _metrics(gt, pred):
    """-> device float32[12]: n_valid, then the 11 values of _KEYS"""
    lib = _lib.load()
    g = _prep(gt, "gt_depth")
    p = _prep(pred, "pred_depth", tuple(g.shape))
    out = torch.empty(12, dtype=torch.float32, device=g.device)
    n = g.numel()
    with torch.cuda.device(g.device):
        wsb = lib.cspn_metrics_workspace_bytes(n)
        ws = _workspace(wsb, g.device)
        rc = lib.cspn_metrics_f32(g.data_ptr(), p.data_ptr(), n, out.data_ptr(), ws.data_ptr(), wsb,
                                  torch.cuda.current_stream(g.device).cuda_stream)
    _lib.check(rc, "cspn_metrics_f32")
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
        lib = _lib.load()
        p, l = pred.contiguous(), label.contiguous()
        gp = torch.empty_like(p)
        gs = grad.reshape(1).to(torch.float32).contiguous()
        with torch.cuda.device(p.device):
            rc = lib.cspn_l1_backward_f32(p.data_ptr(), l.data_ptr(), stats.data_ptr(), gs.data_ptr(), gp.data_ptr(), p.numel(),
                                          torch.cuda.current_stream(p.device).cuda_stream)
        _lib.check(rc, "cspn_l1_backward_f32")
        return gp.view_as(pred), None


class Wighted_L1_Loss(nn.Module):
    """reference loss.py:12-23 (spelling as there)"""

    def forward(self, pred, label):
        return _L1.apply(pred, label)


class _Unpool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stride):
        lib = _lib.load()
        xc = _prep(x, "x")
        N, C, H, W = xc.shape
        out = torch.empty(N, C, H * stride, W * stride, dtype=torch.float32, device=xc.device)
        ctx.shape, ctx.stride = (N, C, H, W), stride
        with torch.cuda.device(xc.device):
            rc = lib.cspn_unpool_f32(xc.data_ptr(), out.data_ptr(), N * C, H, W, stride,
                                     torch.cuda.current_stream(xc.device).cuda_stream)
        _lib.check(rc, "cspn_unpool_f32")
        return out

    @staticmethod
    def backward(ctx, go):
        lib = _lib.load()
        N, C, H, W = ctx.shape
        g = go.contiguous()
        gx = torch.empty(N, C, H, W, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            rc = lib.cspn_unpool_backward_f32(g.data_ptr(), gx.data_ptr(), N * C, H, W, ctx.stride,
                                              torch.cuda.current_stream(g.device).cuda_stream)
        _lib.check(rc, "cspn_unpool_backward_f32")
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
    lib = _lib.load()
    d = _prep(depth_image, "depth_image")
    if d.dim() < 2:
        raise ValueError("depth_image must be [..., H, W]")
    hw = d.shape[-1] * d.shape[-2]
    n_images = d.numel() // hw if hw else 0
    out = torch.empty_like(d)
    if d.numel() == 0:
        return out
    m = {"nyu": 0, "kitti": 1}[mode]
    with torch.cuda.device(d.device):
        wsb = lib.cspn_sparse_sample_workspace_bytes(n_images)
        ws = _workspace(wsb, d.device)
        rc = lib.cspn_sparse_sample_f32(d.data_ptr(), out.data_ptr(), n_images, hw, int(n_sample), m, int(seed) & (2 ** 64 - 1),
                                        ws.data_ptr(), wsb, torch.cuda.current_stream(d.device).cuda_stream)
    _lib.check(rc, "cspn_sparse_sample_f32")
    return out


_PLANES_TO_K = {8: 3, 24: 5, 48: 7}


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


def _heads_kxk_forward(xx, wg, wb, H, W):
    """cspn_guidance_head_kxk_f32: the 24- / 48-plane guidance head and the blur head, raw, on the matrix cores.  xx float16 / bfloat16:
    cspn_guidance_head_kxk_g16, float32 weights (rounded once to xx's dtype in the engine) -> guidance in xx's dtype, blur float32"""
    B, C, h, w = xx.shape
    P = int(wg.shape[0])
    K = _PLANES_TO_K[P]
    dt = _GATE16.get(xx.dtype)
    g = torch.empty(B, P, H, W, dtype=xx.dtype, device=xx.device)
    b = torch.empty(B, 1, H, W, dtype=torch.float32, device=xx.device) if wb is not None else None
    name = "cspn_guidance_head_kxk_f32" if dt is None else "cspn_guidance_head_kxk_g16"
    with torch.cuda.device(xx.device):
        wsb = _lib.late_symbol("cspn_guidance_head_kxk%s_workspace_bytes" % ("" if dt is None else "_g16"))(B, C, h, w, K)
        ws = _workspace(wsb, xx.device)
        rc = _lib.late_symbol(name)(xx.data_ptr(), *(() if dt is None else (dt,)), wg.data_ptr(), wb.data_ptr() if wb is not None else None, g.data_ptr(),
                                    b.data_ptr() if b is not None else None, B, C, h, w, H, W, K, ws.data_ptr(), wsb,
                                    torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, name)
    return g, b


def _heads_kxk_backward(xx, wg, wb, gg, gb, need_x, need_w):
    """cspn_guidance_head_kxk_backward_f32.  xx float16 / bfloat16: cspn_guidance_head_kxk_backward_g16, dL/dguidance in xx's dtype, dL/dblur float32
    (rounded once to xx's dtype as it enters the GEMMs) -> dL/dx in xx's dtype, the weight gradients float32"""
    B, C, h, w = xx.shape
    K = _PLANES_TO_K[int(wg.shape[0])]
    H, W = int(gg.shape[2]), int(gg.shape[3])
    dt = _GATE16.get(xx.dtype)
    dx = torch.empty_like(xx) if need_x else None
    dwg = torch.empty_like(wg) if need_w else None
    dwb = torch.empty_like(wb) if (need_w and wb is not None) else None
    name = "cspn_guidance_head_kxk_backward_%s" % ("f32" if dt is None else "g16")
    with torch.cuda.device(xx.device):
        wsb = _lib.late_symbol("cspn_guidance_head_kxk_backward%s_workspace_bytes" % ("" if dt is None else "_g16"))(B, C, h, w, K)
        ws = _workspace(wsb, xx.device)
        rc = _lib.late_symbol(name)(
            xx.data_ptr(), *(() if dt is None else (dt,)), wg.data_ptr(), wb.data_ptr() if wb is not None else None, gg.data_ptr(),
            gb.data_ptr() if gb is not None else None, dx.data_ptr() if dx is not None else None, dwg.data_ptr() if dwg is not None else None,
            dwb.data_ptr() if dwb is not None else None, B, C, h, w, H, W, K, ws.data_ptr(), wsb, torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, name)
    return dx, dwg, dwb


def _head_dtype16(x, weight_guidance, weight_blur, P):
    """-> the 16-bit dtype of x (float16 / bfloat16: the heads of cspn_guidance_head_kxk_g16), or None for every other x.  Raised before any device check:
    TypeError for a 16-bit x with 8-plane weights, and for 16-bit weights whose dtype differs from x's"""
    if x.dtype not in _GATE16:
        return None
    if P == 8:
        raise TypeError("the 3 x 3 guidance head (weight_guidance [8, C, 3, 3]) is float32 only: its ring has no 16-bit consumer; x is %s -- pass x.float(), "
                        "or use the 24- / 48-plane heads of prop_kernel 5 / 7 (guidance_dtype=torch.float32, or cspn_amd.GuidanceHeads, runs the 16-bit head that emits "
                        "float32 guidance)" % (x.dtype,))
    for t, name in ((weight_guidance, "weight_guidance"), (weight_blur, "weight_blur")):
        if isinstance(t, torch.Tensor) and t.dtype in _GATE16 and t.dtype != x.dtype:
            raise TypeError("x is %s but %s is %s: 16-bit weights must have the dtype of x (or be the float32 master weights)" % (x.dtype, name, t.dtype))
    return x.dtype


def _head_dtype16_f32(x, weight_guidance, weight_blur, P, guidance_dtype, norm_type=None):
    """guidance_dtype given -> the 16-bit dtype of x: the 8-plane head on a float16 / bfloat16 x that emits float32 guidance (cspn_guidance_head_g16).  Raised
    before any device check: ValueError for every other combination, TypeError for 16-bit weights whose dtype differs from x's"""
    if guidance_dtype is not torch.float32:
        raise ValueError("guidance_dtype must be None or torch.float32, got %r" % (guidance_dtype,))
    if P != 8:
        raise ValueError("guidance_dtype=torch.float32 is the 8-plane head's (prop_kernel 3); the %d-plane head of prop_kernel %d returns its guidance in the "
                         "dtype of x" % (P, _PLANES_TO_K[P]))
    if x.dtype not in _GATE16:
        raise ValueError("guidance_dtype=torch.float32 is for a float16 / bfloat16 x; x is %s (a float32 x takes the default guidance_dtype=None)" % (x.dtype,))
    if norm_type is not None:
        raise ValueError("the 16-bit 8-plane head returns raw guidance only (norm_type=None): Affinity_Propagate(prop_time, 3, norm_type) normalises it")
    for t, name in ((weight_guidance, "weight_guidance"), (weight_blur, "weight_blur")):
        if isinstance(t, torch.Tensor) and t.dtype in _GATE16 and t.dtype != x.dtype:
            raise TypeError("x is %s but %s is %s: 16-bit weights must have the dtype of x (or be the float32 master weights)" % (x.dtype, name, t.dtype))
    return x.dtype


def _prep16(t, name, dt, shape=None):
    """a 16-bit tensor of the heads (x, dL/dguidance): on the GPU, of dtype dt, contiguous"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.CspnError("cspn_amd: %s is on %s; the engine is GPU-only (hand-written HIP for gfx950) and has no CPU path" % (name, t.device))
    if t.dtype != dt:
        raise TypeError("%s must be %s as x (got %s)" % (name, dt, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t.contiguous()


def _prep_w16(t, name, dt, shape):
    """a weight of the 16-bit heads: the float32 master weights, or dt weights widened with .float() (exact) -> float32"""
    if isinstance(t, torch.Tensor) and t.dtype == dt:
        t = t.float()
    return _prep(t, name, shape)


def _heads_forward(xx, wg, wb, H, W, norm):
    lib = _lib.load()
    B, C, h, w = xx.shape
    g = torch.empty(B, 8, H, W, dtype=torch.float32, device=xx.device)
    b = torch.empty(B, 1, H, W, dtype=torch.float32, device=xx.device) if wb is not None else None
    with torch.cuda.device(xx.device):
        wsb = lib.cspn_guidance_head_workspace_bytes(C)
        ws = _workspace(wsb, xx.device)
        rc = lib.cspn_guidance_head_f32(xx.data_ptr(), wg.data_ptr(), wb.data_ptr() if wb is not None else None, g.data_ptr(),
                                        b.data_ptr() if b is not None else None, B, C, h, w, H, W, norm, ws.data_ptr(), wsb,
                                        torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, "cspn_guidance_head_f32")
    return g, b


def _heads16_forward(xx, wg, wb, H, W):
    """cspn_guidance_head_g16: the 8-plane guidance head and the blur head, raw, on a float16 / bfloat16 xx; float32 weights (rounded once to xx's dtype in the
    engine) -> guidance and blur in float32, the unrounded accumulators"""
    B, C, h, w = xx.shape
    g = torch.empty(B, 8, H, W, dtype=torch.float32, device=xx.device)
    b = torch.empty(B, 1, H, W, dtype=torch.float32, device=xx.device) if wb is not None else None
    with torch.cuda.device(xx.device):
        wsb = _lib.symbol("cspn_guidance_head_g16_workspace_bytes")(B, C, h, w)
        ws = _workspace(wsb, xx.device)
        rc = _lib.symbol("cspn_guidance_head_g16")(xx.data_ptr(), _GATE16[xx.dtype], wg.data_ptr(), wb.data_ptr() if wb is not None else None, g.data_ptr(),
                                                   b.data_ptr() if b is not None else None, B, C, h, w, H, W, ws.data_ptr(), wsb,
                                                   torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, "cspn_guidance_head_g16")
    return g, b


def _heads16_backward(xx, wg, wb, gg, gb, need_x, need_w):
    """cspn_guidance_head_backward_g16: float32 dL/dguidance and dL/dblur (rounded once to xx's dtype as they enter the GEMMs) -> dL/dx in xx's dtype, the
    weight gradients float32"""
    B, C, h, w = xx.shape
    H, W = int(gg.shape[2]), int(gg.shape[3])
    dx = torch.empty_like(xx) if need_x else None
    dwg = torch.empty_like(wg) if need_w else None
    dwb = torch.empty_like(wb) if (need_w and wb is not None) else None
    with torch.cuda.device(xx.device):
        wsb = _lib.symbol("cspn_guidance_head_backward_g16_workspace_bytes")(B, C, h, w)
        ws = _workspace(wsb, xx.device)
        rc = _lib.symbol("cspn_guidance_head_backward_g16")(
            xx.data_ptr(), _GATE16[xx.dtype], wg.data_ptr(), wb.data_ptr() if wb is not None else None, gg.data_ptr(),
            gb.data_ptr() if gb is not None else None, dx.data_ptr() if dx is not None else None, dwg.data_ptr() if dwg is not None else None,
            dwb.data_ptr() if dwb is not None else None, B, C, h, w, H, W, ws.data_ptr(), wsb, torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, "cspn_guidance_head_backward_g16")
    return dx, dwg, dwb


def guidance_heads_backward(x, weight_guidance, weight_blur, grad_guidance, grad_blur, need_x=True, need_w=True, guidance_dtype=None):
    """cspn_guidance_head_backward_f32: (dL/dx, dL/dweight_guidance, dL/dweight_blur) of the RAW heads -- what torch autograd computes through the two reference
    layers (torch_resnet_cspn_nyu.py:187-206) -- from dL/dguidance [B,8,H,W] and dL/dblur [B,1,H,W] (None without a blur head); skipped outputs are None.
    weight_guidance [24 | 48, C, 3, 3] with dL/dguidance [B, 24 | 48, H, W]: cspn_guidance_head_kxk_backward_f32, the heads of prop_kernel 5 / 7.
    With those weights x may be float16 / bfloat16 = dt (cspn_guidance_head_kxk_backward_g16): grad_guidance is dt (what cspn2d_backward_kxk_norm returns for a
    dt guidance), grad_blur is float32 and is ROUNDED ONCE TO dt as it enters the GEMMs (what a 16-bit convolution's backward would have received); dL/dx comes
    back in dt (rounded once), the weight gradients in float32 (the accumulators) -- or in dt, the float32 ones .to(dt), for weights that are dt themselves.
    guidance_dtype=torch.float32 with a dt x and the 8-plane weights (cspn_guidance_head_backward_g16): grad_guidance AND grad_blur are float32 (what
    cspn2d_backward returns) and are both rounded once to dt as they enter the GEMMs; the outputs as above.  Any other use of guidance_dtype: ValueError."""
    lib = _lib.load()
    P = _head_planes(x, weight_guidance, weight_blur, grad_guidance, grad_blur)
    if guidance_dtype is not None:
        dt = _head_dtype16_f32(x, weight_guidance, weight_blur, P, guidance_dtype)
        xx = _prep16(x, "x", dt)
        B, C, h, w = xx.shape
        wg = _prep_w16(weight_guidance, "weight_guidance", dt, (8, C, 3, 3))
        wb = _prep_w16(weight_blur, "weight_blur", dt, (1, C, 3, 3)) if weight_blur is not None else None
        if not isinstance(grad_guidance, torch.Tensor) or grad_guidance.dim() != 4:
            raise ValueError("grad_guidance must be [B,8,H,W]")
        H, W = int(grad_guidance.shape[2]), int(grad_guidance.shape[3])
        gg = _prep(grad_guidance, "grad_guidance", (B, 8, H, W))
        gb = _prep(grad_blur, "grad_blur", (B, 1, H, W)) if wb is not None else None
        dx, dwg, dwb = _heads16_backward(xx, wg, wb, gg, gb, need_x, need_w)
        if dwg is not None and weight_guidance.dtype == dt:
            dwg = dwg.to(dt)
        if dwb is not None and weight_blur.dtype == dt:
            dwb = dwb.to(dt)
        return dx, dwg, dwb
    dt = _head_dtype16(x, weight_guidance, weight_blur, P)
    if dt is not None:
        xx = _prep16(x, "x", dt)
        B, C, h, w = xx.shape
        wg = _prep_w16(weight_guidance, "weight_guidance", dt, (P, C, 3, 3))
        wb = _prep_w16(weight_blur, "weight_blur", dt, (1, C, 3, 3)) if weight_blur is not None else None
        if not isinstance(grad_guidance, torch.Tensor) or grad_guidance.dim() != 4:
            raise ValueError("grad_guidance must be [B,%d,H,W]" % P)
        H, W = int(grad_guidance.shape[2]), int(grad_guidance.shape[3])
        gg = _prep16(grad_guidance, "grad_guidance", dt, (B, P, H, W))
        gb = _prep(grad_blur, "grad_blur", (B, 1, H, W)) if wb is not None else None
        dx, dwg, dwb = _heads_kxk_backward(xx, wg, wb, gg, gb, need_x, need_w)
        if dwg is not None and weight_guidance.dtype == dt:
            dwg = dwg.to(dt)
        if dwb is not None and weight_blur.dtype == dt:
            dwb = dwb.to(dt)
        return dx, dwg, dwb
    xx = _prep(x, "x")
    B, C, h, w = xx.shape
    wg = _prep(weight_guidance, "weight_guidance", (P, C, 3, 3))
    wb = _prep(weight_blur, "weight_blur", (1, C, 3, 3)) if weight_blur is not None else None
    if not isinstance(grad_guidance, torch.Tensor) or grad_guidance.dim() != 4:
        raise ValueError("grad_guidance must be [B,%d,H,W]" % P)
    H, W = int(grad_guidance.shape[2]), int(grad_guidance.shape[3])
    gg = _prep(grad_guidance, "grad_guidance", (B, P, H, W))
    gb = _prep(grad_blur, "grad_blur", (B, 1, H, W)) if wb is not None else None
    if P != 8:
        return _heads_kxk_backward(xx, wg, wb, gg, gb, need_x, need_w)
    dx = torch.empty_like(xx) if need_x else None
    dwg = torch.empty_like(wg) if need_w else None
    dwb = torch.empty_like(wb) if (need_w and wb is not None) else None
    with torch.cuda.device(xx.device):
        wsb = lib.cspn_guidance_head_backward_workspace_bytes(B, C, h, w)
        ws = _workspace(wsb, xx.device)
        rc = lib.cspn_guidance_head_backward_f32(xx.data_ptr(), wg.data_ptr(), wb.data_ptr() if wb is not None else None, gg.data_ptr(),
                                                 gb.data_ptr() if gb is not None else None, dx.data_ptr() if dx is not None else None,
                                                 dwg.data_ptr() if dwg is not None else None, dwb.data_ptr() if dwb is not None else None,
                                                 B, C, h, w, H, W, ws.data_ptr(), wsb, torch.cuda.current_stream(xx.device).cuda_stream)
    _lib.check(rc, "cspn_guidance_head_backward_f32")
    return dx, dwg, dwb


class _GuidanceHeadsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wg, wb, H, W):
        ctx.save_for_backward(x, wg, wb)
        g, b = _heads_forward(x, wg, wb, H, W, _lib.NORM_TYPES["none"])
        return g, b

    @staticmethod
    def backward(ctx, grad_g, grad_b):
        x, wg, wb = ctx.saved_tensors
        if grad_g is None:
            grad_g = torch.zeros(x.shape[0], 8, *((grad_b.shape[2:]) if grad_b is not None else (2 * x.shape[2], 2 * x.shape[3])), device=x.device)
        if wb is not None and grad_b is None:
            grad_b = torch.zeros(x.shape[0], 1, grad_g.shape[2], grad_g.shape[3], device=x.device)
        dx, dwg, dwb = guidance_heads_backward(x, wg, wb, grad_g.contiguous(), grad_b.contiguous() if grad_b is not None else None,
                                               need_x=ctx.needs_input_grad[0], need_w=ctx.needs_input_grad[1] or (wb is not None and ctx.needs_input_grad[2]))
        return dx, dwg if ctx.needs_input_grad[1] else None, dwb if (wb is not None and ctx.needs_input_grad[2]) else None, None, None


class _GuidanceHeadsKxKFunction(torch.autograd.Function):
    """the 24- / 48-plane guidance head + the blur head: cspn_guidance_head_kxk_f32 and its backward"""

    @staticmethod
    def forward(ctx, x, wg, wb, H, W):
        ctx.save_for_backward(x, wg, wb)
        return _heads_kxk_forward(x, wg, wb, H, W)

    @staticmethod
    def backward(ctx, grad_g, grad_b):
        x, wg, wb = ctx.saved_tensors
        if grad_g is None:
            grad_g = torch.zeros(x.shape[0], wg.shape[0], grad_b.shape[2], grad_b.shape[3], device=x.device)
        if wb is not None and grad_b is None:
            grad_b = torch.zeros(x.shape[0], 1, grad_g.shape[2], grad_g.shape[3], device=x.device)
        need_w = ctx.needs_input_grad[1] or (wb is not None and ctx.needs_input_grad[2])
        dx, dwg, dwb = _heads_kxk_backward(x, wg, wb, grad_g.contiguous(), grad_b.contiguous() if wb is not None else None, ctx.needs_input_grad[0], need_w)
        return dx, dwg if ctx.needs_input_grad[1] else None, dwb if (wb is not None and ctx.needs_input_grad[2]) else None, None, None


class _GuidanceHeadsKxK16Function(torch.autograd.Function):
    """the 24- / 48-plane guidance head + the blur head on a float16 / bfloat16 x: cspn_guidance_head_kxk_g16 and its backward.  wg / wb: float32 master
    weights, or weights of x's dtype (widened exactly; their gradients are the float32 ones .to(dtype))"""

    @staticmethod
    def forward(ctx, x, wg, wb, H, W):
        ctx.save_for_backward(x, wg, wb)
        return _heads_kxk_forward(x, wg.float(), wb.float() if wb is not None else None, H, W)

    @staticmethod
    def backward(ctx, grad_g, grad_b):
        x, wg, wb = ctx.saved_tensors
        if grad_g is None:
            grad_g = torch.zeros(x.shape[0], wg.shape[0], grad_b.shape[2], grad_b.shape[3], dtype=x.dtype, device=x.device)
        if wb is not None and grad_b is None:
            grad_b = torch.zeros(x.shape[0], 1, grad_g.shape[2], grad_g.shape[3], dtype=torch.float32, device=x.device)
        need_w = ctx.needs_input_grad[1] or (wb is not None and ctx.needs_input_grad[2])
        dx, dwg, dwb = _heads_kxk_backward(x, wg.float(), wb.float() if wb is not None else None, grad_g.contiguous(),
                                             grad_b.float().contiguous() if wb is not None else None, ctx.needs_input_grad[0], need_w)
        return (dx, dwg.to(wg.dtype) if ctx.needs_input_grad[1] else None,
                dwb.to(wb.dtype) if (wb is not None and ctx.needs_input_grad[2]) else None, None, None)


class _GuidanceHeads16Function(torch.autograd.Function):
    """the 8-plane guidance head + the blur head on a float16 / bfloat16 x, float32 guidance and blur: cspn_guidance_head_g16 and its backward.  wg / wb:
    float32 master weights, or weights of x's dtype (widened exactly; their gradients are the float32 ones .to(dtype))"""

    @staticmethod
    def forward(ctx, x, wg, wb, H, W):
        ctx.save_for_backward(x, wg, wb)
        return _heads16_forward(x, wg.float(), wb.float() if wb is not None else None, H, W)

    @staticmethod
    def backward(ctx, grad_g, grad_b):
        x, wg, wb = ctx.saved_tensors
        if grad_g is None:
            grad_g = torch.zeros(x.shape[0], 8, grad_b.shape[2], grad_b.shape[3], dtype=torch.float32, device=x.device)
        if wb is not None and grad_b is None:
            grad_b = torch.zeros(x.shape[0], 1, grad_g.shape[2], grad_g.shape[3], dtype=torch.float32, device=x.device)
        need_w = ctx.needs_input_grad[1] or (wb is not None and ctx.needs_input_grad[2])
        dx, dwg, dwb = _heads16_backward(x, wg.float(), wb.float() if wb is not None else None, grad_g.float().contiguous(),
                                         grad_b.float().contiguous() if wb is not None else None, ctx.needs_input_grad[0], need_w)
        return (dx, dwg.to(wg.dtype) if ctx.needs_input_grad[1] else None,
                dwb.to(wb.dtype) if (wb is not None and ctx.needs_input_grad[2]) else None, None, None)


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
    if guidance_dtype is not None:
        dt = _head_dtype16_f32(x, weight_guidance, weight_blur, P, guidance_dtype, norm_type)
        xx = _prep16(x, "x", dt)
        B, C, h, w = xx.shape
        H, W = (int(oheight), int(owidth)) if (oheight and owidth) else (2 * h, 2 * w)
        for t, name, shape in ((weight_guidance, "weight_guidance", (8, C, 3, 3)), (weight_blur, "weight_blur", (1, C, 3, 3))):
            if t is not None and t.dtype == dt:
                _prep16(t, name, dt, shape)
            elif t is not None:
                _prep(t, name, shape)
        wg = weight_guidance.contiguous()
        wb = weight_blur.contiguous() if weight_blur is not None else None
        if torch.is_grad_enabled() and (xx.requires_grad or wg.requires_grad or (wb is not None and wb.requires_grad)):
            return _GuidanceHeads16Function.apply(xx, wg, wb, H, W)
        return _heads16_forward(xx, wg.float(), wb.float() if wb is not None else None, H, W)
    dt = _head_dtype16(x, weight_guidance, weight_blur, P)
    if P != 8:
        if norm_type is not None:
            raise ValueError("the %d-plane guidance head returns raw guidance only (norm_type=None): Affinity_PropagateKxK(prop_time, %d, norm_type) "
                             "normalises it" % (P, _PLANES_TO_K[P]))
        if dt is not None:
            xx = _prep16(x, "x", dt)
            B, C, h, w = xx.shape
            H, W = (int(oheight), int(owidth)) if (oheight and owidth) else (2 * h, 2 * w)
            for t, name, shape in ((weight_guidance, "weight_guidance", (P, C, 3, 3)), (weight_blur, "weight_blur", (1, C, 3, 3))):
                if t is not None and t.dtype == dt:
                    _prep16(t, name, dt, shape)
                elif t is not None:
                    _prep(t, name, shape)
            wg = weight_guidance.contiguous()
            wb = weight_blur.contiguous() if weight_blur is not None else None
            if torch.is_grad_enabled() and (xx.requires_grad or wg.requires_grad or (wb is not None and wb.requires_grad)):
                return _GuidanceHeadsKxK16Function.apply(xx, wg, wb, H, W)
            return _heads_kxk_forward(xx, wg.float(), wb.float() if wb is not None else None, H, W)
        xx = _prep(x, "x")
        B, C, h, w = xx.shape
        wg = _prep(weight_guidance, "weight_guidance", (P, C, 3, 3))
        wb = _prep(weight_blur, "weight_blur", (1, C, 3, 3)) if weight_blur is not None else None
        H, W = (int(oheight), int(owidth)) if (oheight and owidth) else (2 * h, 2 * w)
        if torch.is_grad_enabled() and (xx.requires_grad or wg.requires_grad or (wb is not None and wb.requires_grad)):
            return _GuidanceHeadsKxKFunction.apply(xx, wg, wb, H, W)
        return _heads_kxk_forward(xx, wg, wb, H, W)
    if norm_type is not None and torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, weight_guidance, weight_blur)):
        return _guidance_heads_normalised(x, weight_guidance, weight_blur, oheight, owidth, norm_type)
    xx = _prep(x, "x")
    B, C, h, w = xx.shape
    wg = _prep(weight_guidance, "weight_guidance", (8, C, 3, 3))
    wb = _prep(weight_blur, "weight_blur", (1, C, 3, 3)) if weight_blur is not None else None
    H, W = (int(oheight), int(owidth)) if (oheight and owidth) else (2 * h, 2 * w)
    if norm_type not in (None, "8sum", "8sum_abs"):
        raise ValueError("norm_type must be None (raw guidance), '8sum' or '8sum_abs' (gate_wb)")
    if norm_type is None and torch.is_grad_enabled() and (xx.requires_grad or wg.requires_grad or (wb is not None and wb.requires_grad)):
        return _GuidanceHeadsFunction.apply(xx, wg, wb, H, W)
    return _heads_forward(xx, wg, wb, H, W, _lib.NORM_TYPES["none" if norm_type is None else norm_type])


def _guidance_heads_normalised(x, weight_guidance, weight_blur, oheight, owidth, norm_type):
    """guidance_heads with norm_type under autograd: the raw heads, then cspn2d_normalize (both differentiable).  Forward traffic: the raw guidance
    written (32 B/pixel) and normalised (36 B read + 32 B written) -- the fused mode writes 32 B and normalises in place in the same 32 + 32 B."""
    if norm_type not in ("8sum", "8sum_abs"):
        raise ValueError("norm_type must be None (raw guidance), '8sum' or '8sum_abs' (gate_wb)")
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise ValueError("x must be [B,C,h,w], got %s" % (tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__,))
    for t in (weight_guidance, weight_blur):
        if isinstance(t, torch.Tensor) and t.device != x.device:
            raise ValueError("all tensors must live on the same device")
    xx = _prep(x, "x")
    B, C, h, w = xx.shape
    wg = _prep(weight_guidance, "weight_guidance", (8, C, 3, 3))
    wb = _prep(weight_blur, "weight_blur", (1, C, 3, 3)) if weight_blur is not None else None
    H, W = (int(oheight), int(owidth)) if (oheight and owidth) else (2 * h, 2 * w)
    g, b = _GuidanceHeadsFunction.apply(xx, wg, wb, H, W)
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
