"""K x K propagation with per-step attention (the refinement module of DySPN and of the models built on it) on the engine's dynamic kernels.

Every contract of cspn_amd.cspn uses the same affinities on every step.  Here a small head emits, for every step and every distance ring of the
K x K neighbourhood, a per-pixel attention, plus one for the pixel itself; the affinities are re-weighted by it and re-normalised on each step.
The engine runs the iteration (cspn_amd.functional.cspn2d_forward_kxk_dyn / cspn2d_backward_kxk_dyn) without ever storing a modulated or
normalised gate: the guidance (K*K - 1 planes) and the attention (n (K//2 + 1) planes) are the only gate-sized tensors.  The activation of the
attention is a torch op over that small tensor, run once per call through autograd.

Neighbour k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre, its offset (K//2 - t, K//2 - l) as in Affinity_PropagateKxK,
its ring max(|dy|, |dx|).  Forward and backward are run-to-run bitwise (no atomics).  float32 only.

This module allocates nothing itself: every buffer comes from cspn_amd.functional."""
import torch
import torch.nn as nn

from . import functional as F

ATTENTIONS = (None, 'sigmoid', 'softmax')


class _DynamicFunction(torch.autograd.Function):
    """one cspn2d_forward_kxk_dyn call that keeps the pinned levels where dL/dguidance or dL/dattention will need them, one
    cspn2d_backward_kxk_dyn call"""

    @staticmethod
    def forward(ctx, guidance, att, x, sparse_depth, n_iter, kernel_size):
        ctx.n_iter, ctx.kernel_size = n_iter, kernel_size
        hist = None
        if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and n_iter >= 2:
            out, hist = F.cspn2d_forward_kxk_dyn(guidance, att, x, kernel_size, n_iter, sparse_depth, return_history=True)
        else:
            out = F.cspn2d_forward_kxk_dyn(guidance, att, x, kernel_size, n_iter, sparse_depth)
        ctx.save_for_backward(guidance, att, x, sparse_depth, hist)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        guidance, att, x, sparse_depth, hist = ctx.saved_tensors
        gg, ga, gx = F.cspn2d_backward_kxk_dyn(guidance, att, x, grad_out.contiguous(), ctx.kernel_size, ctx.n_iter, sparse_depth, hist,
                                               ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return gg, ga, gx, None, None, None


def dynamic_propagate(guidance, att, x, sparse_depth, n_iter, kernel_size=7):
    """differentiable cspn2d_forward_kxk_dyn on the attention as given, gradients to guidance, att and x (sparse_depth has none)"""
    if torch.is_grad_enabled() and (guidance.requires_grad or att.requires_grad or x.requires_grad):
        return _DynamicFunction.apply(guidance, att, x, sparse_depth, n_iter, kernel_size)
    return F.cspn2d_forward_kxk_dyn(guidance, att, x, kernel_size, n_iter, sparse_depth)


class Dynamic_Propagate(nn.Module):
    """forward(guidance [B,K*K-1,H,W] raw, attention [B,n (R+1),H,W], x [B,C,H,W], sparse_depth=None [B,1,H,W], n_iter=None) -> [B,C,H,W] after
    prop_time (or n_iter) steps, K = prop_kernel in {3, 5, 7}, R = K // 2, n the number of steps.  Attention channel t (R+1) + r: r = 0 belongs to the
    pixel itself at step t, r >= 1 to ring r (the neighbours with max(|dy|, |dx|) = r).  Per call:
        1. activation (a torch op, through autograd)  None: the attention as given;  'sigmoid': torch.sigmoid;  'softmax': over the R+1 planes of
           each step
        2. the engine's iteration, step t on the level Ht = sparse_depth where sparse_depth > 0 else H:
               w^_k = a[t, ring(k)] g_k     D = a[t, 0] + sum_k |w^_k|     H <- (1 - sum_k w^_k / D) Ht + sum_k (w^_k / D) Ht(p + off_k)
           H_0 = x; a neighbour outside the image contributes 0; the result of the last step is not pinned.
    THESE RULES ARE THE CONTRACT; they were written down from the published description of the method, not from a source: compare them with your
    model's before you port it.  The module has no parameter and no state.
    Gradients flow to guidance, attention (through the activation) and x.  float32 only: a float16 / bfloat16 / float64 tensor is a TypeError."""

    def __init__(self, prop_time, prop_kernel=7, attention=None):
        super(Dynamic_Propagate, self).__init__()
        if prop_kernel not in (3, 5, 7):
            raise ValueError("prop_kernel must be 3, 5 or 7, got %r" % (prop_kernel,))
        if attention not in ATTENTIONS:
            raise ValueError("attention must be one of %s, got %r" % (ATTENTIONS, attention))
        if isinstance(prop_time, bool) or int(prop_time) != prop_time or prop_time < 0:
            raise ValueError("prop_time must be an int >= 0, got %r" % (prop_time,))
        self.prop_time = int(prop_time)
        self.prop_kernel = prop_kernel
        self.attention = attention
        self.num_rings = prop_kernel // 2

    def activate(self, attention, n_iter):
        """step 1 above on attention [B, n_iter (R+1), H, W]"""
        if self.attention == 'sigmoid':
            return torch.sigmoid(attention)
        if self.attention == 'softmax':
            B, _, H, W = attention.shape
            return torch.softmax(attention.reshape(B, n_iter, self.num_rings + 1, H, W), 2).reshape(attention.shape)
        return attention

    def forward(self, guidance, attention, x, sparse_depth=None, n_iter=None):
        n = self.prop_time if n_iter is None else int(n_iter)
        if n < 0:
            raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
        KK, planes = self.prop_kernel ** 2 - 1, n * (self.num_rings + 1)
        for t, name, ch in ((guidance, "guidance", KK), (attention, "attention", planes)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != ch:
                raise ValueError("%s must be [B,%d,H,W], got %s" % (name, ch, tuple(getattr(t, "shape", ()))))
        for t, name in ((guidance, "guidance"), (attention, "attention"), (x, "x"), (sparse_depth, "sparse_depth")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
                raise TypeError("%s must be a float32 tensor (got %s)" % (name, getattr(t, "dtype", type(t))))
        if n == 0:
            return x
        return dynamic_propagate(guidance, self.activate(attention, n), x, sparse_depth, n, self.prop_kernel)

    def extra_repr(self):
        return "prop_time=%d, prop_kernel=%d, attention=%r" % (self.prop_time, self.prop_kernel, self.attention)
