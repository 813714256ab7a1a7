"""Line-scan propagation: the linear, three-way scan-line recurrence of SPN ("Learning Affinity via Spatial Propagation Networks"), the model the
propagation family started from and the baseline in the CSPN papers' tables; the same recurrence is the token mixer of recent line-scan models,
which use a per-pixel input weight lam instead of 1 - sum g.

Every contract of cspn_amd.cspn iterates a convolution; here a hidden line walks across the image once per direction, each pixel mixing its own
input with the three nearest pixels of the line visited before.  The engine runs all directions, channels and steps of a call in one launch
(cspn_amd.functional.cspn2d_forward_scan / cspn2d_backward_scan); the forward's result is the only history the backward needs, so autograd keeps
no per-step slice.  The gate stabiliser and the merge of the directions are torch ops around that one call.

Forward and backward are run-to-run bitwise (no atomics).  float32 only.

This module allocates nothing itself: every buffer comes from cspn_amd.functional or from the torch ops named above."""
import torch
import torch.nn as nn

from . import functional as F

NORMS = (None, 'clip')
MERGES = ('max', 'sum', 'mean', None)


class _LineScanFunction(torch.autograd.Function):
    """one cspn2d_forward_scan call, one cspn2d_backward_scan call on its result"""

    @staticmethod
    def forward(ctx, x, gates, lam, dirs):
        ctx.dirs = dirs
        out = F.cspn2d_forward_scan(x, gates, dirs, lam)
        ctx.save_for_backward(x, gates, lam, out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, gates, lam, out = ctx.saved_tensors
        gx, gg, gl = F.cspn2d_backward_scan(x, gates, out, grad_out.contiguous(), ctx.dirs, lam, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                            lam is not None and ctx.needs_input_grad[2])
        return gx, gg, gl, None


def linescan_propagate(x, gates, dirs=(0, 1, 2, 3), lam=None):
    """differentiable cspn2d_forward_scan on the gates as given -> [B,D*C,H,W]; gradients to x, gates and lam"""
    dirs = tuple(dirs)
    if torch.is_grad_enabled() and (x.requires_grad or gates.requires_grad or (lam is not None and lam.requires_grad)):
        return _LineScanFunction.apply(x, gates, lam, dirs)
    return F.cspn2d_forward_scan(x, gates, dirs, lam)


class LineScan_Propagate(nn.Module):
    """forward(x [B,C,H,W], gates [B,D*Cg*3,H,W], lam=None [B,D*C,H,W]) -> [B,C,H,W] (merge 'max' | 'sum' | 'mean') or [B,D*C,H,W] (merge None).
    dirs: a non-empty subset of {0: left->right, 1: right->left, 2: top->bottom, 3: bottom->top}, D its size, the directions numbered d = 0 .. D-1
    in ascending order of their code.  Gate channel (d*Cg + j)*3 + k: direction d, group j, connection k; Cg = groups (None: read off the gates'
    channel count) divides C and channel c uses group c // (C // Cg): groups = 1 is shared gates, groups = C is SPN's per-channel gates.  Per call:
        1. norm (a torch op, through autograd)   None: the gates as given;  'clip': SPN's stabiliser g_k / max(1, sum_k |g_k|) per direction,
           group and pixel
        2. the engine's scan, per direction: with t the coordinate along the scan and i along the line (directions 0 / 1: a line is a column;
           2 / 3: a row), L the line length, t- the line visited just before t, connection k to h(i + k - 1, t-):
               g^_k(i,t) = g_k(i,t) if t is not the first line and 0 <= i + k - 1 < L, else 0
               b(i,t)    = lam(i,t) if lam is given, else 1 - sum_k g^_k(i,t)
               h(i,t)    = b(i,t) x(i,t) + sum_k g^_k(i,t) h(i + k - 1, t-)
        3. merge (a torch op, through autograd)  the D results of a channel: 'max' their element-wise maximum (SPN), 'sum', 'mean'; None returns
           all of them, channel d*C + c
    THESE RULES ARE THE CONTRACT; they were written down from the published description of the method, not from a source: compare them with your
    model's before you port it.  Nothing is guarded: without 'clip', gates with sum |g| > 1 diverge as the formulas do.
    The module has no parameter and no state.  Gradients flow to x, gates (through norm) and lam.  A line has at most 2048 pixels.  float32 only:
    a float16 / bfloat16 / float64 tensor is a TypeError."""

    def __init__(self, dirs=(0, 1, 2, 3), groups=None, norm=None, merge='max'):
        super(LineScan_Propagate, self).__init__()
        mask, D = F._scan_mask(dirs)
        if norm not in NORMS:
            raise ValueError("norm must be one of %s, got %r" % (NORMS, norm))
        if merge not in MERGES:
            raise ValueError("merge must be one of %s, got %r" % (MERGES, merge))
        if groups is not None and (isinstance(groups, bool) or int(groups) != groups or groups < 1):
            raise ValueError("groups must be None or an int >= 1, got %r" % (groups,))
        self.dirs = tuple(d for d in range(4) if (mask >> d) & 1)
        self.groups = None if groups is None else int(groups)
        self.norm = norm
        self.merge = merge

    def normalize(self, gates):
        """step 1 above on gates [B, D*Cg*3, H, W]"""
        if self.norm == 'clip':
            B, ch, H, W = gates.shape
            g = gates.reshape(B, ch // 3, 3, H, W)
            return (g / g.abs().sum(2, keepdim=True).clamp(min=1)).reshape(gates.shape)
        return gates

    def merged(self, out, C):
        """step 3 above on out [B, D*C, H, W]"""
        if self.merge is None:
            return out
        B, _, H, W = out.shape
        o = out.reshape(B, len(self.dirs), C, H, W)
        if self.merge == 'max':
            return o.max(1).values
        return o.sum(1) if self.merge == 'sum' else o.mean(1)

    def forward(self, x, gates, lam=None):
        for t, name in ((x, "x"), (gates, "gates"), (lam, "lam")):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32):
                raise TypeError("%s must be a float32 tensor (got %s)" % (name, getattr(t, "dtype", type(t))))
        D = len(self.dirs)
        if x.dim() != 4 or gates.dim() != 4 or gates.shape[1] % (3 * D) or gates.shape[1] == 0:
            raise ValueError("x must be [B,C,H,W] and gates [B,%d*Cg*3,H,W], got %s and %s" % (D, tuple(x.shape), tuple(gates.shape)))
        if self.groups is not None and gates.shape[1] != 3 * D * self.groups:
            raise ValueError("gates must have %d*%d*3 = %d channels, got %d" % (D, self.groups, 3 * D * self.groups, gates.shape[1]))
        return self.merged(linescan_propagate(x, self.normalize(gates), self.dirs, lam), x.shape[1])

    def extra_repr(self):
        return "dirs=%r, groups=%r, norm=%r, merge=%r" % (self.dirs, self.groups, self.norm, self.merge)
