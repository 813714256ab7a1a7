"""Non-local spatial propagation (the refinement module of NLSPN and of the models built on it) on the engine's non-local kernels.

Every pixel learns real-valued offsets for its K*K - 1 neighbours; a step reads them by bilinear interpolation at p + base_k + offset_k(p) -- a
modulated deformable convolution with an all-ones weight, iterated on the same offsets and affinities.  The engine runs the iteration
(cspn_amd.functional.cspn2d_forward_nl / cspn2d_backward_nl) and the sampling of a confidence map at the same sites (cspn2d_nl_sample); the affinity
normalisation is a handful of torch ops, run once per call through autograd.

Neighbour k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre and its base is (t - K//2, l - K//2): the deformable
convolution's sign, the OPPOSITE of Affinity_PropagateKxK's (K//2 - t, K//2 - l).

The default backward is NOT run-to-run bitwise: the adjoint of the gather is a scatter with float atomics, whose sums depend on arrival order in
their last bits.  The forward is bitwise reproducible.  A second backward is: under torch.use_deterministic_algorithms(True), or where asked for
(nl_propagate / nl_sample: deterministic=True; the module: its attribute `deterministic`), the gradients come from cspn2d_backward_nl_det and
cspn2d_nl_sample_backward_det, which gather through an inverted index (about 270 bytes a pixel of workspace) and sum order-independently.

float16 / bfloat16 affinities and offsets (what a head under torch.autocast emits) are taken as they are: where aff or offset is 16-bit the calls go
to the *_g16 functions (cspn2d_forward_nl_g16, ...), which widen each value exactly where the kernels read it and return dL/daff and dL/doffset in
the dtype of the tensor they belong to; float32 tensors reach the functions they always reached.

This module allocates nothing itself: every buffer comes from cspn_amd.functional."""
import torch
import torch.nn as nn

from . import functional as F

AFFINITIES = ('AS', 'ASS', 'TC', 'TGASS')


_HALVES = (torch.float16, torch.bfloat16)


def _g16(*tensors):
    """'_g16' where one of the tensors (aff, offset) is 16-bit: the suffix of the cspn_amd.functional names the call goes to"""
    return "_g16" if any(t.dtype in _HALVES for t in tensors) else ""


def _deterministic(forced):
    """which backward runs: what the caller forced, else torch's flag at the time of the backward"""
    return torch.are_deterministic_algorithms_enabled() if forced is None else bool(forced)


class _OffsetGradient(object):
    """where the two uses of one 16-bit offset tensor (the propagation and the confidence sampling) leave their float32 gradients, so that their
    sum is rounded to the offset's dtype once (_OffsetFanout.backward) instead of each being rounded and the two added in 16 bits"""

    def __init__(self):
        self.total = None

    def add(self, grad):
        if self.total is None:
            self.total = grad
        else:
            self.total += grad

    def take(self):
        total, self.total = self.total, None
        return total


def _no_gradient(t):
    """what a use of the offset returns in the offset's place when its float32 gradient went to an _OffsetGradient: zeros of no size in memory"""
    return torch.tensor(0.0, dtype=t.dtype, device=t.device).expand(t.shape)


class _OffsetFanout(torch.autograd.Function):
    """offset -> two aliases of it, one for each use; backward: the float32 sum the two uses left in `joined`, rounded once"""

    @staticmethod
    def forward(ctx, offset, joined):
        ctx.joined, ctx.dtype = joined, offset.dtype
        return offset.view_as(offset), offset.view_as(offset)

    @staticmethod
    def backward(ctx, g1, g2):
        total = ctx.joined.take()
        return (None if total is None else total.to(ctx.dtype)), None


class _NonLocalFunction(torch.autograd.Function):
    """one cspn2d_forward_nl call that keeps the levels where dL/daff or dL/doffset will need them, one cspn2d_backward_nl call.  joined (the
    module with a confidence on a 16-bit offset): the backward runs on offset.float(), whose history is the forward's bit for bit, and leaves
    the float32 dL/doffset there"""

    @staticmethod
    def forward(ctx, aff, offset, x, sparse_depth, n_iter, kernel_size, deterministic, joined=None):
        ctx.n_iter, ctx.kernel_size, ctx.deterministic, ctx.joined = n_iter, kernel_size, deterministic, joined
        hist = None
        forward = getattr(F, "cspn2d_forward_nl" + _g16(aff, offset))
        if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and n_iter >= 2:
            out, hist = forward(aff, offset, x, sparse_depth, n_iter, kernel_size, return_history=True)
        else:
            out = forward(aff, offset, x, sparse_depth, n_iter, kernel_size)
        ctx.save_for_backward(aff, offset, x, sparse_depth, hist)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        aff, offset, x, sparse_depth, hist = ctx.saved_tensors
        backward = getattr(F, ("cspn2d_backward_nl_det" if _deterministic(ctx.deterministic) else "cspn2d_backward_nl") + _g16(aff, offset))
        joined = ctx.joined is not None and ctx.needs_input_grad[1]
        ga, gd, gx = backward(aff, offset.float() if joined else offset, x, sparse_depth, grad_out.contiguous(), ctx.n_iter, ctx.kernel_size, hist,
                              ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        if joined:
            ctx.joined.add(gd)
            gd = _no_gradient(offset)
        return ga, gd, gx, None, None, None, None, None


class _NLSampleFunction(torch.autograd.Function):
    """cspn2d_nl_sample and its backward: f [B,1,H,W] read at the K*K - 1 sites of every pixel"""

    @staticmethod
    def forward(ctx, offset, f, kernel_size, deterministic, joined=None):
        ctx.kernel_size, ctx.deterministic, ctx.joined = kernel_size, deterministic, joined
        ctx.save_for_backward(offset, f)
        return getattr(F, "cspn2d_nl_sample" + _g16(offset))(offset, f, kernel_size)

    @staticmethod
    def backward(ctx, grad_out):
        offset, f = ctx.saved_tensors
        backward = getattr(F, ("cspn2d_nl_sample_backward_det" if _deterministic(ctx.deterministic) else "cspn2d_nl_sample_backward") + _g16(offset))
        joined = ctx.joined is not None and ctx.needs_input_grad[0]
        gf, gd = backward(offset.float() if joined else offset, f, grad_out.contiguous(), ctx.kernel_size, ctx.needs_input_grad[1], ctx.needs_input_grad[0])
        if joined:
            ctx.joined.add(gd)
            gd = _no_gradient(offset)
        return gd, gf, None, None, None


def nl_sample(offset, f, kernel_size=3, deterministic=None):
    """differentiable cspn2d_nl_sample: out[:, k](p) = bil(f, p + base_k + offset_k(p)), gradients to f and offset.  deterministic: True / False
    picks the run-to-run bitwise backward or the scatter; None follows torch.are_deterministic_algorithms_enabled() when the backward runs.  offset
    float32, float16 or bfloat16 (dL/doffset in its dtype); f float32"""
    if torch.is_grad_enabled() and (offset.requires_grad or f.requires_grad):
        return _NLSampleFunction.apply(offset, f, kernel_size, deterministic)
    return getattr(F, "cspn2d_nl_sample" + _g16(offset))(offset, f, kernel_size)


def nl_propagate(aff, offset, x, sparse_depth, n_iter, kernel_size=3, deterministic=None):
    """differentiable cspn2d_forward_nl on affinities as given, gradients to aff, offset and x (sparse_depth has none).  deterministic: as in
    nl_sample.  aff / offset in the pairs (float32, float32), (float32, T), (T, T), T float16 or bfloat16: their gradients come back in their dtypes"""
    if torch.is_grad_enabled() and (aff.requires_grad or offset.requires_grad or x.requires_grad):
        return _NonLocalFunction.apply(aff, offset, x, sparse_depth, n_iter, kernel_size, deterministic)
    return getattr(F, "cspn2d_forward_nl" + _g16(aff, offset))(aff, offset, x, sparse_depth, n_iter, kernel_size)


class NonLocal_Propagate(nn.Module):
    """forward(affinity [B,8,H,W] raw, offset [B,16,H,W], feat [B,C,H,W], confidence=None [B,1,H,W], sparse_depth=None [B,1,H,W], n_iter=None)
    -> [B,C,H,W] after prop_time (or n_iter) non-local steps.  Per call, in torch and through autograd, with KK = prop_kernel**2 - 1:
        1. squash     'TC': a = tanh(g) / KK;  'TGASS': a = tanh(g) / (scale + 1e-8);  'AS', 'ASS': a = g
        2. confidence (where given)  a_k <- a_k * bil(confidence, p + base_k + offset_k(p))      (cspn2d_nl_sample)
        3. abs-sum    with S = sum_k |a_k|:  'AS': a / (S + 1e-4);  'ASS' and 'TGASS': a / max(S + 1e-4, 1);  'TC': a
    then the engine's iteration on these affinities: H <- (1 - sum_k a_k) Ht + sum_k a_k bil(Ht, p + base_k + offset_k(p)), where Ht is H with
    sparse_depth put back where sparse_depth > 0 (preserve_input and a sparse_depth given; otherwise no mask).  offset channel 2k is dy_k, 2k + 1
    is dx_k; base_k = (t - 1, l - 1) in raster order without the centre: the deformable convolution's sign.
    scale is a parameter the module owns ('TGASS' only, initialised to affinity_gamma * KK): the module's only state.
    THESE FOUR RULES ARE THE CONTRACT; they were written down from the published module's description, not from its source: compare them with
    your model's before you port it.
    Gradients flow to affinity, offset, feat, confidence and scale; the default backward is not run-to-run bitwise (float atomics in the adjoint).
    deterministic (a class attribute, None; set it on an instance): True takes the run-to-run bitwise backward for the propagation and the confidence
    sampling, False the scatter, None follows torch.are_deterministic_algorithms_enabled() when the backward runs.
    Mixed precision: affinity and offset may each be float32, float16 or bfloat16, as a head under torch.autocast emits them.  A 16-bit affinity is
    widened with .float() and steps 1 - 3 run in float32 with autocast disabled, so dL/daffinity returns in the affinity's dtype through autograd;
    the offset goes to the engine as it is (no float32 copy of its 16 planes is made in the forward) and dL/doffset comes back in its dtype,
    rounded once: with a confidence the offset is used twice (the sampling and the steps), and the two backwards then run on offset.float() and
    add their float32 gradients before that one rounding (16 float32 planes twice, for the time of the backward).  A 16-bit feat, confidence or
    sparse_depth is widened with .float() (single planes).  The output is float32.  float64 anywhere is a TypeError."""

    deterministic = None

    def __init__(self, prop_time, prop_kernel=3, affinity='TGASS', affinity_gamma=0.5, preserve_input=True):
        super(NonLocal_Propagate, self).__init__()
        if prop_kernel != 3:
            raise ValueError("non-local propagation is built for prop_kernel 3 only (5 and 7 are not), got %r" % (prop_kernel,))
        if affinity not in AFFINITIES:
            raise ValueError("affinity must be one of %s, got %r" % (AFFINITIES, affinity))
        if isinstance(prop_time, bool) or int(prop_time) != prop_time or prop_time < 0:
            raise ValueError("prop_time must be an int >= 0, got %r" % (prop_time,))
        self.prop_time = int(prop_time)
        self.prop_kernel = prop_kernel
        self.affinity = affinity
        self.affinity_gamma = float(affinity_gamma)
        self.preserve_input = bool(preserve_input)
        self.num_neighbors = prop_kernel * prop_kernel - 1
        if affinity == 'TGASS':
            self.scale = nn.Parameter(self.affinity_gamma * self.num_neighbors * torch.ones(1))

    def normalize(self, affinity, offset=None, confidence=None):
        """steps 1 - 3 above -> the affinities the engine uses as given; a 16-bit affinity (or confidence) is widened first and the steps run in
        float32 whatever autocast region the call is made in"""
        with torch.autocast(affinity.device.type, enabled=False):
            a, confidence = F.widen16(affinity, confidence)
            sampled = None if confidence is None else nl_sample(offset, confidence, self.prop_kernel, self.deterministic)
            return self._normalize(a, sampled)

    def _normalize(self, a, sampled):
        """steps 1 - 3 on a float32 affinity and the confidence as sampled at the neighbours' sites (or None)"""
        with torch.autocast(a.device.type, enabled=False):
            if self.affinity == 'TC':
                a = torch.tanh(a) / self.num_neighbors
            elif self.affinity == 'TGASS':
                a = torch.tanh(a) / (self.scale + 1e-8)
            if sampled is not None:
                a = a * sampled
            if self.affinity == 'TC':
                return a
            S = a.abs().sum(1, keepdim=True) + 1e-4
            if self.affinity != 'AS':
                S = S.clamp(min=1.0)
            return a / S

    def forward(self, affinity, offset, feat, confidence=None, sparse_depth=None, n_iter=None):
        n = self.prop_time if n_iter is None else int(n_iter)
        if n < 0:
            raise ValueError("n_iter must be >= 0 (got %r)" % (n_iter,))
        KK = self.num_neighbors
        for t, name, ch in ((affinity, "affinity", KK), (offset, "offset", 2 * KK)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != ch:
                raise ValueError("%s must be [B,%d,H,W], got %s" % (name, ch, tuple(getattr(t, "shape", ()))))
        if confidence is not None and (not isinstance(confidence, torch.Tensor) or confidence.dim() != 4
                                       or tuple(confidence.shape) != (affinity.shape[0], 1) + tuple(affinity.shape[2:])):
            raise ValueError("confidence must be [B,1,H,W] = %s, got %s" % ((affinity.shape[0], 1) + tuple(affinity.shape[2:]),
                                                                           tuple(getattr(confidence, "shape", ()))))
        if n == 0:
            return feat
        feat, sparse_depth = F.widen16(feat, sparse_depth)
        sparse_depth = sparse_depth if self.preserve_input else None
        if confidence is not None and offset.dtype in _HALVES and offset.requires_grad and torch.is_grad_enabled():
            # the offset is used twice: its two float32 gradients are added and rounded once (_OffsetFanout), not rounded twice and added in 16 bits
            joined = _OffsetGradient()
            for_sampling, for_steps = _OffsetFanout.apply(offset, joined)
            a, confidence = F.widen16(affinity, confidence)
            aff = self._normalize(a, _NLSampleFunction.apply(for_sampling, confidence, self.prop_kernel, self.deterministic, joined))
            return _NonLocalFunction.apply(aff, for_steps, feat, sparse_depth, n, self.prop_kernel, self.deterministic, joined)
        aff = self.normalize(affinity, offset, confidence)
        return nl_propagate(aff, offset, feat, sparse_depth, n, self.prop_kernel, self.deterministic)

    def extra_repr(self):
        return "prop_time=%d, prop_kernel=%d, affinity=%r, affinity_gamma=%g, preserve_input=%r" % (
            self.prop_time, self.prop_kernel, self.affinity, self.affinity_gamma, self.preserve_input)
