"""Drop-in for reference cspn_pytorch/models/cspn.py: same class name, same
constructor, same forward call -- the arithmetic runs in hand-written HIP kernels
(libcspn_amd.so) instead of ZeroPad2d + cat + Conv3d.

    reference                                   here
    Affinity_Propagate(prop_time, prop_kernel,  identical signature (cspn.py:16-19)
                       norm_type='8sum')
    forward(guidance, blur_depth,               identical, plus an optional n_iter that
            sparse_depth=None)                  overrides prop_time (BASELINE north_star)

Differences a caller can observe, all deliberate:
  * no `sum_conv` sub-module ever appears in state_dict() (the reference registers one
    during its first forward, cspn.py:44-53; checkpoints are key-filtered on load,
    update_model.py:16-23, so both directions keep working);
  * inputs must already be on the GPU (the reference calls .cuda() itself, cspn.py:50);
  * differentiable w.r.t. guidance and blur_depth (HIP backward kernels, cspn_amd/csrc/cspn2d_backward.hip: the gradient
    torch autograd computes through the reference forward, which reference train.py:196-198 back-propagates through);
    sparse_depth gets no gradient (only its sign is used, cspn.py:64);
  * blur_depth [B,C,H,W] with C > 1 is propagated on the shared affinities like the reference's broadcast (cspn.py:58-81), with
    sparse_depth None, [B,1,H,W] or [B,C,H,W]: one engine call each way (cspn2d_forward_multi_f32 / cspn2d_backward_multi_f32),
    dL/dguidance summed over the channels;
  * float16 / bfloat16 inputs (heads under torch.autocast) are taken and the result is float32: Affinity_PropagateKxK with prop_kernel
    5 / 7, CSPN in 2D with prop_kernel 5 / 7, CSPN in 3D and Affinity_Propagate3d hand a 16-bit guidance / guide to the engine as it is
    (widened exactly where used, its gradient in its dtype); everything without a 16-bit kernel (Affinity_Propagate, prop_kernel 3 in 2D,
    propagate_prenorm) widens with a differentiable .float() first, and so does every module with its value tensors."""
import torch
import torch.nn as nn

from . import functional as F


# the functional calls of one channel and of C > 1 channels on the shared guidance: history size query, forward keeping the history, backward from it,
# plain forward, plain backward
_CALLS = {False: (F.cspn2d_history_bytes, F.cspn2d_forward_with_history, F.cspn2d_backward_from_history, F.cspn2d_forward, F.cspn2d_backward),
          True: (F.cspn2d_history_bytes_multi, F.cspn2d_forward_with_history_multi, F.cspn2d_backward_from_history_multi,
                 F.cspn2d_forward_multi, F.cspn2d_backward_multi)}


class _CSPN2dFunction(torch.autograd.Function):
    """blur_depth [B,1,H,W] runs exactly the single-channel calls; [B,C,H,W] with C > 1 the multi-channel ones on the shared guidance (reference
    cspn.py:58-81 broadcasts the affinities): one engine call each way, dL/dguidance summed over the channels inside the engine"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, n_iter, norm_type, algo, keep_history):
        ctx.n_iter, ctx.norm_type = n_iter, norm_type
        ctx.multi = isinstance(blur_depth, torch.Tensor) and blur_depth.dim() == 4 and blur_depth.shape[1] > 1
        history_bytes, forward_with_history, _, forward, _ = _CALLS[ctx.multi]
        needs_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        shape = blur_depth.shape if ctx.multi else (guidance.shape[0],) + tuple(guidance.shape[2:])
        if (keep_history and needs_grad and algo in ("auto", "fused") and guidance.is_cuda
                and history_bytes(*shape, n_iter) > 0):
            # training: the forward keeps every FOURTH intermediate level (H_4 .. H_20) and the folded coefficients -- 13 planes per
            # image-channel, where autograd keeps ~27 temporaries per iteration for the reference --, the backward starts from them and
            # recomputes the three levels in between
            out, hist = forward_with_history(guidance, blur_depth, sparse_depth, n_iter, norm_type)
            ctx.save_for_backward(guidance, blur_depth, sparse_depth, hist)
            return out
        ctx.save_for_backward(guidance, blur_depth, sparse_depth, None)
        return forward(guidance, blur_depth, sparse_depth, n_iter, norm_type, algo)

    @staticmethod
    def backward(ctx, grad_out):
        guidance, blur_depth, sparse_depth, hist = ctx.saved_tensors
        _, _, backward_from_history, _, backward = _CALLS[ctx.multi]
        need = dict(need_guidance=ctx.needs_input_grad[0], need_blur=ctx.needs_input_grad[1])
        if hist is not None:
            gg, gh = backward_from_history(guidance, blur_depth, sparse_depth, grad_out, hist, ctx.n_iter, ctx.norm_type, **need)
        else:
            gg, gh = backward(guidance, blur_depth, sparse_depth, grad_out, ctx.n_iter, ctx.norm_type, **need)
        return gg, gh, None, None, None, None, None


_apply = _CSPN2dFunction.apply


def propagate_prenorm(gate_wb, blur_depth, sparse_depth=None, n_iter=24, algo="auto", keep_history=True):
    """The loop of reference cspn.py:66-81 started from the tensor its affinity_normalization returns (gate_wb [B,8,H,W], cropped to the
    image: what cspn_amd.cspn2d_normalize or the guidance head with norm_type='8sum' emit) -- the pre-normalised input contract
    (CSPN_NORM_PRENORM), differentiable: the gradients w.r.t. gate_wb and blur_depth are what torch autograd computes through the
    reference forward for those two tensors (tests/golden/cspn2d_grad_prenorm_golden.npz).  Autograd chains dL/dgate_wb into whatever produced it:
    both producers the engine ships are differentiable -- cspn_amd.cspn2d_normalize (cspn2d_normalize_backward_f32) and
    train_utils.guidance_heads(..., norm_type='8sum' | '8sum_abs') (that, then cspn_guidance_head_backward_f32)."""
    if n_iter == 0:
        return blur_depth
    gate_wb, blur_depth, sparse_depth = F.widen16(gate_wb, blur_depth, sparse_depth)
    return _apply(gate_wb, blur_depth, sparse_depth, int(n_iter), "prenorm", algo, keep_history)


class Affinity_Propagate(nn.Module):

    def __init__(self, prop_time, prop_kernel, norm_type='8sum'):
        super(Affinity_Propagate, self).__init__()
        self.prop_time = prop_time
        self.prop_kernel = prop_kernel
        assert prop_kernel == 3, 'this version only support 8 (3x3 - 1) neighborhood'  # cspn.py:33
        self.norm_type = norm_type
        assert norm_type in ['8sum', '8sum_abs']  # cspn.py:36
        self.in_feature = 1
        self.out_feature = 1
        self.algo = "auto"
        self.keep_history = True   # training: keep the forward's checkpoints (every fourth level + folded coefficients) for the backward

    def forward(self, guidance, blur_depth, sparse_depth=None, n_iter=None):
        n = self.prop_time if n_iter is None else int(n_iter)
        if '8sum' not in self.norm_type:  # cspn.py:75-78
            raise ValueError('unknown norm %s' % self.norm_type)
        if n == 0:
            return blur_depth  # cspn.py:61,66,83: the very same tensor object
        guidance, blur_depth, sparse_depth = F.widen16(guidance, blur_depth, sparse_depth)   # no 16-bit 3 x 3 kernel: float32 from here on
        return _apply(guidance, blur_depth, sparse_depth, n, self.norm_type, self.algo, self.keep_history)

    def extra_repr(self):
        return "prop_time=%d, prop_kernel=%d, norm_type=%r" % (self.prop_time, self.prop_kernel, self.norm_type)


class _CSPN3dNormFunction(torch.autograd.Function):
    """F.cspn3d_forward_norm in a normalising mode; the backward is one cspn3d_backward_norm_f32 / _g16 call (the fold and the levels are
    recomputed there).  A float16 / bfloat16 guidance is saved as it is and gets its gradient in its dtype.  blur_depth [B,C,D,H,W] with
    C > 1 and a shared mask: the multi-channel entry points, one call each way"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, n_iter, norm_type, algo):
        ctx.n_iter, ctx.norm_type, ctx.algo = n_iter, norm_type, algo
        ctx.save_for_backward(guidance, blur_depth, sparse_depth)
        return F.cspn3d_forward_norm(guidance, blur_depth, sparse_depth, n_iter, norm_type, algo)

    @staticmethod
    def backward(ctx, grad_out):
        guidance, blur_depth, sparse_depth = ctx.saved_tensors
        gg, gh = F.cspn3d_backward_norm(guidance, blur_depth, sparse_depth, grad_out, ctx.n_iter, ctx.norm_type,
                                        "stepwise" if ctx.algo == "stepwise" else "auto",   # ('persistent' is a wish about the forward)
                                        need_guidance=ctx.needs_input_grad[0], need_feat=ctx.needs_input_grad[1])
        return gg, gh, None, None, None, None


class Affinity_Propagate3d(nn.Module):
    """The 3D twin of Affinity_Propagate (same constructor, same forward): guidance [B,26,D,H,W] raw, blur_depth and sparse_depth
    [B,1,D,H,W] -- neighbour-sited gates divided by the abs-sum of the in-range ones, the (1 - sigma) H_0 centre term and the sparse pin over
    the 26-neighbourhood (F.cspn3d_forward with '8sum' / '8sum_abs'), differentiable w.r.t. guidance and blur_depth
    (F.cspn3d_backward_norm); sparse_depth gets no gradient.  A float16 / bfloat16 guidance (a head under torch.autocast) goes to the engine
    as it is -- widened exactly where a kernel reads it, no float32 copy, its gradient in its dtype (cspn3d_forward_norm_g16 /
    cspn3d_backward_norm_g16); a 16-bit blur_depth or sparse_depth is widened with a differentiable .float().  The result is float32.
    blur_depth [B,C,D,H,W] with C > 1 (the feature channels of a cost volume) is propagated on the shared affinities, as the 2D module
    broadcasts its own (reference cspn.py:58-81), with sparse_depth None or [B,1,D,H,W]: one engine call each way
    (cspn3d_forward_norm_multi_f32 / cspn3d_backward_norm_multi_f32 and their _g16 forms), dL/dguidance summed over the channels inside the
    engine.  A per-channel mask [B,C,D,H,W] has no shared folded weights: it takes the SLOW route, one single-channel call per channel, and
    autograd sums the C guidance gradients."""

    def __init__(self, prop_time, prop_kernel=3, norm_type='8sum_abs'):
        super(Affinity_Propagate3d, self).__init__()
        self.prop_time = prop_time
        self.prop_kernel = prop_kernel
        assert prop_kernel == 3, 'this version only support 26 (3x3x3 - 1) neighborhood'
        self.norm_type = norm_type
        assert norm_type in ['8sum', '8sum_abs']
        self.algo = "auto"   # 'stepwise': one launch per step, forward and backward

    def forward(self, guidance, blur_depth, sparse_depth=None, n_iter=None):
        n = self.prop_time if n_iter is None else int(n_iter)
        if n == 0:
            return blur_depth
        blur_depth, sparse_depth = F.widen16(blur_depth, sparse_depth)   # the guidance stays as it is: the 3D kernels read it in 16 bits
        C = blur_depth.shape[1] if blur_depth.dim() == 5 else 1
        if C > 1 and sparse_depth is not None and sparse_depth.dim() == 5 and sparse_depth.shape[1] == C:   # a mask per channel: the slow route
            return torch.cat([_CSPN3dNormFunction.apply(guidance, blur_depth[:, c:c + 1].contiguous(), sparse_depth[:, c:c + 1].contiguous(), n,
                                                        self.norm_type, self.algo) for c in range(C)], 1)
        return _CSPN3dNormFunction.apply(guidance, blur_depth, sparse_depth, n, self.norm_type, self.algo)

    def extra_repr(self):
        return "prop_time=%d, prop_kernel=%d, norm_type=%r" % (self.prop_time, self.prop_kernel, self.norm_type)


class _CSPN2dKxKFoldFunction(torch.autograd.Function):
    """The folded and the assembling K x K contracts under autograd, pinned or not (F._fold_forward / F._fold_backward): one forward engine call
    that keeps the history where a gradient that reads it is needed -- dL/dguidance or dL/dpin_conf at n_iter >= 2 (both read the gradient of the
    folded gates), dL/dconf always (it reads the collected levels) -- and one backward engine call.  The four classes below say which inputs
    they have; their forward's parameter list is what autograd numbers needs_input_grad by, always in this order: guidance, blur_depth,
    sparse_depth, [pin_conf,] [conf, steps,] kernel_size, n_iter, norm_type, dilation."""

    @staticmethod
    def run(ctx, guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, dilation):
        """assemble: None or (conf, steps)"""
        ctx.pinned, ctx.steps, ctx.args, ctx.dilation = pinned, assemble and assemble[1], (kernel_size, n_iter, norm_type), dilation
        need = ctx.needs_input_grad
        keep = ((need[0] or (pinned and need[3])) and n_iter >= 2) or (assemble is not None and need[3 + pinned])
        out = F._fold_forward(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, kernel_size, n_iter, norm_type, keep, dilation)
        out, hist = out if keep else (out, None)
        ctx.save_for_backward(guidance, blur_depth, sparse_depth, *((pin_conf,) if pinned else ()), *(assemble[:1] if assemble else ()), hist)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        guidance, blur_depth, sparse_depth, *rest, hist = ctx.saved_tensors
        pinned = ctx.pinned
        pin_conf = rest.pop(0) if pinned else None
        assemble = (rest.pop(0), ctx.steps) if ctx.steps is not None else None
        need = ctx.needs_input_grad
        # (a flag read at the position of an input the class does not have is dropped by F._fold_backward, which knows the contract)
        gg, gh, gc, gs, gp = F._fold_backward(guidance, blur_depth, sparse_depth, pin_conf, pinned, assemble, grad_out, *ctx.args, hist, ctx.dilation,
                                              need_guidance=need[0], need_blur=need[1], need_conf=need[3 + pinned], need_sparse=need[2], need_pin=need[3])
        grads = (gg, gh, gs) + ((gp,) if pinned else ()) + ((gc,) if assemble else ())
        return grads + (None,) * (len(need) - len(grads))


class _CSPN2dKxKNormFunction(_CSPN2dKxKFoldFunction):
    """Affinity_PropagateKxK without a pin_conf: cspn2d_forward_kxk_norm keeping H_1 .. H_{n-1}, cspn2d_backward_kxk_norm (the fold is recomputed
    there)"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, kernel_size, n_iter, norm_type, dilation):
        return _CSPN2dKxKFoldFunction.run(ctx, guidance, blur_depth, sparse_depth, None, False, None, kernel_size, n_iter, norm_type, dilation)


class _CSPN2dKxKNormPinFunction(_CSPN2dKxKFoldFunction):
    """Affinity_PropagateKxK with a pin_conf, every prop_kernel: cspn2d_forward_kxk_norm_pin keeping H_1 .. H_{n-1}, cspn2d_backward_kxk_norm_pin"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, pin_conf, kernel_size, n_iter, norm_type, dilation):
        return _CSPN2dKxKFoldFunction.run(ctx, guidance, blur_depth, sparse_depth, pin_conf, True, None, kernel_size, n_iter, norm_type, dilation)


class _CSPN2dKxKAssembleFunction(_CSPN2dKxKFoldFunction):
    """one kernel size of Affinity_PropagateAssemble: cspn2d_forward_kxk_assemble keeping H_1 .. H_n, cspn2d_backward_kxk_assemble"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, conf, steps, kernel_size, n_iter, norm_type, dilation):
        return _CSPN2dKxKFoldFunction.run(ctx, guidance, blur_depth, sparse_depth, None, False, (conf, steps), kernel_size, n_iter, norm_type, dilation)


class _CSPN2dKxKAssemblePinFunction(_CSPN2dKxKFoldFunction):
    """one kernel size of Affinity_PropagateAssemble with a pin_conf: cspn2d_forward_kxk_assemble_pin keeping H_1 .. H_n,
    cspn2d_backward_kxk_assemble_pin"""

    @staticmethod
    def forward(ctx, guidance, blur_depth, sparse_depth, pin_conf, conf, steps, kernel_size, n_iter, norm_type, dilation):
        return _CSPN2dKxKFoldFunction.run(ctx, guidance, blur_depth, sparse_depth, pin_conf, True, (conf, steps), kernel_size, n_iter, norm_type, dilation)


class Affinity_PropagateKxK(nn.Module):
    """Affinity_Propagate (same constructor, same forward) with prop_kernel 3, 5 or 7 -- what cspn_config['kernel'] asks of the reference
    (torch_resnet_cspn_nyu.py:281,344-347; cspn.py:24 "current only support 3x3").  guidance [B, K*K-1, H, W] raw, channel k the k-th
    pair (t, l) in raster order over {0..K-1}^2 without the centre, its gate sited at the neighbour (K//2 - t, K//2 - l): at K = 3 the
    reference's gate1 .. gate8.  prop_kernel 3 runs today's 3 x 3 path (bitwise Affinity_Propagate); 5 and 7 the K x K engine
    (F.cspn2d_forward_kxk_norm), differentiable w.r.t. guidance and blur_depth.  float16 / bfloat16 guidance goes to the K x K engine as it
    is (prop_kernel 3: widened first); the result is float32.
    dilation 2 puts the neighbour of gate (t, l) at 2 * (K//2 - t, K//2 - l) -- the dilated pass of PENet's refinement (dilated CSPN++),
    which runs each propagation at dilation 2 and then once more at dilation 1.  It runs the K x K engine for every prop_kernel, 3
    included (the engine's own K = 3 instance, not the 3 x 3 ring).
    forward(..., pin_conf=...) pins softly to the measured depth, as CSPN++-style refinements (PENet's included) do after every step:
    H <- (1 - m) step(H) + m sparse_depth with m = sign(sparse_depth) * pin_conf, in place of the reference's hard pin to blur_depth.  pin_conf
    has sparse_depth's shape and is used as given (a sigmoid of a confidence head is the caller's); it needs a sparse_depth.  One engine call
    each way (F.cspn2d_forward_kxk_norm_pin / F.cspn2d_backward_kxk_norm_pin), differentiable w.r.t. guidance, blur_depth, sparse_depth and
    pin_conf; it runs the K x K engine for every prop_kernel and dilation (the ring does not pin softly).  pin_conf=None is the module as it
    was."""

    def __init__(self, prop_time, prop_kernel, norm_type='8sum', dilation=1):
        super(Affinity_PropagateKxK, self).__init__()
        assert prop_kernel in (3, 5, 7), 'the neighbourhood is 3 x 3, 5 x 5 or 7 x 7'
        assert norm_type in ['8sum', '8sum_abs']
        self.prop_time = prop_time
        self.prop_kernel = prop_kernel
        self.norm_type = norm_type
        self.dilation = F.check_dilation(dilation)
        self.algo = "auto"          # prop_kernel 3: as Affinity_Propagate
        self.keep_history = True

    def forward(self, guidance, blur_depth, sparse_depth=None, n_iter=None, pin_conf=None):
        if pin_conf is not None and sparse_depth is None:
            raise ValueError("pin_conf needs a sparse_depth: it weights the pin to the measured depth")
        n = self.prop_time if n_iter is None else int(n_iter)
        if n == 0:
            return blur_depth
        blur_depth, sparse_depth = F.widen16(blur_depth, sparse_depth)
        if pin_conf is not None:
            pin_conf = F.widen16(pin_conf)
            if torch.is_grad_enabled() and any(t.requires_grad for t in (guidance, blur_depth, sparse_depth, pin_conf)):
                return _CSPN2dKxKNormPinFunction.apply(guidance, blur_depth, sparse_depth, pin_conf, self.prop_kernel, n, self.norm_type, self.dilation)
            return F.cspn2d_forward_kxk_norm_pin(guidance, blur_depth, sparse_depth, pin_conf, self.prop_kernel, n, self.norm_type, dilation=self.dilation)
        if self.prop_kernel == 3 and self.dilation == 1:
            return _apply(F.widen16(guidance), blur_depth, sparse_depth, n, self.norm_type, self.algo, self.keep_history)
        if torch.is_grad_enabled() and (guidance.requires_grad or blur_depth.requires_grad):
            return _CSPN2dKxKNormFunction.apply(guidance, blur_depth, sparse_depth, self.prop_kernel, n, self.norm_type, self.dilation)
        return F.cspn2d_forward_kxk_norm(guidance, blur_depth, sparse_depth, self.prop_kernel, n, self.norm_type, dilation=self.dilation)

    def extra_repr(self):
        return "prop_time=%d, prop_kernel=%d, norm_type=%r" % (self.prop_time, self.prop_kernel, self.norm_type) \
            + (", dilation=%d" % self.dilation if self.dilation != 1 else "")


class Affinity_PropagateAssemble(nn.Module):
    """The propagation of CSPN++ ("context-aware" CSPN; with dilations, each pass of PENet's dilated refinement): Affinity_PropagateKxK over several kernel sizes at once, the result a
    per-pixel weighted sum over collected iterations and over kernel sizes,
        out = sum_k kernel_conf[:, k] * sum_j iter_conf[k][:, j] * H^{K_k}_{steps[j]},      H^K_0 = blur_depth.
    prop_kernels: kernel sizes out of 3, 5, 7 (3 runs the K x K engine's own K = 3 instance, not the 3 x 3 ring); steps: the collected
    iterations, strictly increasing, ending at prop_time (None: (prop_time,), the last level only).
    forward(guidances, blur_depth, sparse_depth=None, iter_conf=None, kernel_conf=None, n_iter=None): guidances and iter_conf are sequences with
    one entry per kernel size, [B,K*K-1,H,W] raw (the channel order of Affinity_PropagateKxK) and [B,len(steps),H,W]; kernel_conf
    [B,len(prop_kernels),H,W].  iter_conf None means ones, kernel_conf None no such factor.  No softmax is applied: normalising the
    confidences is the caller's job.  kernel_conf[:, k:k+1] is multiplied into iter_conf[k] with one torch op, then each kernel size is one
    engine call each way (F.cspn2d_forward_kxk_assemble / F.cspn2d_backward_kxk_assemble) and the results are summed.  Differentiable w.r.t. the
    guidances, blur_depth, iter_conf and kernel_conf.  float16 / bfloat16 guidance goes to the engine as it is; the result is float32.  n_iter
    overrides prop_time and needs steps that end at it; n_iter == 0 returns blur_depth itself, as the other modules do.  No parameters or buffers.
    dilations: 1 or 2, one int for all or one per entry of prop_kernels (the same kernel size may appear twice with different dilations); the
    neighbour of gate (t, l) of entry k is dilations[k] * (K//2 - t, K//2 - l).  PENet's refinement is this module at dilation 2 feeding the
    same module at dilation 1.
    forward(..., pin_conf=...): the levels are pinned softly to the measured depth after every step, H <- (1 - m) step(H) + m sparse_depth with
    m = sign(sparse_depth) * pin_conf (Affinity_PropagateKxK).  pin_conf is one tensor of sparse_depth's shape for all kernel sizes, or a
    sequence with one per entry of prop_kernels (each size has its own confidence head, as in PENet); it needs a sparse_depth.  Gradients then
    also flow to sparse_depth and pin_conf (F.cspn2d_*_kxk_assemble_pin).  pin_conf=None is the module as it was."""

    def __init__(self, prop_time, prop_kernels=(3, 5, 7), steps=None, norm_type='8sum', dilations=1):
        super(Affinity_PropagateAssemble, self).__init__()
        prop_kernels = tuple(prop_kernels)
        assert len(prop_kernels) >= 1 and all(k in (3, 5, 7) for k in prop_kernels), 'the neighbourhoods are 3 x 3, 5 x 5 or 7 x 7'
        assert norm_type in ['8sum', '8sum_abs']
        steps = (prop_time,) if steps is None else tuple(steps)
        assert len(steps) >= 1 and all(isinstance(s, int) and not isinstance(s, bool) for s in steps), 'steps are ints'
        assert steps[0] >= 0 and all(b > a for a, b in zip(steps, steps[1:])) and steps[-1] == prop_time, \
            'steps must be strictly increasing, start at >= 0 and end at prop_time'
        self.prop_time = prop_time
        self.prop_kernels = prop_kernels
        self.steps = steps
        self.norm_type = norm_type
        dilations = tuple(dilations) if isinstance(dilations, (tuple, list)) else (dilations,) * len(prop_kernels)
        assert len(dilations) == len(prop_kernels), 'dilations is one int, or one per entry of prop_kernels'
        self.dilations = tuple(F.check_dilation(d) for d in dilations)

    def forward(self, guidances, blur_depth, sparse_depth=None, iter_conf=None, kernel_conf=None, n_iter=None, pin_conf=None):
        if pin_conf is not None and sparse_depth is None:
            raise ValueError("pin_conf needs a sparse_depth: it weights the pin to the measured depth")
        n = self.prop_time if n_iter is None else int(n_iter)
        if n == 0:
            return blur_depth
        nk, T = len(self.prop_kernels), len(self.steps)
        if isinstance(pin_conf, (tuple, list)):
            if len(pin_conf) != nk:
                raise ValueError("pin_conf is one tensor, or a sequence with one entry per kernel size %s" % (self.prop_kernels,))
            pins = [F.widen16(p) for p in pin_conf]
        else:
            pins = [None if pin_conf is None else F.widen16(pin_conf)] * nk
        if len(guidances) != nk or (iter_conf is not None and len(iter_conf) != nk):
            raise ValueError("guidances and iter_conf need one entry per kernel size %s" % (self.prop_kernels,))
        if kernel_conf is not None and (kernel_conf.dim() != 4 or kernel_conf.shape[1] != nk):
            raise ValueError("kernel_conf must be [B,%d,H,W], got %s" % (nk, tuple(kernel_conf.shape)))
        blur_depth, sparse_depth, kernel_conf = F.widen16(blur_depth, sparse_depth, kernel_conf)
        out = None
        for k, K in enumerate(self.prop_kernels):
            conf = F.assemble_conf(None if iter_conf is None else F.widen16(iter_conf[k]), kernel_conf, k, T, blur_depth)
            if pins[k] is None:
                y = _CSPN2dKxKAssembleFunction.apply(guidances[k], blur_depth, sparse_depth, conf, self.steps, K, n, self.norm_type, self.dilations[k])
            else:
                y = _CSPN2dKxKAssemblePinFunction.apply(guidances[k], blur_depth, sparse_depth, pins[k], conf, self.steps, K, n, self.norm_type,
                                                        self.dilations[k])
            out = y if out is None else out + y
        return out

    def extra_repr(self):
        return "prop_time=%d, prop_kernels=%r, steps=%r, norm_type=%r" % (self.prop_time, self.prop_kernels, self.steps, self.norm_type) \
            + (", dilations=%r" % (self.dilations,) if any(d != 1 for d in self.dilations) else "")


class CSPN(nn.Module):
    """reference cspn_paddle/demo.py:10-54 (the demo's module): same constructor, same cspn(guide, feat) -- also the forward.  guide
    [N, feat_chan*K, *S] raw (K = prop_kernel^dim_num - 1; prop_kernel 3, or 5 / 7 in 2D), feat [N, feat_chan, *S]: abs, each channel's
    slice of K gates divided by its abs-sum, prop_step chained propagations (F.absnorm_propagate: one engine call for all channels, the 3D
    normalisation inside the persistent kernel; for prop_kernel 5 / 7 inside the K x K engine's step, F.cspn2d_forward_kxk_absnorm, which
    stores no normalised gate).  A float16 / bfloat16 guide goes to the engine as it is in 3D (cspn3d_forward_absnorm_g16) and for
    prop_kernel 5 / 7, and its gradient comes back in its dtype; 2D 3 x 3 widens it first.  The result is float32.  A port of demo.py changes its
    imports and tensor types, nothing else."""

    def __init__(self, dim_num, feat_chan, prop_kernel, prop_step):
        super(CSPN, self).__init__()
        assert dim_num in (2, 3), 'dim_num must be 2 or 3'   # (demo.py:87)
        assert prop_kernel == 3 or (dim_num == 2 and prop_kernel in (5, 7)), \
            'the neighbourhood is 3 x 3 (x 3), or 5 x 5 / 7 x 7 in 2D'   # (demo.py:90)
        self.dim_num = dim_num
        self.feat_chan = feat_chan
        self.prop_kernel = prop_kernel
        self.prop_step = prop_step

    def cspn(self, guide, feat):
        if feat.dim() != self.dim_num + 2:
            raise ValueError("feat must have %d dimensions for dim_num %d, got %s" % (self.dim_num + 2, self.dim_num, tuple(feat.shape)))
        if self.dim_num == 3 or self.prop_kernel != 3:
            feat = F.widen16(feat)   # the K x K engine and the 3D kernels widen a 16-bit guide where they read it; values are float32
        else:
            guide, feat = F.widen16(guide, feat)   # 2D 3 x 3: the gate_absnorm tensor op has no 16-bit kernel, float32 from here on
        return F.absnorm_propagate(guide, feat, self.prop_step, self.prop_kernel)

    def forward(self, guide, feat):
        return self.cspn(guide, feat)

    def extra_repr(self):
        return "dim_num=%d, feat_chan=%d, prop_kernel=%d, prop_step=%d" % (self.dim_num, self.feat_chan, self.prop_kernel, self.prop_step)
