"""C channels of blur_depth on shared 2D guidance (reference cspn_pytorch/models/cspn.py:58-81 multiplies and broadcasts, so a
blur_depth [B,C,H,W] is propagated channel by channel on the same normalised affinities and dL/dguidance is the sum over the
channels): the cspn2d_*_multi entry points, cspn_amd.Affinity_Propagate, propagate_prenorm and the 2D affinity_propagate.
CPU tests check the argument handling of the C ABI; the GPU tests hold the multi-channel calls to a per-channel loop of the
single-channel calls and to the float64 oracles."""
import ctypes

import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from helpers import rel_err
from oracle import cspn2d_oracle
from oracle.backward import cspn2d_backward_oracle

KITTI = (304, 1216)


def _sym(name):
    return _lib.late_symbol(name)


# ---- CPU: the C ABI ---------------------------------------------------------------------------------------------------------
def test_multi_sizes_follow_the_single_channel_sizes():
    lib = cspn_amd.load()
    H, W = KITTI
    assert _sym("cspn2d_workspace_bytes_multi")(8, 1, H, W, 24) == lib.cspn2d_workspace_bytes(8, H, W, 24)
    assert _sym("cspn2d_backward_multi_workspace_bytes")(8, 1, H, W, 24) == lib.cspn2d_backward_workspace_bytes(8, H, W, 24)
    assert _sym("cspn2d_history_bytes_multi")(8, 1, H, W, 24) == lib.cspn2d_history_bytes(8, H, W, 24)
    # the history of C channels: checkpoints and folded planes per image-channel
    assert _sym("cspn2d_history_bytes_multi")(8, 4, H, W, 24) == lib.cspn2d_history_bytes(32, H, W, 24) > 0
    assert _sym("cspn2d_history_bytes_multi")(2, 3, 40, 72, 24) == 0            # narrow: no history mode
    assert _sym("cspn2d_backward_history_multi_workspace_bytes")(8, 4, H, W, 24) > 0
    assert _sym("cspn2d_workspace_bytes_multi")(8, 4, H, W, 0) == 0


def test_multi_supported():
    H, W = KITTI
    ok = _sym("cspn2d_multi_supported")
    assert ok(8, 4, H, W, 24) and ok(8, 4, H, W, 7) and ok(64, 2, H, W, 30)
    assert not ok(8, 4, H, 1218, 24)      # W % 4 != 0: the library loops over the channels
    assert not ok(2, 3, 40, 200, 24)      # narrower than a band
    assert not ok(8, 0, H, W, 24) and not ok(8, 4, H, W, 0)
    assert not ok(4096, 16, H, W, 24)     # B*C*H*W beyond 32-bit plane indexing


def test_multi_argument_errors_before_the_device():
    fwd = _sym("cspn2d_forward_multi_f32")
    bwd = _sym("cspn2d_backward_multi_f32")
    p = ctypes.c_void_p(256)   # never dereferenced: every call below fails its argument checks first
    H, W = KITTI
    # C = 0
    assert fwd(p, p, None, p, 2, 0, 1, H, W, 24, 0, 0, p, 1 << 30, None) == -1
    assert bwd(p, p, None, p, p, p, 2, 0, 1, H, W, 24, 0, p, 1 << 30, None) == -1
    # a mask of neither 1 nor C channels
    assert fwd(p, p, p, p, 2, 3, 2, H, W, 24, 0, 0, p, 1 << 30, None) == -1
    assert bwd(p, p, p, p, p, p, 2, 3, 2, H, W, 24, 0, p, 1 << 30, None) == -1
    assert b"channels" in cspn_amd.load().cspn_last_error()
    # the 32-bit plane guard applies to B*C*H*W
    assert fwd(p, p, None, p, 4096, 16, 1, H, W, 24, 0, 0, p, 1 << 30, None) == -3
    assert bwd(p, p, None, p, p, p, 4096, 16, 1, H, W, 24, 0, p, 1 << 30, None) == -3
    # a workspace below the size the call needs
    need = _sym("cspn2d_workspace_bytes_multi")(2, 3, H, W, 24)
    assert fwd(p, p, None, p, 2, 3, 1, H, W, 24, 0, 0, p, need - 1, None) == -2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _inputs(B, C, H, W, seed=0, sparse=None, neg=False):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, 8, H, W, generator=gen)
    h = torch.rand(B, C, H, W, generator=gen) * 10
    s = None
    if sparse is not None:
        sc = 1 if sparse == "shared" else C
        m = (torch.rand(B, sc, H, W, generator=gen) < 0.05).float()
        s = m * (torch.rand(B, sc, H, W, generator=gen) * 10 + 0.1)
        if neg:
            s.view(-1)[5] = -2.5
    return g, h, s


def _dev(*ts):
    return [t.cuda() if t is not None else None for t in ts]


def _chan(s, c):
    if s is None:
        return None
    return s[:, c:c + 1].contiguous() if s.shape[1] > 1 else s


def _loop_forward(g, h, s, n, norm, algo):
    return torch.cat([F.cspn2d_forward(g, h[:, c:c + 1].contiguous(), _chan(s, c), n, norm, algo) for c in range(h.shape[1])], 1)


def _loop_backward(g, h, s, go, n, norm):
    gg, gh = None, []
    for c in range(h.shape[1]):
        a, b = F.cspn2d_backward(g, h[:, c:c + 1].contiguous(), _chan(s, c), go[:, c:c + 1].contiguous(), n, norm)
        gg = a if gg is None else gg + a
        gh.append(b)
    return gg, torch.cat(gh, 1)


def _rel(a, b):
    return rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [None, "shared", "per_channel"])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("B,C,H,W,n", [(2, 3, 11, 13, 5), (1, 2, 16, 272, 24), (1, 2, 16, 272, 12), (1, 3, 20, 264, 7)])
def test_affinity_propagate_multichannel_vs_float64_oracle(B, C, H, W, n, norm, sparse):
    """the drop-in module with blur_depth [B,C,H,W]: forward and both gradients against the float64 oracle channel by channel
    (on the parent tree this call raised ValueError)"""
    g, h, s = _inputs(B, C, H, W, seed=B * 100 + C + n, sparse=sparse, neg=sparse is not None)
    gd, hd, sd = _dev(g, h, s)
    gd.requires_grad_(True)
    hd.requires_grad_(True)
    m = cspn_amd.Affinity_Propagate(n, 3, norm)
    out = m(gd, hd, sd)
    assert out.shape == (B, C, H, W)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(7))
    out.backward(go.cuda())
    ref_gg = np.zeros((B, 8, H, W))
    for c in range(C):
        sc = None if s is None else (s[:, c:c + 1] if s.shape[1] > 1 else s)
        ref = cspn2d_oracle(g, h[:, c:c + 1], sc, n, norm)
        assert rel_err(out[:, c:c + 1].detach().cpu().numpy(), ref) <= 1e-4
        _, rgg, rgh = cspn2d_backward_oracle(g.numpy(), h[:, c:c + 1].numpy(), None if sc is None else sc.numpy(), go[:, c:c + 1].numpy(), n, norm,
                                          dtype=np.float64)
        ref_gg += rgg
        assert rel_err(hd.grad[:, c:c + 1].cpu().numpy(), rgh) <= 1e-4
    assert rel_err(gd.grad.cpu().numpy(), ref_gg) <= 1e-4


@pytest.mark.gpu
def test_multi_supported_for_the_benchmarked_shape():
    assert cspn_amd.cspn2d_multi_supported(8, 4, *KITTI, 24)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["auto", "fused", "stepwise", "fused_cxx"])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs", "none", "prenorm"])
def test_forward_multi_equals_the_channel_loop_at_kitti(norm, algo):
    B, C = 8, 4
    H, W = KITTI
    for sparse in (None, "shared", "per_channel"):
        g, h, s = _dev(*_inputs(B, C, H, W, seed=3, sparse=sparse, neg=True))
        if norm in ("none", "prenorm"):
            g = F.cspn2d_normalize(g, "8sum")
        for n in (1, 7, 12, 24, 30):
            a = F.cspn2d_forward_multi(g, h, s, n, norm, algo)
            b = _loop_forward(g, h, s, n, norm, algo)
            assert _rel(a, b) <= 1e-6, (sparse, n)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "none"])
def test_forward_multi_fused_padded_equals_the_channel_loop(norm):
    B, C, H, W = 4, 3, 64, 1218
    for sparse in (None, "shared", "per_channel"):
        g, h, s = _dev(*_inputs(B, C, H, W, seed=5, sparse=sparse))
        if norm == "none":
            g = F.cspn2d_normalize(g, "8sum")
        for n in (7, 24):
            a = F.cspn2d_forward_multi(g, h, s, n, norm, "fused_padded")
            b = _loop_forward(g, h, s, n, norm, "fused_padded")
            assert _rel(a, b) <= 1e-6, (sparse, n)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs", "none", "prenorm"])
@pytest.mark.parametrize("n", [24, 12, 7])
@pytest.mark.parametrize("shape", [(2, 3) + KITTI, (2, 2, 40, 72)])
def test_backward_multi_equals_the_channel_loop(shape, n, norm):
    B, C, H, W = shape
    for sparse in (None, "shared", "per_channel"):
        g, h, s = _dev(*_inputs(B, C, H, W, seed=11, sparse=sparse, neg=True))
        if norm in ("none", "prenorm"):
            g = F.cspn2d_normalize(g, "8sum")
        go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(2)).cuda()
        gg, gh = F.cspn2d_backward_multi(g, h, s, go, n, norm)
        rg, rh = _loop_backward(g, h, s, go, n, norm)
        tol = 1e-5
        assert float((gg - rg).abs().max()) <= tol * float(rg.abs().max()), (sparse,)
        assert float((gh - rh).abs().max()) <= tol * float(rh.abs().max()), (sparse,)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs", "prenorm"])
@pytest.mark.parametrize("sparse", [None, "shared", "per_channel"])
@pytest.mark.parametrize("n", [24, 12])
def test_training_mode_multi_is_bitwise_the_recomputing_path(n, sparse, norm):
    B, C = 2, 4
    H, W = KITTI
    g, h, s = _dev(*_inputs(B, C, H, W, seed=31, sparse=sparse, neg=True))
    if norm == "prenorm":
        g = F.cspn2d_normalize(g, "8sum")
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(9)).cuda()
    out_h, hist = F.cspn2d_forward_with_history_multi(g, h, s, n, norm)
    out = F.cspn2d_forward_multi(g, h, s, n, norm)
    # (as for one channel: the plain forward streams the linear plan, the history forward band groups -- another summation order)
    assert float((out_h - out).abs().max()) <= 4e-6 * float(out.abs().max())
    a = F.cspn2d_backward_from_history_multi(g, h, s, go, hist, n, norm)
    b = F.cspn2d_backward_multi(g, h, s, go, n, norm)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
def test_module_training_step_uses_the_history_and_matches_eval_gradients():
    B, C = 2, 3
    H, W = KITTI
    g, h, s = _dev(*_inputs(B, C, H, W, seed=41, sparse="shared"))
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    grads = []
    for keep in (True, False):
        m = cspn_amd.Affinity_Propagate(24, 3, "8sum")
        m.keep_history = keep
        gd, hd = g.clone().requires_grad_(True), h.clone().requires_grad_(True)
        m(gd, hd, s).backward(go)
        grads.append((gd.grad, hd.grad))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


@pytest.mark.gpu
def test_c1_through_the_multi_entry_points_is_bitwise_the_single_channel_call():
    B, H, W = 2, 64, 512
    g, h, s = _dev(*_inputs(B, 1, H, W, seed=51, sparse="per_channel"))
    go = torch.randn(B, 1, H, W).cuda()
    for n in (7, 24):
        assert torch.equal(F.cspn2d_forward_multi(g, h, s, n), F.cspn2d_forward(g, h, s, n))
        a, b = F.cspn2d_backward_multi(g, h, s, go, n), F.cspn2d_backward(g, h, s, go, n)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    o1, h1 = F.cspn2d_forward_with_history_multi(g, h, s, 24)
    o2, h2 = F.cspn2d_forward_with_history(g, h, s, 24)
    assert torch.equal(o1, o2)
    a = F.cspn2d_backward_from_history_multi(g, h, s, go, h1, 24)
    b = F.cspn2d_backward_from_history(g, h, s, go, h2, 24)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 3, 40, 288), (1, 2, 17, 30)])
def test_affinity_propagate_2d_multichannel(shape):
    B, C, H, W = shape
    g, h, _ = _inputs(B, C, H, W, seed=61)
    gate = (g.abs() / g.abs().sum(1, keepdim=True)).cuda()
    x = h.cuda()
    go = torch.randn(B, C, H, W).cuda()
    for n in (1, 3, 24):
        gt, xt = gate.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out = cspn_amd.affinity_propagate(xt, gt, 3, n)
        ref = torch.cat([F.cspn2d_forward(gate, x[:, c:c + 1].contiguous(), None, n, "none") for c in range(C)], 1)
        assert _rel(out, ref) <= 1e-6
        with torch.no_grad():
            assert _rel(cspn_amd.affinity_propagate(x, gate, 3, n), ref) <= 1e-6
        out.backward(go)
        rg, rh = _loop_backward(gate, x, None, go, n, "none")
        assert float((gt.grad - rg).abs().max()) <= 1e-5 * float(rg.abs().max())
        assert float((xt.grad - rh).abs().max()) <= 1e-5 * float(rh.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [None, "shared", "per_channel"])
def test_propagate_prenorm_multichannel(sparse):
    B, C = 2, 3
    H, W = 48, 520
    g, h, s = _dev(*_inputs(B, C, H, W, seed=71, sparse=sparse))
    wb = F.cspn2d_normalize(g, "8sum").requires_grad_(True)
    hd = h.clone().requires_grad_(True)
    go = torch.randn(B, C, H, W).cuda()
    out = cspn_amd.propagate_prenorm(wb, hd, s, 24)
    assert _rel(out, _loop_forward(wb.detach(), h, s, 24, "prenorm", "auto")) <= 1e-6
    out.backward(go)
    rg, rh = _loop_backward(wb.detach(), h, s, go, 24, "prenorm")
    assert float((wb.grad - rg).abs().max()) <= 1e-5 * float(rg.abs().max())
    assert float((hd.grad - rh).abs().max()) <= 1e-5 * float(rh.abs().max())


@pytest.mark.gpu
def test_module_rejects_mismatched_sparse_channels():
    g, h, _ = _dev(*_inputs(1, 3, 16, 260, seed=81))
    s = torch.zeros(1, 2, 16, 260, device="cuda")
    m = cspn_amd.Affinity_Propagate(24, 3, "8sum")
    with pytest.raises(ValueError):
        m(g, h, s)
    with pytest.raises(ValueError):
        m(g, h[:, :, :, :-1], None)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2])
def test_merged_autograd_functions_are_bitwise_the_public_functional_calls(C):
    """The one autograd Function behind Affinity_Propagate (one channel and C > 1, with and without the kept history) and the one behind the
    3 x 3 affinity_propagate against the public functional call each path stands for: the same engine calls, so no tolerance.  The forward
    that keeps a history is compared with cspn2d_forward_with_history[_multi], whose output differs from the plain forward's in the
    summation order (test_training_mode_multi_is_bitwise_the_recomputing_path)."""
    sfx = "_multi" if C > 1 else ""
    fn = lambda name: getattr(F, name + sfx)   # noqa: E731
    for (B, H, W), has_history in (((2, 64, 512), True), ((1, 17, 30), False)):
        hb = F.cspn2d_history_bytes_multi(B, C, H, W, 24) if C > 1 else F.cspn2d_history_bytes(B, H, W, 24)
        assert (hb > 0) == has_history
        for sparse in (None, "shared"):
            g, h, s = _dev(*_inputs(B, C, H, W, seed=91, sparse=sparse))
            go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5)).cuda()
            for keep in (True, False):
                m = cspn_amd.Affinity_Propagate(24, 3)
                m.keep_history = keep
                gd, hd = g.clone().requires_grad_(True), h.clone().requires_grad_(True)
                out = m(gd, hd, s)
                out.backward(go)
                if keep and has_history:
                    ref, hist = fn("cspn2d_forward_with_history")(g, h, s, 24, "8sum")
                    rg, rh = fn("cspn2d_backward_from_history")(g, h, s, go, hist, 24, "8sum")
                else:
                    ref = fn("cspn2d_forward")(g, h, s, 24, "8sum")
                    rg, rh = fn("cspn2d_backward")(g, h, s, go, 24, "8sum")
                assert torch.equal(out, ref) and torch.equal(gd.grad, rg) and torch.equal(hd.grad, rh)
    if C == 1:
        return
    # the NONE op on C = 2 channels, 2D and 3D: the merged Function calls the multi-channel backward
    for shape, K, backward in (((2, 2, 17, 30), 8, lambda gate, x, go, n: F.cspn2d_backward_multi(gate, x, None, go, n, "none")),
                               ((1, 2, 4, 8, 8), 26, F.cspn3d_backward_multi)):
        gen = torch.Generator().manual_seed(93)
        gate = torch.rand(shape[0], K, *shape[2:], generator=gen)
        gate = (gate / gate.sum(1, keepdim=True)).cuda()
        x = torch.rand(*shape, generator=gen).cuda()
        go = torch.randn(*shape, generator=gen).cuda()
        for n in (1, 3):
            gt, xt = gate.clone().requires_grad_(True), x.clone().requires_grad_(True)
            cspn_amd.affinity_propagate(xt, gt, 3, n).backward(go)
            rg, rx = backward(gate, x, go, n)
            assert torch.equal(gt.grad, rg) and torch.equal(xt.grad, rx)
