"""The depth-completion contract of Affinity_Propagate (reference cspn_pytorch/models/cspn.py:42-144) over K x K neighbourhoods,
K = 3, 5 or 7: guidance [B, K*K-1, H, W] normalised by its abs-sum, each gate sited at its neighbour, a (1 - gate_sum) blur term and
sparse depth pinned.  Channel k is the k-th pair (t, l) in raster order over {0..K-1}^2 without the centre; the reference's padding
generalised is ZeroPad2d((l, K-1-l, t, K-1-t)) followed by a crop of K//2 on each side.
CPU: a float64 torch statement written that way reproduces the unmodified reference's outputs and gradients at K = 3 (the goldens), which
ties its K = 5 / 7 form to the reference; exports, header, ABI version, C and Python argument errors, the module's constructor.
GPU: the new entry points against the goldens at K = 3 and against the statement at K = 5 / 7, forward and both gradients, the module."""
import ctypes
import os
import re

import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from helpers import rel_err
from test_backward import NORMS, _check
from test_backward import _golden as _grad_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_kxk_norm_workspace_bytes", "cspn2d_kxk_norm_history_bytes", "cspn2d_forward_kxk_norm_f32",
       "cspn2d_backward_kxk_norm_workspace_bytes", "cspn2d_backward_kxk_norm_f32"]
RTOL = 1e-4


# ---- the float64 torch statement ----
def _pads(K):
    R = K // 2
    return [(l, K - 1 - l, t, K - 1 - t) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def torch_kxk_norm(guidance, blur, sparse, K, n, norm):
    """cspn.py:42-144 with the eight ZeroPad2d tuples generalised to K x K: the gates padded (sited at the neighbour), normalised by
    their abs-sum, the depth padded with the same tuples, the weighted sum cropped by R; blur [B,C,H,W] broadcast over the gates"""
    R = K // 2
    P = _pads(K)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)   # [B,KK,H+2R,W+2R]
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, R:-R, R:-R]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)   # [B,KK,C,H+2R,W+2R]
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, R:-R, R:-R]
        if m is not None:
            x = (1 - m) * x + m * blur
    return x


def _inputs(B, C, H, W, K, sparse, seed):
    """raw signed guidance, depth in [0, 10), a mask of ~10 % with one negative value; sparse None, 1 or C planes"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, K * K - 1, H, W, generator=gen)
    h = torch.rand(B, C, H, W, generator=gen) * 10
    s = None
    if sparse:
        sc = 1 if sparse == "shared" else C
        s = (torch.rand(B, sc, H, W, generator=gen) < 0.1).float() * (torch.rand(B, sc, H, W, generator=gen) * 10 + 0.1)
        s.view(-1)[min(3, s.numel() - 1)] = -2.5
    return g, h, s


def _misaligned(t):
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _cuda(*ts):
    return [t.cuda() if t is not None else None for t in ts]


# ---- CPU ----
def test_statement_at_k3_reproduces_the_reference_forward(golden):
    for name, c in golden.items():
        B, H, W, n, norm = (int(v) for v in c["meta"])
        s = torch.from_numpy(c["sparse"]).double() if "sparse" in c else None
        out = torch_kxk_norm(torch.from_numpy(c["guidance"]).double(), torch.from_numpy(c["blur"]).double(), s, 3, n, NORMS[norm])
        assert rel_err(out.numpy(), c["out"]) <= 1e-5, name


def test_statement_at_k3_reproduces_the_reference_gradients():
    for name, c in _grad_golden():
        B, H, W, n, norm = (int(v) for v in c["meta"])
        g = torch.from_numpy(c["guidance"]).double().requires_grad_(True)
        h = torch.from_numpy(c["blur"]).double().requires_grad_(True)
        s = torch.from_numpy(c["sparse"]).double() if "sparse" in c else None
        torch_kxk_norm(g, h, s, 3, n, NORMS[norm]).backward(torch.from_numpy(c["grad_out"]).double())
        assert rel_err(g.grad.numpy(), c["grad_guidance"]) <= 1e-5, name
        assert _check(g.grad.numpy(), c["grad_guidance"], name) and _check(h.grad.numpy(), c["grad_blur"], name)


def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert {"cspn2d_forward_kxk_norm", "cspn2d_backward_kxk_norm", "Affinity_PropagateKxK"} <= set(cspn_amd.__all__)


def test_byte_counts():
    wsb = _lib.late_symbol("cspn2d_kxk_norm_workspace_bytes")
    hb = _lib.late_symbol("cspn2d_kxk_norm_history_bytes")
    bwb = _lib.late_symbol("cspn2d_backward_kxk_norm_workspace_bytes")
    B, C, H, W = 2, 3, 10, 13
    L = B * C * H * W
    assert hb(B, C, H, W, 5, 4) == 4 * L * 3 and hb(B, C, H, W, 3, 1) == 0 and hb(B, C, H, W, 9, 4) == 0
    for K in (3, 5, 7):
        KK = K * K - 1
        fold = 4 * (B * KK * H * W + L)
        assert wsb(B, C, 0, H, W, K, 1) >= fold and wsb(B, C, 1, H, W, K, 4) >= fold + 2 * 4 * L
        assert wsb(B, C, C, H, W, K, 1) >= 4 * (B * C * KK * H * W + L)   # a mask per channel: one w' per channel
        assert bwb(B, C, 0, H, W, K, 4) >= 2 * fold + 3 * 4 * L and bwb(B, C, 1, H, W, K, 1) >= 2 * fold
    for f in (lambda *a: wsb(*a), lambda *a: bwb(*a)):
        assert f(B, C, 0, H, W, 5, 0) == 0 and f(B, C, 0, H, W, 9, 4) == 0 and f(0, C, 0, H, W, 5, 4) == 0 and f(B, C, 2, H, W, 5, 4) == 0


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    fwd = _lib.late_symbol("cspn2d_forward_kxk_norm_f32")
    bwd = _lib.late_symbol("cspn2d_backward_kxk_norm_f32")
    g, x, s, o, h, w, gg, gx = (ctypes.c_void_p(i << 32) for i in range(1, 9))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    # forward: (guidance, blur, sparse, out, history, history_bytes, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream)
    for K in (1, 2, 4, 9, 0):
        assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, K, 3, 0, w, M, None) == -1 and b"K must be" in err()
    for norm in (2, 3, -1, 7):
        assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, norm, w, M, None) == -1 and b"norm" in err()
    for sc, sp in ((2, s), (4, s), (0, s), (1, None), (3, None), (-1, s)):
        assert fwd(g, x, sp, o, None, 0, 2, 3, sc, 8, 8, 5, 3, 0, w, M, None) == -1 and b"sparse_C" in err()
    assert fwd(None, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"null" in err()
    assert fwd(g, None, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
    assert fwd(g, x, None, None, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
    for B, C, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, -2)):
        assert fwd(g, x, None, o, None, 0, B, C, 0, H, W, 5, 3, 0, w, M, None) == -1 and b"bad shape" in err()
    assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, -1, 0, w, M, None) == -1
    assert fwd(g, x, s, x, None, 0, 2, 1, 1, 8, 8, 7, 3, 1, w, M, None) == -1 and b"alias" in err()
    assert fwd(g, x, s, s, None, 0, 2, 1, 1, 8, 8, 3, 3, 1, w, M, None) == -1 and b"alias" in err()   # out on the mask
    assert fwd(g, x, None, ctypes.c_void_p((1 << 32) + 64), None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1   # out inside the guidance
    assert fwd(g, x, None, o, x, M, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()   # history on the input
    assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, ctypes.c_void_p(g.value + 256), M, None) == -1 and b"alias" in err()
    assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, None, 0, None) == -2 and b"workspace" in err()
    assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, w, 100, None) == -2
    assert fwd(g, x, None, o, h, M, 2, 1, 0, 8, 8, 5, 3, 0, w, 100, None) == -2   # with a history the fold still needs room
    assert fwd(g, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 3, 0, ctypes.c_void_p((6 << 32) + 4), M, None) == -2 and b"aligned" in err()
    assert fwd(g, x, None, o, h, 100, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -2 and b"history" in err()
    assert fwd(g, x, None, o, None, 0, 1 << 12, 1 << 8, 0, 1 << 6, 1 << 6, 5, 3, 0, w, M, None) == -3   # 2^32 elements
    assert fwd(g, x, None, o, None, 0, 1 << 8, 1, 0, 1 << 10, 1 << 8, 7, 3, 0, w, M, None) == -3       # 48 2^26 guidance elements
    assert fwd(g, x, s, o, None, 0, 1 << 8, 4, 4, 1 << 10, 1 << 8, 3, 3, 0, w, M, None) == -3        # per-channel w': 2^31 elements
    assert fwd(g, x, s, o, None, 0, 1 << 8, 4, 1, 1 << 10, 1 << 8, 3, 3, 0, w, 100, None) == -2       # a shared mask: 2^29, within range
    # backward: (guidance, blur, sparse, history, history_bytes, grad_out, grad_guidance, grad_blur, B, C, sparse_C, H, W, K, n_iter,
    #            norm, ws, ws_bytes, stream)
    hbytes = 4 * 2 * 8 * 8 * 2
    assert bwd(g, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 9, 3, 0, w, M, None) == -1 and b"K must be" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 2, w, M, None) == -1 and b"norm" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, gx, 2, 2, 2, 8, 8, 5, 3, 0, w, M, None) == -1 and b"sparse_C" in err()
    assert bwd(None, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"null" in err()
    assert bwd(g, x, None, h, hbytes, None, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1
    assert bwd(g, x, None, None, 0, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"history" in err()
    assert bwd(g, x, None, h, 64, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"history" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, gg, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, o, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert bwd(g, x, None, h, hbytes, o, x, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert bwd(g, x, s, h, hbytes, o, gg, s, 2, 1, 1, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, h, 2, 1, 0, 8, 8, 5, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, None, 0, None) == -2 and b"workspace" in err()
    assert bwd(g, x, None, h, hbytes, o, gg, gx, 2, 1, 0, 8, 8, 5, 3, 0, w, 64, None) == -2
    # the NONE op keeps rejecting K = 3
    assert _lib.late_symbol("cspn2d_forward_kxk_f32")(g, x, o, None, 0, 2, 1, 8, 8, 3, 3, w, M, None) == -1 and b"K must be" in err()


def test_python_argument_errors_without_gpu():
    g5, h, s = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9)
    f = F.cspn2d_forward_kxk_norm
    for ks in (4, 9, 1, 0, True, 5.0):
        with pytest.raises(ValueError, match="kernel_size"):
            f(g5, h, s, ks, 3)
    for nt in ("none", "prenorm", "8SUM", None):
        with pytest.raises(ValueError, match="norm_type"):
            f(g5, h, s, 5, 3, nt)
    with pytest.raises(ValueError, match="n_iter"):
        f(g5, h, s, 5, -1)
    for ks, ch in ((5, 8), (5, 48), (7, 24), (3, 24)):
        with pytest.raises(ValueError, match="guidance"):
            f(torch.rand(1, ch, 6, 9), h, None, ks, 3)
    with pytest.raises(ValueError, match="blur_depth"):
        f(g5, torch.rand(1, 2, 6, 8), None, 5, 3)
    with pytest.raises(ValueError, match="blur_depth"):
        f(g5, torch.rand(2, 2, 6, 9), None, 5, 3)
    for bad in (torch.rand(1, 3, 6, 9), torch.rand(1, 1, 6, 8), torch.rand(1, 6, 9)):
        with pytest.raises(ValueError, match="sparse_depth"):
            f(g5, h, bad, 5, 3)
    with pytest.raises(TypeError):
        f(g5.numpy(), h, None, 5, 3)
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_backward_kxk_norm(g5, h, s, torch.rand(1, 1, 6, 9), 5, 3)
    # well-formed, but on the CPU: the engine is GPU-only and has no CPU path
    with pytest.raises(cspn_amd.CspnError):
        f(g5, h, s, 5, 3)
    with pytest.raises(cspn_amd.CspnError):
        F.cspn2d_backward_kxk_norm(g5, h, s, torch.rand(1, 2, 6, 9), 5, 3)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.Affinity_PropagateKxK(3, 5)(g5, h, s)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.Affinity_PropagateKxK(3, 7, "8sum_abs")(torch.rand(1, 48, 6, 9).requires_grad_(True), h)
    assert f(g5, h, s, 5, 0) is h   # n_iter == 0: the very same tensor
    assert cspn_amd.Affinity_PropagateKxK(0, 5)(g5, h, s) is h
    assert cspn_amd.Affinity_PropagateKxK(24, 7)(g5, h, s, n_iter=0) is h


def test_module_constructor():
    for ks in (3, 5, 7):
        for nt in ("8sum", "8sum_abs"):
            m = cspn_amd.Affinity_PropagateKxK(24, ks, nt)
            assert (m.prop_time, m.prop_kernel, m.norm_type) == (24, ks, nt) and list(m.parameters()) == [] and m.state_dict() == {}
    for ks in (1, 2, 4, 9):
        with pytest.raises(AssertionError):
            cspn_amd.Affinity_PropagateKxK(24, ks)
    for nt in ("none", "abs", "8SUM"):
        with pytest.raises(AssertionError):
            cspn_amd.Affinity_PropagateKxK(24, 5, nt)
    with pytest.raises(AssertionError):   # the 3 x 3 module stays as it is
        cspn_amd.Affinity_Propagate(24, 5)


# ---- GPU ----
@pytest.mark.gpu
def test_k3_entry_points_vs_reference_goldens(golden):
    for name, c in golden.items():
        B, H, W, n, norm = (int(v) for v in c["meta"])
        g, h = torch.from_numpy(c["guidance"]).cuda(), torch.from_numpy(c["blur"]).cuda()
        s = torch.from_numpy(c["sparse"]).cuda() if "sparse" in c else None
        out = F.cspn2d_forward_kxk_norm(g, h, s, 3, n, NORMS[norm])
        assert rel_err(out.cpu().numpy(), c["out"]) <= RTOL, name
    for name, c in _grad_golden():
        B, H, W, n, norm = (int(v) for v in c["meta"])
        t = {k: torch.from_numpy(v).cuda() for k, v in c.items() if k != "meta"}
        out, hist = F.cspn2d_forward_kxk_norm(t["guidance"], t["blur"], t.get("sparse"), 3, n, NORMS[norm], return_history=True)
        assert rel_err(out.cpu().numpy(), c["out"]) <= RTOL, name
        gg, gh = F.cspn2d_backward_kxk_norm(t["guidance"], t["blur"], t.get("sparse"), t["grad_out"], 3, n, NORMS[norm], hist)
        assert _check(gg.cpu().numpy(), c["grad_guidance"], name) and _check(gh.cpu().numpy(), c["grad_blur"], name)


# (B, C, H, W, n, sparse): W % 4 in {0, 1, 2, 3}, images smaller than K, n 1 / 2 / 5 / 24, masks None / [B,1] / [B,C]
CASES = [(2, 1, 11, 14, 6, "shared"), (1, 2, 9, 40, 24, "per"), (2, 3, 13, 33, 5, None), (1, 3, 17, 66, 2, "per"),
         (1, 2, 2, 3, 5, "shared"), (2, 1, 6, 2, 1, None), (1, 1, 20, 67, 24, "shared"), (1, 2, 19, 64, 5, "shared")]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("B,C,H,W,n,sparse", CASES)
def test_forward_and_gradients_vs_fp64_statement(K, norm, B, C, H, W, n, sparse):
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K * 1000 + W * 10 + n)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(n))
    gt, ht = g.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = torch_kxk_norm(gt, ht, s.double() if s is not None else None, K, n, norm)
    ref.backward(go.double())
    gd, hd, sd, god = _cuda(g, h, s, go)
    out, hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True)
    assert rel_err(out.cpu().numpy(), ref.detach().numpy()) <= RTOL
    assert torch.equal(F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm), out)
    gg, gh = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, hist)
    assert _check(gg.cpu().numpy(), gt.grad.numpy(), "dL/dguidance") and _check(gh.cpu().numpy(), ht.grad.numpy(), "dL/dblur")
    # deterministic, and the same without a kept history
    gg2, gh2 = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm)
    assert torch.equal(gg, gg2) and torch.equal(gh, gh2)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("need_guidance,need_blur", [(True, False), (False, True), (True, True), (False, False)])
@pytest.mark.parametrize("sparse", [None, "per"])
def test_gradient_subsets(K, need_guidance, need_blur, sparse):
    B, C, H, W, n, norm = 2, 2, 12, 36, 5, "8sum_abs"
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K + need_guidance * 2 + need_blur)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(5))
    gd, hd, sd, god = _cuda(g, h, s, go)
    full_g, full_h = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm)
    gg, gh = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, need_guidance=need_guidance, need_blur=need_blur)
    assert (gg is None) != need_guidance and (gh is None) != need_blur
    assert gg is None or torch.equal(gg, full_g)
    assert gh is None or torch.equal(gh, full_h)
    # through the module: the gradients autograd asks for
    m = cspn_amd.Affinity_PropagateKxK(n, K, norm)
    gc, hc = gd.clone().requires_grad_(need_guidance), hd.clone().requires_grad_(need_blur)
    y = m(gc, hc, sd)
    assert torch.equal(y.detach(), F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm))
    if need_guidance or need_blur:
        y.backward(god)
        assert (gc.grad is None or torch.equal(gc.grad, full_g)) and (hc.grad is None or torch.equal(hc.grad, full_h))
        assert (gc.grad is not None) == need_guidance and (hc.grad is not None) == need_blur


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("H,W", [(12, 64), (9, 37)])
def test_misaligned_views(K, H, W):
    B, C, n, norm = 2, 2, 5, "8sum"
    g, h, s = _inputs(B, C, H, W, K, "per", seed=K + W)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(2))
    gd, hd, sd, god = _cuda(g, h, s, go)
    out = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm)
    gg, gh = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm)
    gm, hm, sm, gom = (_misaligned(t) for t in (g, h, s, go))
    assert torch.equal(F.cspn2d_forward_kxk_norm(gm, hm, sm, K, n, norm), out)
    gg2, gh2 = F.cspn2d_backward_kxk_norm(gm, hm, sm, gom, K, n, norm)
    assert torch.equal(gg2, gg) and torch.equal(gh2, gh)
    ref = torch_kxk_norm(g.double(), h.double(), s.double(), K, n, norm)
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("C,sparse", [(1, "shared"), (2, "per"), (1, None)])
def test_module_at_k3_is_bitwise_affinity_propagate(norm, C, sparse):
    B, H, W, n = 2, 24, 64, 24
    g, h, s = _inputs(B, C, H, W, 3, sparse, seed=C)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    res = []
    for m in (cspn_amd.Affinity_Propagate(n, 3, norm), cspn_amd.Affinity_PropagateKxK(n, 3, norm)):
        gd, hd = g.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
        y = m(gd, hd, s.cuda() if s is not None else None)
        y.backward(go)
        res.append((y.detach(), gd.grad, hd.grad))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_kitti_full_size_vs_fp32_torch_on_the_gpu():
    B, C, H, W, K, n = 2, 1, 304, 1216, 5, 24
    g, h, s = _cuda(*_inputs(B, C, H, W, K, "shared", seed=1216))
    with torch.no_grad():
        ref = torch_kxk_norm(g, h, s, K, n, "8sum")
        out = cspn_amd.Affinity_PropagateKxK(n, K, "8sum")(g, h, s)
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) <= RTOL
