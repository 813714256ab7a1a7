"""The 2D NONE op over 5 x 5 and 7 x 7 neighbourhoods (fluid.layers.affinity_propagate's kernel_size, reference cspn_paddle/README.md:54-56):
gate [N, K*K-1, H, W] used as given, x [N, C, H, W] on shared gates.  Gate channel k is the k-th pair (t, l) in raster order over {0..K-1}^2
without the centre, neighbour offset (K//2 - t, K//2 - l).  Pinned against a float64 torch statement of that recurrence, whose K = 3 form is
today's 3 x 3 op, and whose autograd gives the reference gradients.
CPU: exports, header, ABI version, C and Python argument errors, the module's constructor.  GPU: forward, C channels, gradients, the
public routes (affinity_propagate, CSPN, gate_absnorm with K = 24 / 48).  The gradient cases here fit one 64 x 16 tile; tile seams and
tile grids that are not square are covered in tests/test_kxk_tilegrid.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_kxk_workspace_bytes", "cspn2d_kxk_history_bytes", "cspn2d_forward_kxk_f32", "cspn2d_backward_kxk_workspace_bytes",
       "cspn2d_backward_kxk_f32"]
RTOL = 1e-4
GFLOOR = 5e-6
GTOL = 2e-4   # the element-wise gradient form of tests/test_absnorm.py


# ---- float64 torch statements ----
def _offsets(K):
    R = K // 2
    return [(R - t, R - l) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def _torch_noneKxK(g, x, K, n):
    """H_{t+1}(p) = sum_k g_k(p) H_t(p + off_k), zero outside, summed in channel order; x [N,C,H,W] on the shared gates g [N,K*K-1,H,W]"""
    R = K // 2
    H, W = x.shape[2:]
    for _ in range(n):
        pad = torch.nn.functional.pad(x, (R, R, R, R))
        acc = 0
        for k, (dy, dx) in enumerate(_offsets(K)):
            acc = acc + g[:, k:k + 1] * pad[:, :, R + dy:R + dy + H, R + dx:R + dx + W]
        x = acc
    return x


def _torch_absnorm(g, K):
    """demo.py:24,34-36,47-49: abs, sum over each channel's K gates, div"""
    N, M = g.shape[:2]
    a = g.abs().reshape(N, M // K, K, *g.shape[2:])
    return (a / a.sum(2, keepdim=True)).reshape(g.shape)


def _torch_module(guide, feat, ks, n):
    """the demo's cspn() in torch: per channel its own slice, normalised, then the recurrence"""
    K = ks * ks - 1
    w = _torch_absnorm(guide, K)
    return torch.cat([_torch_noneKxK(w[:, c * K:(c + 1) * K], feat[:, c:c + 1], ks, n) for c in range(feat.shape[1])], 1)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _check_grad(a, b, what=""):
    from helpers import assert_close
    assert_close(a, b, what, rtol=GTOL, atol_frac=GFLOOR)


def _gates(N, K, H, W, seed):
    """signed, unnormalised gates whose abs-sum stays near 1, so that 30 steps keep the values in range"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(N, K * K - 1, H, W, generator=gen) * (1.2 / (K * K - 1))


def _values(N, C, H, W, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand(N, C, H, W, generator=gen) * 4 - 1


def _misaligned(t):
    """a device copy of t whose storage starts 1 float after a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


# ---- CPU ----
def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert {"cspn2d_forward_kxk", "cspn2d_backward_kxk"} <= set(cspn_amd.__all__)


def test_byte_counts():
    wsb = _lib.late_symbol("cspn2d_kxk_workspace_bytes")
    hb = _lib.late_symbol("cspn2d_kxk_history_bytes")
    bwb = _lib.late_symbol("cspn2d_backward_kxk_workspace_bytes")
    L = 2 * 3 * 10 * 13
    assert hb(2, 3, 10, 13, 5, 4) == 4 * L * 3 and hb(2, 3, 10, 13, 7, 1) == 0
    assert wsb(2, 3, 10, 13, 5, 4) >= 2 * 4 * L and wsb(2, 3, 10, 13, 5, 2) >= 4 * L and wsb(2, 3, 10, 13, 5, 1) == 0
    assert bwb(2, 3, 10, 13, 7, 4) >= 4 * L * 3 and bwb(2, 3, 10, 13, 7, 1) == 0
    for f in (wsb, hb, bwb):
        assert f(2, 3, 10, 13, 3, 4) == 0 and f(2, 3, 10, 13, 9, 4) == 0 and f(0, 3, 10, 13, 5, 4) == 0


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    fwd = _lib.late_symbol("cspn2d_forward_kxk_f32")
    bwd = _lib.late_symbol("cspn2d_backward_kxk_f32")
    g, x, o, h, w, gg, gx = (ctypes.c_void_p(i << 32) for i in range(1, 8))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    # forward: (gate, x, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    for K in (3, 4, 9, 0):
        assert fwd(g, x, o, None, 0, 2, 1, 8, 8, K, 3, w, 1 << 20, None) == -1 and b"K must be" in err()
    assert fwd(None, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"null" in err()
    assert fwd(g, None, o, None, 0, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1
    assert fwd(g, x, None, None, 0, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1
    for B, C, H, W in ((0, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (-1, 1, 8, 8)):
        assert fwd(g, x, o, None, 0, B, C, H, W, 5, 3, w, 1 << 20, None) == -1 and b"bad shape" in err()
    assert fwd(g, x, o, None, 0, 2, 1, 8, 8, 5, -1, w, 1 << 20, None) == -1
    assert fwd(g, x, x, None, 0, 2, 1, 8, 8, 7, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert fwd(g, x, g, None, 0, 2, 1, 8, 8, 7, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert fwd(g, x, ctypes.c_void_p((1 << 32) + 64), None, 0, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1   # out inside the gates
    assert fwd(g, x, o, x, 1 << 20, 2, 1, 8, 8, 5, 3, None, 0, None) == -1 and b"alias" in err()   # history on the input
    assert fwd(g, x, o, None, 0, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"workspace" in err()
    assert fwd(g, x, o, None, 0, 2, 1, 8, 8, 5, 3, w, 100, None) == -2
    assert fwd(g, x, o, None, 0, 2, 1, 8, 8, 5, 3, ctypes.c_void_p((6 << 32) + 4), 1 << 20, None) == -2 and b"aligned" in err()
    assert fwd(g, x, o, h, 100, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"history" in err()
    assert fwd(g, x, o, None, 0, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, 1 << 20, None) == -3   # 2^32 elements
    assert fwd(g, x, o, None, 0, 1 << 8, 1, 1 << 10, 1 << 8, 7, 3, w, 1 << 20, None) == -3       # 48 2^26 gate elements
    # backward: (gate, x, history, history_bytes, grad_out, grad_gate, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    hbytes = 4 * 2 * 8 * 8 * 2
    assert bwd(g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 9, 3, w, 1 << 20, None) == -1 and b"K must be" in err()
    assert bwd(None, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"null" in err()
    assert bwd(g, x, h, hbytes, None, gg, gx, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1
    assert bwd(g, x, h, hbytes, o, gg, gx, 2, 1, 0, 8, 5, 3, w, 1 << 20, None) == -1
    assert bwd(g, x, None, 0, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"history" in err()
    assert bwd(g, x, h, 64, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"history" in err()
    assert bwd(g, x, h, hbytes, o, gg, gg, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert bwd(g, x, h, hbytes, o, gg, o, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert bwd(g, x, h, hbytes, o, x, gx, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert bwd(g, x, h, hbytes, o, gg, h, 2, 1, 8, 8, 5, 3, w, 1 << 20, None) == -1 and b"alias" in err()
    assert bwd(g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, None, 0, None) == -2 and b"workspace" in err()
    assert bwd(g, x, h, hbytes, o, gg, gx, 2, 1, 8, 8, 5, 3, w, 64, None) == -2
    # the gate normaliser takes K = 24 and 48 (past the K check: the aliasing is what it reports), K = 9 and 7 stay errors
    norm = _lib.late_symbol("cspn_gate_absnorm_f32")
    back = _lib.late_symbol("cspn_gate_absnorm_backward_f32")
    for K in (24, 48):
        assert norm(g, g, 2, K, 64, None) == -1 and b"alias" in err()
        assert back(g, x, g, 2, K, 64, None) == -1 and b"alias" in err()
    assert norm(g, x, 2, 9, 64, None) == -1 and b"K must be" in err()
    assert back(g, x, o, 1, 7, 16, None) == -1 and b"K must be" in err()


def test_python_argument_errors_without_gpu():
    x, g5 = torch.rand(1, 2, 6, 9), torch.rand(1, 24, 6, 9)
    with pytest.raises(ValueError, match="2D only"):
        cspn_amd.affinity_propagate(torch.rand(1, 1, 3, 6, 9), torch.rand(1, 124, 3, 6, 9), 5, 2)
    for ks in (4, 6, 2, 1, 0, 9, 11, -3):
        with pytest.raises(ValueError, match="kernel_size"):
            cspn_amd.affinity_propagate(x, g5, ks, 2)
    for ks, ch in ((5, 8), (5, 48), (7, 24), (7, 49)):
        with pytest.raises(ValueError, match="channels"):
            cspn_amd.affinity_propagate(x, torch.rand(1, ch, 6, 9), ks, 2)
    with pytest.raises(cspn_amd.CspnError):   # well-formed, but on the CPU: the engine is GPU-only
        cspn_amd.affinity_propagate(x, g5, 5, 2)
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk(g5, x, 3, 2)
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk(g5, x, 7, 2)
    with pytest.raises(ValueError):
        F.cspn2d_backward_kxk(g5, x, torch.rand(1, 2, 6, 8), 5, 2)
    with pytest.raises(ValueError):
        cspn_amd.absnorm_propagate(torch.rand(1, 124, 2, 4, 8), torch.rand(1, 1, 2, 4, 8), 3, kernel_size=5)
    with pytest.raises(ValueError):
        cspn_amd.absnorm_propagate(torch.rand(1, 48, 4, 8), torch.rand(1, 1, 4, 8), 3, kernel_size=5)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.absnorm_propagate(torch.rand(1, 48, 4, 8), torch.rand(1, 2, 4, 8), 3, kernel_size=5)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.gate_absnorm(torch.rand(1, 48, 4, 8), 48)
    with pytest.raises(ValueError):
        cspn_amd.gate_absnorm(torch.rand(1, 47, 4, 8), 48)
    assert cspn_amd.affinity_propagate(x, g5, 5, 0) is x   # n_iter == 0: the very same tensor
    assert F.cspn2d_forward_kxk(g5, x, 5, 0) is x


def test_module_takes_5x5_and_7x7_in_2d_only():
    for ks in (5, 7):
        m = cspn_amd.CSPN(2, 1, ks, 4)
        assert (m.dim_num, m.feat_chan, m.prop_kernel, m.prop_step) == (2, 1, ks, 4) and list(m.parameters()) == []
        g, x = torch.rand(1, ks * ks - 1, 4, 8), torch.rand(1, 1, 4, 8)
        with pytest.raises(cspn_amd.CspnError):
            m(g, x)
        with pytest.raises(ValueError):   # 8 gates is the 3 x 3 module's guide
            m(torch.rand(1, 8, 4, 8), x)
        assert cspn_amd.CSPN(2, 1, ks, 0)(g, x) is x
    for args in ((3, 1, 5, 12), (3, 1, 7, 12), (2, 1, 9, 4), (2, 1, 4, 4), (4, 1, 3, 12)):
        with pytest.raises(AssertionError):
            cspn_amd.CSPN(*args)


def test_reference_at_k3_is_todays_3x3_op():
    from test_absnorm import _torch_none2d
    gen = torch.Generator().manual_seed(3)
    g = torch.randn(2, 8, 7, 11, generator=gen, dtype=torch.float64) / 6
    x = torch.rand(2, 1, 7, 11, generator=gen, dtype=torch.float64)
    assert torch.equal(_torch_noneKxK(g, x, 3, 5), _torch_none2d(g, x, 5))


# ---- GPU ----
FWD_CASES = [(1, 1, 3, 4, 5), (2, 1, 4, 6, 24), (1, 2, 9, 33, 30), (2, 1, 13, 64, 5), (1, 1, 17, 65, 24), (2, 1, 11, 66, 1),
             (1, 1, 20, 67, 5), (1, 1, 6, 2, 30), (1, 1, 2, 130, 5), (1, 1, 40, 1216, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("N,C,H,W,n", FWD_CASES)
def test_forward_vs_fp64_torch(K, N, C, H, W, n):
    """H or W < K, odd widths, W % 4 in {0, 1, 2, 3}, a KITTI-width row, n_iter 1 .. 30, signed unnormalised gates"""
    g = _gates(N, K, H, W, seed=K * 100 + W + n)
    x = _values(N, C, H, W, seed=H + n)
    ref = _torch_noneKxK(g.double(), x.double(), K, n)
    out = F.cspn2d_forward_kxk(g.cuda(), x.cuda(), K, n)
    assert out.shape == x.shape
    assert _rel(out.cpu(), ref) <= RTOL
    out_h, hist = F.cspn2d_forward_kxk(g.cuda(), x.cuda(), K, n, return_history=True)
    assert torch.equal(out_h, out)
    if n >= 2:   # the kept levels are H_1 .. H_{n-1}
        lv = hist.view(n - 1, N, C, H, W)
        assert _rel(lv[n - 2].cpu(), _torch_noneKxK(g.double(), x.double(), K, n - 1)) <= RTOL
        assert _rel(lv[0].cpu(), _torch_noneKxK(g.double(), x.double(), K, 1)) <= RTOL


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("H,W", [(12, 64), (9, 37)])
def test_misaligned_views(K, H, W):
    g = _gates(2, K, H, W, seed=K + W)
    x = _values(2, 2, H, W, seed=W)
    n = 5
    ref = _torch_noneKxK(g.double(), x.double(), K, n)
    aligned = F.cspn2d_forward_kxk(g.cuda(), x.cuda(), K, n)
    gm, xm = _misaligned(g), _misaligned(x)
    out = F.cspn2d_forward_kxk(gm, xm, K, n)
    assert _rel(out.cpu(), ref) <= RTOL and torch.equal(out, aligned)
    go = _values(2, 2, H, W, seed=1).cuda()
    ga, gxa = F.cspn2d_backward_kxk(g.cuda(), x.cuda(), go, K, n)
    gb, gxb = F.cspn2d_backward_kxk(gm, xm, _misaligned(go.cpu()), K, n)
    assert torch.equal(ga, gb) and torch.equal(gxa, gxb)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
def test_channels_share_the_gates(K):
    N, H, W, n = 2, 19, 70, 6
    g = _gates(N, K, H, W, seed=K).cuda()
    x = _values(N, 3, H, W, seed=K + 1).cuda()
    out = F.cspn2d_forward_kxk(g, x, K, n)
    for c in range(3):
        assert torch.equal(out[:, c:c + 1], F.cspn2d_forward_kxk(g, x[:, c:c + 1].contiguous(), K, n))
    assert torch.equal(cspn_amd.affinity_propagate(x, g, K, n), out)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("N,C,H,W,n", [(2, 1, 9, 13, 4), (1, 3, 16, 64, 6), (2, 2, 5, 6, 1), (1, 1, 12, 34, 24)])
@pytest.mark.parametrize("which", ["gate", "x", "both"])
def test_gradients_vs_fp64_autograd(K, N, C, H, W, n, which):
    g = _gates(N, K, H, W, seed=K + H + n)
    x = _values(N, C, H, W, seed=W + C)
    go = _values(N, C, H, W, seed=7)
    gt, xt = g.double().requires_grad_(which != "x"), x.double().requires_grad_(which != "gate")
    _torch_noneKxK(gt, xt, K, n).backward(go.double())
    gg, gx = F.cspn2d_backward_kxk(g.cuda(), x.cuda(), go.cuda(), K, n, need_gate=which != "x", need_x=which != "gate")
    if which != "x":
        _check_grad(gg.cpu().numpy(), gt.grad.numpy(), "dL/dgate K=%d" % K)   # summed over the C channels
    else:
        assert gg is None
    if which != "gate":
        _check_grad(gx.cpu().numpy(), xt.grad.numpy(), "dL/dx K=%d" % K)
    else:
        assert gx is None
    # deterministic: a second call is bitwise equal
    gg2, gx2 = F.cspn2d_backward_kxk(g.cuda(), x.cuda(), go.cuda(), K, n, need_gate=which != "x", need_x=which != "gate")
    for a, b in ((gg, gg2), (gx, gx2)):
        assert (a is None and b is None) or torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("C", [1, 2])
def test_affinity_propagate_under_autograd(K, C):
    N, H, W, n = 2, 14, 40, 5
    g = _gates(N, K, H, W, seed=K * C)
    x = _values(N, C, H, W, seed=C)
    go = _values(N, C, H, W, seed=11)
    gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
    (_torch_noneKxK(gt, xt, K, n) * go.double()).sum().backward()
    gc, xc = g.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    y = cspn_amd.affinity_propagate(xc, gc, kernel_size=K, n_iter=n)
    assert y.grad_fn is not None and _rel(y.detach().cpu(), _torch_noneKxK(g.double(), x.double(), K, n)) <= RTOL
    (y * go.cuda()).sum().backward()
    _check_grad(gc.grad.cpu().numpy(), gt.grad.numpy(), "dL/dgate_weight")
    _check_grad(xc.grad.cpu().numpy(), xt.grad.numpy(), "dL/dinput")
    with torch.no_grad():
        assert torch.equal(cspn_amd.affinity_propagate(xc, gc, K, n), y.detach())
    assert cspn_amd.affinity_propagate(xc, gc, K, 0) is xc


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [5, 7])
@pytest.mark.parametrize("offset", [0, 1])
def test_gate_absnorm_24_48_vs_fp64_torch(ks, offset):
    K = ks * ks - 1
    shape = (2, 2 * K, 7, 9) if offset else (2, K, 8, 12)
    gen = torch.Generator().manual_seed(K + offset)
    g = torch.randn(*shape, generator=gen)
    g.view(shape[0], shape[1], -1)[0, :, 3] = 0.   # an all-zero pixel: NaN, as torch's 0 / 0
    gw = torch.randn(*shape, generator=gen)
    gd = _misaligned(g) if offset else g.cuda()
    gwd = _misaligned(gw) if offset else gw.cuda()
    w = cspn_amd.gate_absnorm(gd, K).cpu()
    ref = _torch_absnorm(g.double(), K)
    assert torch.equal(torch.isnan(w), torch.isnan(ref)) and bool(torch.isnan(ref).any())
    ok = ~torch.isnan(ref)
    assert float((w.double()[ok] - ref[ok]).abs().max()) <= 1e-6
    gt = g.double().requires_grad_(True)
    _torch_absnorm(gt, K).backward(gw.double())
    dg = F.gate_absnorm_backward(gd, gwd, K).cpu()
    assert torch.equal(torch.isnan(dg), torch.isnan(gt.grad))
    ok = ~torch.isnan(gt.grad)
    _check_grad(dg.double()[ok].numpy(), gt.grad[ok].numpy(), "dL/dguide K=%d" % K)


@pytest.mark.gpu
@pytest.mark.parametrize("ks", [5, 7])
@pytest.mark.parametrize("C", [1, 2])
def test_cspn_module_vs_fp64_torch(ks, C):
    K = ks * ks - 1
    N, H, W, n = 2, 12, 36, 6
    gen = torch.Generator().manual_seed(ks + C)
    g = (torch.rand(N, C * K, H, W, generator=gen) + 0.05) * torch.sign(torch.randn(N, C * K, H, W, generator=gen))
    x = torch.rand(N, C, H, W, generator=gen)
    go = torch.randn(N, C, H, W, generator=gen)
    gt, xt = g.double().requires_grad_(True), x.double().requires_grad_(True)
    ref = _torch_module(gt, xt, ks, n)
    ref.backward(go.double())
    m = cspn_amd.CSPN(2, C, ks, n)
    with torch.no_grad():
        out = m(g.cuda(), x.cuda())
    assert _rel(out.cpu(), ref.detach()) <= 1e-5
    gc, xc = g.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    y = m.cspn(gc, xc)
    assert y.grad_fn is not None and torch.equal(y.detach(), out)
    y.backward(go.cuda())
    _check_grad(gc.grad.cpu().numpy(), gt.grad.numpy(), "dL/dguide")
    _check_grad(xc.grad.cpu().numpy(), xt.grad.numpy(), "dL/dfeat")
