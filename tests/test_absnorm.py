"""The demo's CSPN module (reference cspn_paddle/demo.py:20-54): abs, each channel's slice of K = 3^d - 1 gates divided by its own abs-sum,
then the chained propagation.  Defined as "the demo's torch-side normalisation, then the engine's NONE op", so everything here is pinned
against code that exists: float64 torch statements of abs / sum / div and of the NONE recurrence, and today's composition
(torch normalisation + affinity_propagate, or gate_absnorm + cspn3d_forward(..., 'none')).
CPU: exports, header, ABI version, argument errors.  GPU: the normaliser and its adjoint, the fused 3D forward, per-channel gates, gradients."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from oracle.backward import DX, DY, OFF3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn_gate_absnorm_f32", "cspn_gate_absnorm_backward_f32", "cspn3d_forward_absnorm_workspace_bytes", "cspn3d_forward_absnorm_f32"]
GFLOOR = 5e-6
GTOL = 2e-4   # the element-wise gradient form of tests/test_backward3d.py


# ---- float64 torch statements ----
def _torch_absnorm(g, K):
    """demo.py:24,34-36,47-49: abs, sum over each channel's K gates, div"""
    N, M = g.shape[:2]
    a = g.abs().reshape(N, M // K, K, *g.shape[2:])
    return (a / a.sum(2, keepdim=True)).reshape(g.shape)


def _torch_none3d(w, h, n_iter):
    """H_{t+1}(p) = sum_k w_k(p) H_t(p + off_k), zero outside (tests/test_backward3d.py::_torch_forward)"""
    B, _, D, H, W = w.shape
    x = h[:, 0]
    for _ in range(n_iter):
        pad = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))
        acc = 0
        for k, (dz, dy, dx) in enumerate(OFF3):
            acc = acc + w[:, k] * pad[:, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        x = acc
    return x[:, None]


def _torch_none2d(w, h, n_iter):
    """the 2D NONE op: H_{t+1}(p) = sum_k w_k(p) H_t(p + (DY_k, DX_k)), centre-sited, no centre term"""
    B, _, H, W = w.shape
    x = h[:, 0]
    for _ in range(n_iter):
        pad = torch.nn.functional.pad(x, (1, 1, 1, 1))
        acc = 0
        for k in range(8):
            acc = acc + w[:, k] * pad[:, 1 + DY[k]:1 + DY[k] + H, 1 + DX[k]:1 + DX[k] + W]
        x = acc
    return x[:, None]


def _torch_module(guide, feat, n_iter):
    """the demo's cspn() in torch: per channel its own slice, normalised, then the NONE recurrence"""
    d = feat.dim() - 2
    K = 3 ** d - 1
    w = _torch_absnorm(guide, K)
    step = _torch_none3d if d == 3 else _torch_none2d
    return torch.cat([step(w[:, c * K:(c + 1) * K], feat[:, c:c + 1], n_iter) for c in range(feat.shape[1])], 1)


def _port_today(guide, feat, n_iter):
    """what a port of demo.py writes today: torch abs / sum / div per channel, then cspn_amd.affinity_propagate"""
    K = 3 ** (feat.dim() - 2) - 1
    outs = []
    for c in range(feat.shape[1]):
        s = guide[:, c * K:(c + 1) * K].abs()
        outs.append(cspn_amd.affinity_propagate(feat[:, c:c + 1], s / s.sum(1, keepdim=True), 3, n_iter))
    return torch.cat(outs, 1)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _check_grad(a, b, what=""):
    from helpers import assert_close
    assert_close(a, b, what, rtol=GTOL, atol_frac=GFLOOR)


# ---- CPU ----
def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    norm = _lib.late_symbol("cspn_gate_absnorm_f32")
    back = _lib.late_symbol("cspn_gate_absnorm_backward_f32")
    a, b, c = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)
    assert norm(a, b, 2, 9, 64, None) == -1 and b"K must be" in lib.cspn_last_error()
    assert norm(None, b, 2, 26, 64, None) == -1 and b"null" in lib.cspn_last_error()
    assert norm(a, a, 2, 26, 64, None) == -1 and b"alias" in lib.cspn_last_error()
    assert norm(a, ctypes.c_void_p((1 << 20) + 64), 2, 8, 64, None) == -1   # overlapping ranges
    assert norm(a, b, 0, 8, 64, None) == -1 and norm(a, b, 1, 8, 0, None) == -1
    assert back(a, b, a, 1, 26, 16, None) == -1 and back(a, b, b, 1, 8, 16, None) == -1
    assert back(a, None, c, 1, 8, 16, None) == -1 and back(a, b, c, 1, 7, 16, None) == -1
    wsb = _lib.late_symbol("cspn3d_forward_absnorm_workspace_bytes")
    vol = 2 * 8 * 16 * 128 * 4
    assert wsb(2, 8, 16, 128, 4) >= 26 * vol + 2 * vol   # the normalised gates of the unfused route + two value volumes
    assert wsb(2, 8, 16, 126, 4) >= 26 * 2 * 8 * 16 * 126 * 4 + lib.cspn3d_workspace_bytes(2, 8, 16, 126, 4)
    assert wsb(0, 8, 16, 128, 4) == 0 and wsb(1, 8, 16, 128, 0) == 0
    fwd = _lib.late_symbol("cspn3d_forward_absnorm_f32")
    assert fwd(None, b, c, 1, 2, 4, 4, 3, 0, None, 0, None) == -1
    assert fwd(a, b, b, 1, 2, 4, 4, 3, 0, None, 0, None) == -1 and b"alias" in lib.cspn_last_error()
    assert fwd(a, b, c, 1, 2, 4, 4, 3, 7, None, 0, None) == -1 and b"algo" in lib.cspn_last_error()
    assert fwd(a, b, c, 1, 2, 4, 4, 3, 0, None, 0, None) == -2 and b"workspace" in lib.cspn_last_error()
    assert fwd(a, b, c, 1, 2, 4, 4, -1, 0, None, 0, None) == -1


def test_python_api_exists_and_raises_without_gpu():
    assert {"CSPN", "gate_absnorm", "absnorm_propagate"} <= set(cspn_amd.__all__)
    m = cspn_amd.CSPN(dim_num=3, feat_chan=1, prop_kernel=3, prop_step=12)   # demo.py:96-98
    assert (m.dim_num, m.feat_chan, m.prop_kernel, m.prop_step) == (3, 1, 3, 12) and list(m.parameters()) == []
    with pytest.raises(AssertionError):
        cspn_amd.CSPN(3, 1, 5, 12)
    with pytest.raises(AssertionError):
        cspn_amd.CSPN(4, 1, 3, 12)
    g3, x3 = torch.rand(1, 26, 2, 4, 8), torch.rand(1, 1, 2, 4, 8)
    with pytest.raises(cspn_amd.CspnError):
        m.cspn(g3, x3)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.gate_absnorm(g3, 26)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.absnorm_propagate(torch.rand(2, 16, 4, 8), torch.rand(2, 2, 4, 8), 3)
    with pytest.raises(ValueError):   # channel count is not C * K
        cspn_amd.absnorm_propagate(torch.rand(1, 26, 2, 4, 8), torch.rand(1, 2, 2, 4, 8), 3)
    with pytest.raises(ValueError):
        cspn_amd.CSPN(2, 1, 3, 4)(torch.rand(1, 9, 4, 8), torch.rand(1, 1, 4, 8))
    with pytest.raises(ValueError):
        cspn_amd.gate_absnorm(torch.rand(1, 25, 4, 8), 26)
    with pytest.raises(ValueError):
        cspn_amd.gate_absnorm(torch.rand(1, 26, 4, 8), 9)
    with pytest.raises(ValueError):
        cspn_amd.absnorm_propagate(torch.rand(1, 8, 4), torch.rand(1, 1, 4), 3)
    assert cspn_amd.absnorm_propagate(g3, x3, 0) is x3   # n_iter == 0: the very same tensor (Affinity_Propagate's rule)
    assert cspn_amd.CSPN(3, 1, 3, 0).cspn(g3, x3) is x3


# ---- GPU ----
def _guide(shape, seed, zero_voxel=None, zero_gates=False):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(*shape, generator=gen)
    flat = g.view(shape[0], shape[1], -1)
    if zero_voxel is not None:
        flat[0, :, zero_voxel] = 0.   # every slice of that voxel all zero: NaN, as torch's 0 / 0
    if zero_gates:
        flat[:, 1::5, 3::7] = 0.      # zeros inside slices that do not sum to zero: gradient 0 there
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("K,shape", [(26, (2, 26, 3, 5, 7)), (26, (1, 52, 4, 6, 8)), (8, (3, 8, 7, 9)), (8, (2, 16, 12, 20))])
@pytest.mark.parametrize("offset", [0, 1])
def test_normaliser_forward_backward_vs_fp64_torch(K, shape, offset):
    """odd V, V % 4 == 0, misaligned views (offset 1 float), an all-zero voxel (NaN where torch has NaN), zeros inside a slice"""
    g = _guide(shape, seed=K + offset, zero_voxel=2, zero_gates=True)
    gen = torch.Generator().manual_seed(7)
    gw = torch.randn(*shape, generator=gen)
    n = g.numel()
    buf = torch.empty(n + offset, device="cuda")
    gd = buf[offset:].view(shape)
    gd.copy_(g)
    assert (gd.data_ptr() % 16 != 0) == (offset != 0)
    bufw = torch.empty(n + offset, device="cuda")
    gwd = bufw[offset:].view(shape)
    gwd.copy_(gw)
    w = cspn_amd.gate_absnorm(gd, K).cpu()
    ref = _torch_absnorm(g.double(), K)
    assert torch.equal(torch.isnan(w), torch.isnan(ref)) and bool(torch.isnan(ref).any())
    ok = ~torch.isnan(ref)
    assert float((w.double()[ok] - ref[ok]).abs().max()) <= 1e-6
    # backward against float64 autograd through abs / sum / div
    gt = g.double().requires_grad_(True)
    _torch_absnorm(gt, K).backward(gw.double())
    dg = F.gate_absnorm_backward(gd, gwd, K).cpu()
    assert torch.equal(torch.isnan(dg), torch.isnan(gt.grad))
    ok = ~torch.isnan(gt.grad)
    _check_grad(dg.double()[ok].numpy(), gt.grad[ok].numpy(), "dL/dguide K=%d" % K)
    z = (g == 0) & ok
    assert bool(z.any()) and bool((dg[z] == 0).all())   # sign(0) = 0 wherever the voxel's sum is not 0
    # under autograd: the same kernels
    ga = gd.detach().clone().requires_grad_(True)
    wa = cspn_amd.gate_absnorm(ga, K)
    assert wa.grad_fn is not None and torch.equal(torch.nan_to_num(wa.detach().cpu(), 7.), torch.nan_to_num(w, 7.))
    wa.backward(gwd)
    assert torch.equal(torch.nan_to_num(ga.grad.cpu(), 7.), torch.nan_to_num(dg, 7.))


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,H,W,n", [(1, 8, 16, 128, 4), (2, 6, 10, 64, 12), (1, 9, 17, 72, 5), (2, 5, 9, 68, 2)])
def test_fused_3d_forward_is_bitwise_the_composed_path(B, D, H, W, n):
    g = _guide((B, 26, D, H, W), seed=D + n).cuda()
    gen = torch.Generator().manual_seed(1)
    x = torch.rand(B, 1, D, H, W, generator=gen).cuda()
    fused = F.cspn3d_forward_absnorm(g, x, n, algo="persistent")   # raises where the persistent kernel does not take the call
    auto = F.cspn3d_forward_absnorm(g, x, n)
    composed = cspn_amd.cspn3d_forward(cspn_amd.gate_absnorm(g, 26), x, None, n, "none", algo="persistent")
    cspn_amd.cspn3d_check_status()
    assert torch.equal(fused, composed) and torch.equal(auto, composed)
    stepwise = F.cspn3d_forward_absnorm(g, x, n, algo="stepwise")
    ref = _torch_module(g.cpu().double(), x.cpu().double(), n)
    for o in (fused, stepwise):
        assert _rel(o.cpu(), ref) <= 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("B,D,H,W,n", [(1, 6, 10, 66, 4),    # W % 4 != 0
                                       (1, 8, 16, 128, 1),   # n_iter 1
                                       (1, 4, 8, 64, 61),    # n_iter 61
                                       (2, 3, 5, 7, 3)])     # small and odd
def test_3d_forward_where_the_persistent_kernel_does_not_take_the_call(B, D, H, W, n):
    g = _guide((B, 26, D, H, W), seed=W + n).abs().cuda()   # (non-negative gates keep 61 steps of values in range)
    gen = torch.Generator().manual_seed(2)
    x = torch.rand(B, 1, D, H, W, generator=gen).cuda()
    with pytest.raises(cspn_amd.CspnError):
        F.cspn3d_forward_absnorm(g, x, n, algo="persistent")
    out = F.cspn3d_forward_absnorm(g, x, n)
    ref = _torch_module(g.cpu().double(), x.cpu().double(), n)
    assert _rel(out.cpu(), ref) <= 1e-6
    # misaligned guide view: the normaliser's scalar path, then the NONE op
    buf = torch.empty(g.numel() + 1, device="cuda")
    gv = buf[1:].view(g.shape)
    gv.copy_(g)
    assert torch.equal(F.cspn3d_forward_absnorm(gv, x, n), out)


@pytest.mark.gpu
@pytest.mark.parametrize("d,C", [(2, 1), (2, 3), (3, 1), (3, 3)])
def test_per_channel_gates_against_the_port_as_it_stands(d, C):
    S = (40, 264) if d == 2 else (6, 12, 64)
    K = 3 ** d - 1
    N, n = 2, 6
    gen = torch.Generator().manual_seed(10 * d + C)
    g = torch.randn(N, C * K, *S, generator=gen).cuda()
    x = torch.rand(N, C, *S, generator=gen).cuda()
    m = cspn_amd.CSPN(d, C, 3, n)
    with torch.no_grad():
        out = m.cspn(g, x)
        today = _port_today(g, x, n)
    assert out.shape == x.shape
    assert _rel(out.cpu(), today.cpu()) <= 1e-5
    assert _rel(out.cpu(), _torch_module(g.cpu().double(), x.cpu().double(), n)) <= 1e-6
    assert torch.equal(m(g, x), out)


@pytest.mark.gpu
@pytest.mark.parametrize("d,C,S,n", [(3, 1, (4, 6, 64), 4), (3, 2, (3, 5, 12), 3), (2, 1, (12, 20), 5), (2, 2, (16, 264), 8)])
@pytest.mark.parametrize("which", ["guide", "feat", "both"])
def test_gradients_through_cspn_vs_fp64_autograd(d, C, S, n, which):
    K = 3 ** d - 1
    N = 2
    gen = torch.Generator().manual_seed(3 * d + C + n)
    g = (torch.rand(N, C * K, *S, generator=gen) + 0.05) * torch.sign(torch.randn(N, C * K, *S, generator=gen))
    x = torch.rand(N, C, *S, generator=gen)
    go = torch.randn(N, C, *S, generator=gen)
    gt, xt = g.double().requires_grad_(which != "feat"), x.double().requires_grad_(which != "guide")
    _torch_module(gt, xt, n).backward(go.double())
    gc, xc = g.cuda().requires_grad_(which != "feat"), x.cuda().requires_grad_(which != "guide")
    y = cspn_amd.CSPN(d, C, 3, n).cspn(gc, xc)
    assert y.grad_fn is not None
    y.backward(go.cuda())
    if which != "feat":
        _check_grad(gc.grad.cpu().numpy(), gt.grad.numpy(), "dL/dguide")
    else:
        assert gc.grad is None
    if which != "guide":
        _check_grad(xc.grad.cpu().numpy(), xt.grad.numpy(), "dL/dfeat")
    else:
        assert xc.grad is None


@pytest.mark.gpu
def test_dtype_and_device_errors():
    g, x = torch.rand(1, 26, 2, 4, 8, device="cuda"), torch.rand(1, 1, 2, 4, 8, device="cuda")
    with pytest.raises(TypeError):
        cspn_amd.absnorm_propagate(g.double(), x, 3)
    with pytest.raises(TypeError):
        cspn_amd.gate_absnorm(g.half(), 26)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.absnorm_propagate(g, x.cpu(), 3)


@pytest.mark.gpu
def test_config5_forward_equals_the_composed_path():
    """config 5: 4 x 26 x 32 x 160 x 608, 12 steps (gates 1.295 GB)"""
    B, D, H, W, n = 4, 32, 160, 608, 12
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.rand(B, 26, D, H, W, device="cuda", generator=gen) - 0.2
    x = torch.rand(B, 1, D, H, W, device="cuda", generator=gen)
    out = cspn_amd.CSPN(3, 1, 3, n).cspn(g, x)
    cspn_amd.cspn3d_check_status()
    w = cspn_amd.gate_absnorm(g, 26)
    composed = cspn_amd.cspn3d_forward(w, x, None, n, "none")
    cspn_amd.cspn3d_check_status()
    assert torch.equal(out, composed)
    assert bool(torch.isfinite(out).all())
