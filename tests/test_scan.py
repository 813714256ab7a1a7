"""Line-scan propagation, SPN's three-way recurrence (cspn2d_*_scan_*, cspn_amd/csrc/cspn2d_scan.hip, cspn_amd.LineScan_Propagate):
a hidden line walks across the image once per direction, each pixel mixing its input with the three nearest pixels of the line visited before.
  CPU  the four symbols, the ABI version, __all__; the byte queries and the line-length limit; the argument errors of the C and Python layers; the
       statement's own anchors (zero gates, the copy, the flipped problems)
  1.   forward and the three gradients against the float64 statement of the contract (written here as the loop over lines, shifts with zero
       padding, gradients from autograd) on the tile grids of test_kxk_tilegrid plus 5 x 7, 1 x 1, 1 x 9, 9 x 1, 3 x 1030 and 1030 x 3, each
       single direction and all four, (C, Cg) = (1,1), (2,1), (2,2), (4,2), with and without lam; grad_gates exactly 0 on every dropped gate
  2.   the anchors on the GPU, bit for bit
  3.   <F x, y> == <x, F^T y>; two calls give the same bits; each gradient output may be left out without changing the others' bits
  4.   LineScan_Propagate gives the functional calls' bits, 'clip' and every merge against torch's own, one engine call per pass
  5.   peak memory of a training step keeps no per-step slice
  6.   every call between guard bands on poisoned workspaces and in a stale arena (tests/memguard.py, this file's own table)
  7.   a captured graph of forward + backward replays the eager bits
Bounds (the project's): forward max|d| <= 1e-5 max|ref|; gradients helpers.assert_close(rtol=2e-4, atol_frac=5e-6); the adjoint identity 2e-4 of
sum |F x y|.  Each comparison prints its error as a fraction of its bound."""
import contextlib
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
import memguard
import test_memory_hygiene as hygiene
from cspn_amd import _lib
from cspn_amd import functional as F
from helpers import assert_close
from test_kxk_tilegrid import SHAPES as TILEGRID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_scan_workspace_bytes", "cspn2d_forward_scan_f32", "cspn2d_backward_scan_workspace_bytes", "cspn2d_backward_scan_f32"]
RTOL = 1e-5
GTOL, GFLOOR = 2e-4, 5e-6
ATOL_ADJ = 2e-4
B = 2
ALL_DIRS = (0, 1, 2, 3)
SHAPES = dict(TILEGRID, small=(5, 7), pixel=(1, 1), row=(1, 9), column=(9, 1), flat=(3, 1030), thin=(1030, 3))
DIRSETS = [(0,), (1,), (2,), (3,), ALL_DIRS]
CHANNELS = [(1, 1), (2, 1), (2, 2), (4, 2)]
MAX_LINE = 2048
# __all__ as it was before this contract (the list is closed)
ALL = 36


# ---- the float64 statement ----
def _canon(t, code):
    """[..., H, W] -> [..., L, T]: the line along the second last dimension, the scan ascending along the last"""
    if code >= 2:
        t = t.transpose(-1, -2)
    return t.flip(-1) if code in (1, 3) else t


def _uncanon(t, code):
    if code in (1, 3):
        t = t.flip(-1)
    return t.transpose(-1, -2) if code >= 2 else t


def _neighbour(h, k):
    """h [..., L] -> h(i + k - 1), zero outside the line"""
    y = torch.zeros_like(h)
    if k == 0:
        y[..., 1:] = h[..., :-1]
    elif k == 2:
        y[..., :-1] = h[..., 1:]
    else:
        y = h
    return y


def statement(x, gates, dirs=ALL_DIRS, lam=None):
    """the contract, in the dtype of its arguments -> out [B, D C, H, W]"""
    Bn, C, H, W = x.shape
    dirs = sorted(dirs)
    D = len(dirs)
    Cg = gates.shape[1] // (3 * D)
    outs = []
    for d, code in enumerate(dirs):
        g = _canon(gates[:, d * Cg * 3:(d + 1) * Cg * 3].reshape(Bn, Cg, 3, H, W).repeat_interleave(C // Cg, 1), code)   # [B, C, 3, L, T]
        xs = _canon(x, code)
        lm = None if lam is None else _canon(lam[:, d * C:(d + 1) * C], code)
        L, T = xs.shape[-2:]
        keep = torch.ones(3, L, dtype=x.dtype)   # a connection that leaves the line is dropped
        keep[0, 0] = 0
        keep[2, L - 1] = 0
        h, lines = None, []
        for t in range(T):
            gk = [torch.zeros_like(xs[..., t]) if t == 0 else g[:, :, k, :, t] * keep[k] for k in range(3)]
            b = lm[..., t] if lm is not None else 1 - (gk[0] + gk[1] + gk[2])
            hn = b * xs[..., t]
            if t:
                hn = hn + sum(gk[k] * _neighbour(h, k) for k in range(3))
            lines.append(hn)
            h = hn
        outs.append(_uncanon(torch.stack(lines, -1), code))
    return torch.cat(outs, 1)


def clip(gates):
    """SPN's stabiliser: g_k / max(1, sum_k |g_k|) per direction, group and pixel"""
    Bn, ch, H, W = gates.shape
    g = gates.reshape(Bn, ch // 3, 3, H, W)
    return (g / g.abs().sum(2, keepdim=True).clamp(min=1)).reshape(gates.shape)


def _dropped(code, Cg, H, W):
    """bool [Cg 3, H, W]: the gates of one direction the contract drops (the first line, the connections that leave the line)"""
    L, T = (H, W) if code < 2 else (W, H)
    m = torch.zeros(Cg, 3, L, T, dtype=torch.bool)
    m[..., 0] = True
    m[:, 0, 0, :] = True
    m[:, 2, L - 1, :] = True
    return _uncanon(m, code).reshape(Cg * 3, H, W)


@functools.lru_cache(maxsize=None)
def _inputs(name, C, Cg, lam, seed=0):
    """the problem of all four directions: x in [0, 10), gates randn through the clip rule, lam in [0.1, 1.1), grad_out randn"""
    H, W = SHAPES[name] if isinstance(name, str) else name
    gen = torch.Generator().manual_seed(100003 * H + 101 * W + 10 * C + Cg + 7 * seed + (3 if lam else 0))
    x = torch.rand(B, C, H, W, generator=gen) * 10
    g = clip(torch.randn(B, 4 * Cg * 3, H, W, generator=gen))
    lm = torch.rand(B, 4 * C, H, W, generator=gen) + 0.1 if lam else None
    go = torch.randn(B, 4 * C, H, W, generator=gen)
    return x, g, lm, go


def _select(inp, dirs, C, Cg):
    """the problem of the directions dirs out of the four-direction one"""
    x, g, lm, go = inp
    gs = torch.cat([g[:, d * Cg * 3:(d + 1) * Cg * 3] for d in dirs], 1).contiguous()
    ls = None if lm is None else torch.cat([lm[:, d * C:(d + 1) * C] for d in dirs], 1).contiguous()
    return x, gs, ls, torch.cat([go[:, d * C:(d + 1) * C] for d in dirs], 1).contiguous()


@functools.lru_cache(maxsize=None)
def _reference1(name, C, Cg, lam, code):
    """(out, dL/dx, dL/dgates, dL/dlam) of the float64 statement for one direction, computed once"""
    x, g, lm, go = (None if t is None else t.double() for t in _select(_inputs(name, C, Cg, lam), (code,), C, Cg))
    leaves = [t.requires_grad_(True) for t in (x, g, lm) if t is not None]
    out = statement(x, g, (code,), lm)
    out.backward(go)
    # (a scan of one line uses no gate: autograd leaves the gates' gradient unset, the contract says 0)
    return out.detach(), x.grad, (torch.zeros_like(g) if g.grad is None else g.grad), (None if lm is None else lm.grad), leaves


def _reference(name, C, Cg, lam, dirs):
    """the same for a set of directions: the channels side by side, dL/dx summed"""
    parts = [_reference1(name, C, Cg, lam, code) for code in dirs]
    return (torch.cat([p[0] for p in parts], 1), sum(p[1] for p in parts), torch.cat([p[2] for p in parts], 1),
            None if not lam else torch.cat([p[3] for p in parts], 1))


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _fwd(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e = float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))
    print("scan fwd  %-52s %.3g of %g" % (what, e / RTOL, RTOL))
    assert np.isfinite(a).all() and e <= RTOL, "%s: relative error %.3g > %g" % (what, e, RTOL)


def _grad(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    bound = GFLOOR * max(np.abs(ref).max(), 1e-30) + GTOL * np.abs(ref)
    print("scan grad %-52s %.3g of the bound" % (what, float((np.abs(a - ref) / bound).max())))
    assert_close(a, ref, what, rtol=GTOL, atol_frac=GFLOOR)


# ---- CPU ----
def test_symbols_are_declared_and_exported_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert s in _lib._SYMBOLS and _lib.symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+CSPN_ABI_VERSION\s+(\d+)", text).group(1)) == 5
    assert len(cspn_amd.__all__) == ALL and not any("scan" in n.lower() for n in cspn_amd.__all__)
    assert cspn_amd.LineScan_Propagate is __import__("cspn_amd.spn", fromlist=["x"]).LineScan_Propagate
    assert callable(F.cspn2d_forward_scan) and callable(F.cspn2d_backward_scan)


def test_byte_queries_and_the_line_length_limit():
    fwd, bwd = _lib.symbol("cspn2d_scan_workspace_bytes"), _lib.symbol("cspn2d_backward_scan_workspace_bytes")
    Bq, H, W = 2, 10, 13
    for C, Cg in ((1, 1), (6, 1), (6, 2), (6, 6)):
        for dirs in range(1, 16):
            D = bin(dirs).count("1")
            for lam in (0, 1):
                f, b = fwd(Bq, C, Cg, H, W, dirs, lam), bwd(Bq, C, Cg, H, W, dirs, lam)
                parts = 4 * Bq * H * W * ((D - 1) * C + (C // Cg - 1) * D * Cg * 3)
                assert 256 <= f < (1 << 20) and f % 256 == 0
                assert b % 256 == 0 and 256 + parts <= b <= 256 + parts + 2 * 256
    assert 256 <= fwd(8, 32, 32, 304, 1216, 15, 1) < (1 << 20) and 256 <= fwd(8, 32, 1, 304, 1216, 15, 0) < (1 << 20)
    for q in (fwd, bwd):
        for C, Cg in ((6, 4), (6, 0), (6, -1), (2, 4)):
            assert q(Bq, C, Cg, H, W, 15, 0) == 0
        for dirs in (0, 16, -1, 31):
            assert q(Bq, 2, 1, H, W, dirs, 0) == 0
        for shape in ((0, 2, 1, 10, 13), (2, 0, 1, 10, 13), (2, 2, 1, 0, 13), (2, 2, 1, 10, 0), (-1, 2, 1, 10, 13)):
            assert q(*shape, 15, 0) == 0
        # the longest line: H for directions 0 / 1, W for 2 / 3; the scan itself may be longer
        assert q(1, 1, 1, MAX_LINE, 5, 1, 0) >= 256 and q(1, 1, 1, MAX_LINE + 1, 5, 1, 0) == 0 and q(1, 1, 1, MAX_LINE + 1, 5, 2, 0) == 0
        assert q(1, 1, 1, 5, MAX_LINE, 4, 0) >= 256 and q(1, 1, 1, 5, MAX_LINE + 1, 4, 0) == 0 and q(1, 1, 1, 5, MAX_LINE + 1, 8, 0) == 0
        assert q(1, 1, 1, MAX_LINE + 1, 5, 12, 0) >= 256 and q(1, 1, 1, 5, MAX_LINE + 1, 3, 0) >= 256
        assert q(1, 1, 1, MAX_LINE, MAX_LINE, 15, 1) >= 256 and q(1, 1, 1, MAX_LINE + 1, MAX_LINE, 15, 1) == 0
        assert q(1, 1, 1, 5, MAX_LINE + 1, 5, 0) == 0   # one direction of the mask refuses
        # a tensor of more than 2^31 - 1 elements: out (B D C H W), the gates (B D Cg 3 H W)
        assert q(1 << 10, 1 << 9, 1, 1 << 6, 1 << 6, 1, 0) == 0 and q(1 << 10, 1 << 8, 1 << 8, 1 << 6, 1 << 6, 1, 0) == 0
        assert q(1 << 10, 1 << 7, 1, 1 << 6, 1 << 6, 15, 0) == 0 and q(1 << 10, 1 << 7, 1, 1 << 6, 1 << 6, 1, 0) >= 256


def test_argument_errors_of_the_c_layer():
    """no call below reaches a launch: every one fails a check (or, needing nothing, returns 0) before the stream is touched"""
    x, g, lm, o, go, gx, gg, gl, w = (ctypes.c_void_p(i << 32) for i in range(1, 10))
    big = 1 << 22
    # (x, gates, lam, out, B, C, Cg, H, W, dirs, ws, ws_bytes, stream)
    fwd = [((None, g, lm, o, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, None, lm, o, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, None, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 3, 2, 8, 8, 15, w, big, None), -1),       # Cg does not divide C
           ((x, g, lm, o, 2, 2, 0, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 2, 1, 8, 8, 0, w, big, None), -1),        # dirs outside 1 .. 15
           ((x, g, lm, o, 2, 2, 1, 8, 8, 16, w, big, None), -1),
           ((x, g, lm, o, 2, 2, 1, 8, 8, -1, w, big, None), -1),
           ((x, g, lm, o, 0, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 0, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 2, 1, 0, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 2, 1, 8, -3, 15, w, big, None), -1),
           ((x, g, lm, x, 2, 2, 1, 8, 8, 15, w, big, None), -1),       # out aliases x, the gates, lam, the workspace
           ((x, g, lm, g, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, lm, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, w, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, 2, 2, 1, 8, 8, 15, g, big, None), -1),       # the workspace aliases the gates
           ((x, g, lm, o, 2, 2, 1, 8, 8, 15, None, 0, None), -2),
           ((x, g, lm, o, 2, 2, 1, 8, 8, 15, w, 100, None), -2),
           ((x, g, lm, o, 2, 2, 1, 8, 8, 15, ctypes.c_void_p((9 << 32) + 4), big, None), -2),
           ((x, g, lm, o, 1, 1, 1, MAX_LINE + 1, 8, 1, w, big, None), -3),
           ((x, g, lm, o, 1, 1, 1, 8, MAX_LINE + 1, 8, w, big, None), -3),
           ((x, g, lm, o, 1 << 10, 1 << 9, 1, 1 << 6, 1 << 6, 1, w, big, None), -3)]
    # (x, gates, lam, out, grad_out, grad_x, grad_gates, grad_lam, B, C, Cg, H, W, dirs, ws, ws_bytes, stream)
    bwd = [((None, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, None, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, None, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, None, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, None, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),     # grad_lam without lam
           ((x, g, lm, o, go, gx, gg, gl, 2, 3, 2, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 0, w, big, None), -1),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 0, 15, w, big, None), -1),
           ((x, g, lm, o, go, gx, gx, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),       # two gradients in one place
           ((x, g, lm, o, go, gx, gg, gg, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, gl, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, go, gg, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),       # a gradient on an input
           ((x, g, lm, o, go, gx, o, gl, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, gx, gg, x, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, gx, gg, lm, 2, 2, 1, 8, 8, 15, w, big, None), -1),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, gg, big, None), -1),      # the workspace on grad_gates, on out
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, o, big, None), -1),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, None, 0, None), -2),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, w, 64, None), -2),
           ((x, g, lm, o, go, gx, gg, gl, 2, 2, 1, 8, 8, 15, ctypes.c_void_p((9 << 32) + 128), big, None), -2),
           ((x, g, lm, o, go, gx, gg, gl, 1, 1, 1, MAX_LINE + 1, 8, 2, w, big, None), -3),
           ((x, g, lm, o, go, gx, gg, gl, 1 << 10, 1 << 8, 1 << 8, 1 << 6, 1 << 6, 1, w, big, None), -3),
           ((x, g, lm, o, go, None, None, None, 2, 2, 1, 8, 8, 15, w, big, None), 0)]   # nothing asked for: nothing done
    for name, cases in (("cspn2d_forward_scan_f32", fwd), ("cspn2d_backward_scan_f32", bwd)):
        f = _lib.symbol(name)
        for args, code in cases:
            assert f(*args) == code, (name, args)
            if code:
                assert name.encode() in cspn_amd.load().cspn_last_error()


def test_python_argument_errors_without_gpu():
    x, g, lm = torch.zeros(1, 4, 4, 5), torch.zeros(1, 4 * 2 * 3, 4, 5), torch.zeros(1, 16, 4, 5)
    for dirs in ((), (0, 0), (4,), (-1,), (0, 1.0), 3, (True,)):
        with pytest.raises(ValueError):
            F.cspn2d_forward_scan(x, g, dirs)
        with pytest.raises(ValueError):
            cspn_amd.LineScan_Propagate(dirs)
    with pytest.raises(ValueError):
        F.cspn2d_forward_scan(x, g[:, :23])                  # 23 channels are not D Cg 3
    with pytest.raises(ValueError):
        F.cspn2d_forward_scan(x, g, (0, 1, 2))               # 24 channels are not 3 directions x Cg x 3
    with pytest.raises(ValueError):
        F.cspn2d_forward_scan(x, torch.zeros(1, 36, 4, 5))   # 3 groups do not divide 4 channels
    with pytest.raises(ValueError):
        F.cspn2d_forward_scan(x, g, lam=lm[:, :4])
    with pytest.raises(ValueError):
        F.cspn2d_forward_scan(x, g[..., :4])
    with pytest.raises(ValueError):
        F.cspn2d_backward_scan(x, g, lm, lm[:, :4])
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        for i in range(3):
            args = [x, g, lm]
            args[i] = args[i].to(bad)
            with pytest.raises(TypeError):
                F.cspn2d_forward_scan(args[0], args[1], ALL_DIRS, args[2])
            with pytest.raises(TypeError):
                cspn_amd.LineScan_Propagate()(*args)
        with pytest.raises(TypeError):
            F.cspn2d_backward_scan(x, g, lm, lm.to(bad))
    with pytest.raises(_lib.CspnError):
        F.cspn2d_forward_scan(x, g)                          # no CPU path
    for kw in ({"norm": "softmax"}, {"merge": "min"}, {"groups": 0}, {"groups": 1.5}):
        with pytest.raises(ValueError):
            cspn_amd.LineScan_Propagate(**kw)
    with pytest.raises(ValueError):
        cspn_amd.LineScan_Propagate(groups=4)(x, g)          # the gates hold 2 groups
    m = cspn_amd.LineScan_Propagate((3, 0))
    assert (m.dirs, m.groups, m.norm, m.merge) == ((0, 3), None, None, "max") and not list(m.parameters())


def test_the_statement_has_the_contracts_anchors():
    """float64, CPU: all-zero gates return x (or lam x); g_1 = 1 alone copies the first line along the scan; direction 1 is direction 0 on the
    horizontally flipped problem, 3 is 2 on the vertically flipped one"""
    C, Cg = 2, 1
    for name in ("small", "row", "column", "pixel"):
        H, W = SHAPES[name]
        x, g, lm, _ = (None if t is None else t.double() for t in _inputs(name, C, Cg, True))
        zero = torch.zeros_like(g)
        assert torch.equal(statement(x, zero), x.repeat(1, 4, 1, 1)) and torch.equal(statement(x, zero, ALL_DIRS, lm), lm * x.repeat(1, 4, 1, 1))
        copy = zero.clone()
        copy[:, 1::3] = 1
        out = statement(x, copy).view(B, 4, C, H, W)
        first = (x[..., :, :1], x[..., :, -1:], x[..., :1, :], x[..., -1:, :])
        for d in range(4):
            assert torch.equal(out[:, d], first[d].expand(B, C, H, W))
        for a, b_, dim in ((1, 0, -1), (3, 2, -2)):
            _, ga, la, _ = _select((x, g, lm, lm), (a,), C, Cg)
            mine = statement(x, ga, (a,), la)
            assert torch.equal(mine, statement(x.flip(dim), ga.flip(dim), (b_,), la.flip(dim)).flip(dim))
            assert name != "small" or not torch.equal(mine, statement(x, ga, (b_,), la))


# ---- 1. against the float64 statement ----
@pytest.mark.gpu
@pytest.mark.parametrize("lam", [False, True])
@pytest.mark.parametrize("C,Cg", CHANNELS)
@pytest.mark.parametrize("dirs", DIRSETS, ids=lambda d: "d" + "".join(map(str, d)))
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_and_gradients_vs_fp64_statement(name, dirs, C, Cg, lam):
    H, W = SHAPES[name]
    r_out, r_gx, r_gg, r_gl = _reference(name, C, Cg, lam, dirs)
    x, g, lm, go = _cuda(*_select(_inputs(name, C, Cg, lam), dirs, C, Cg))
    what = "%s dirs=%s C=%d Cg=%d%s" % (name, "".join(map(str, dirs)), C, Cg, " lam" if lam else "")
    out = F.cspn2d_forward_scan(x, g, dirs, lm)
    _fwd(out.cpu().numpy(), r_out.numpy(), what + " out")
    gx, gg, gl = F.cspn2d_backward_scan(x, g, out, go, dirs, lm)
    _grad(gx.cpu().numpy(), r_gx.numpy(), what + " dL/dx")
    _grad(gg.cpu().numpy(), r_gg.numpy(), what + " dL/dgates")
    if lam:
        _grad(gl.cpu().numpy(), r_gl.numpy(), what + " dL/dlam")
    else:
        assert gl is None
    dropped = torch.cat([_dropped(code, Cg, H, W) for code in dirs], 0)
    assert bool((gg.cpu()[:, dropped] == 0).all()), what + ": a dropped gate has a gradient"
    assert bool((r_gg[:, dropped] == 0).all())


# ---- 2. anchors ----
@pytest.mark.gpu
@pytest.mark.parametrize("lam", [False, True])
@pytest.mark.parametrize("name", ["wide", "tall", "flat", "thin", "column"])
def test_anchors_bit_for_bit(name, lam):
    C, Cg = 2, 1
    H, W = SHAPES[name]
    x, g, lm, _ = _cuda(*_inputs(name, C, Cg, lam))
    zero = torch.zeros_like(g)
    want = x.repeat(1, 4, 1, 1) if lm is None else lm * x.repeat(1, 4, 1, 1)
    assert torch.equal(F.cspn2d_forward_scan(x, zero, ALL_DIRS, lm), want)
    copy = zero.clone()
    copy[:, 1::3] = 1
    out = F.cspn2d_forward_scan(x, copy).view(B, 4, C, H, W)
    first = (x[..., :, :1], x[..., :, -1:], x[..., :1, :], x[..., -1:, :])
    for d in range(4):
        assert torch.equal(out[:, d], first[d].expand(B, C, H, W)), "direction %d does not copy its first line" % d
    for a, b_, dim in ((1, 0, -1), (3, 2, -2)):
        _, ga, la, _ = _select((x, g, lm, x), (a,), C, Cg)
        flipped = F.cspn2d_forward_scan(x.flip(dim).contiguous(), ga.flip(dim).contiguous(), (b_,), None if la is None else la.flip(dim).contiguous())
        assert torch.equal(F.cspn2d_forward_scan(x, ga, (a,), la), flipped.flip(dim)), "direction %d is not direction %d flipped" % (a, b_)


# ---- 3. adjointness, determinism, optional outputs ----
@pytest.mark.gpu
@pytest.mark.parametrize("lam", [False, True])
@pytest.mark.parametrize("dirs", DIRSETS, ids=lambda d: "d" + "".join(map(str, d)))
@pytest.mark.parametrize("name", ["tall", "flat", "thin"])
def test_scan_and_adjoint_scan_are_adjoint(name, dirs, lam):
    C, Cg = 2, 1
    x, g, lm, y = _cuda(*_select(_inputs(name, C, Cg, lam), dirs, C, Cg))
    fx = F.cspn2d_forward_scan(x, g, dirs, lm)
    bty, none, none2 = F.cspn2d_backward_scan(x, g, fx, y, dirs, lm, need_gates=False, need_lam=False)
    assert none is None and none2 is None
    lhs, rhs = float((fx.double() * y.double()).sum()), float((x.double() * bty.double()).sum())
    scale = float((fx.double() * y.double()).abs().sum())
    print("scan adj  %-52s %.3g of the bound" % ("%s dirs=%s%s" % (name, "".join(map(str, dirs)), " lam" if lam else ""), abs(lhs - rhs) / (ATOL_ADJ * scale)))
    assert np.isfinite(lhs) and np.isfinite(rhs) and scale > 0
    assert abs(lhs - rhs) <= ATOL_ADJ * scale, "<F x, y> = %.9g, <x, F^T y> = %.9g, sum |F x y| = %.6g" % (lhs, rhs, scale)


def _all_outputs(dirs, x, g, lm, go):
    out = F.cspn2d_forward_scan(x, g, dirs, lm)
    return (out,) + tuple(F.cspn2d_backward_scan(x, g, out, go, dirs, lm))


@pytest.mark.gpu
@pytest.mark.parametrize("lam", [False, True])
@pytest.mark.parametrize("C,Cg", [(2, 2), (4, 2)])
@pytest.mark.parametrize("name", ["wide", "thin"])
def test_two_calls_give_the_same_bits_and_each_gradient_may_be_left_out(name, C, Cg, lam):
    x, g, lm, go = _cuda(*_inputs(name, C, Cg, lam))
    ref = _all_outputs(ALL_DIRS, x, g, lm, go)
    memguard.assert_same_outputs(_all_outputs(ALL_DIRS, x, g, lm, go), ref, "second call")
    out = ref[0]
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True)):
        got = F.cspn2d_backward_scan(x, g, out, go, ALL_DIRS, lm, *need)
        for i, n in enumerate(need):
            if n and ref[1 + i] is not None:
                assert torch.equal(got[i], ref[1 + i]), "output %d changed when the others were left out (%s)" % (i, need)
            else:
                assert got[i] is None


# ---- 4. the module ----
@pytest.mark.gpu
@pytest.mark.parametrize("lam", [False, True])
@pytest.mark.parametrize("merge", ["max", "sum", "mean", None])
@pytest.mark.parametrize("norm", [None, "clip"])
def test_module_gives_the_functional_calls_bits(norm, merge, lam):
    C, Cg, dirs = 4, 2, (0, 2, 3)
    H, W = SHAPES["tall"]
    D = len(dirs)
    x, g, lm, go = _cuda(*_select(_inputs("tall", C, Cg, lam), dirs, C, Cg))
    raw = g * 3 if norm else g   # what a head would emit: sum |g| > 1 at many pixels
    merged = {"max": lambda o: o.view(B, D, C, H, W).max(1).values, "sum": lambda o: o.view(B, D, C, H, W).sum(1),
              "mean": lambda o: o.view(B, D, C, H, W).mean(1), None: lambda o: o}[merge]
    # the composition by hand: torch's clip, the two engine calls, torch's merge
    gl_ = raw.clone().requires_grad_(True)
    gn = clip(gl_) if norm else gl_
    out = F.cspn2d_forward_scan(x, gn.detach().contiguous(), dirs, lm)
    ol = out.clone().requires_grad_(True)
    y_ref = merged(ol)
    gy = go[:, :y_ref.shape[1]].contiguous()
    y_ref.backward(gy)
    gx, gg, glam = F.cspn2d_backward_scan(x, gn.detach().contiguous(), out, ol.grad.contiguous(), dirs, lm)
    gn.backward(gg)
    m = cspn_amd.LineScan_Propagate(dirs, Cg, norm, merge)
    with torch.no_grad():
        assert torch.equal(m(x, raw, lm), y_ref.detach())
    leaves = [t.clone().requires_grad_(True) for t in (x, raw)] + ([lm.clone().requires_grad_(True)] if lam else [])
    y = m(*leaves)
    assert torch.equal(y.detach(), y_ref.detach())
    y.backward(gy)
    assert torch.equal(leaves[0].grad, gx) and torch.equal(leaves[1].grad, gl_.grad)
    if lam:
        assert torch.equal(leaves[2].grad, glam)
    # one gradient alone; groups read off the gates
    gr = raw.clone().requires_grad_(True)
    cspn_amd.LineScan_Propagate(dirs, None, norm, merge)(x, gr, lm).backward(gy)
    assert torch.equal(gr.grad, gl_.grad)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            m(x.to(dt), raw, lm)
        with pytest.raises(TypeError):
            m(x, raw.to(dt), lm)


@pytest.mark.gpu
def test_one_engine_call_per_pass_whatever_the_size(monkeypatch):
    calls = []
    real = F._launch

    def counting(name, *a, **kw):
        calls.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(F, "_launch", counting)
    m = cspn_amd.LineScan_Propagate(norm="clip", merge="max")
    for name in ("small", "wide", "thin"):
        x, g, lm, go = _cuda(*_inputs(name, 2, 2, True))
        leaves = [t.clone().requires_grad_(True) for t in (x, g, lm)]
        del calls[:]
        y = m(*leaves)
        assert calls == ["cspn2d_forward_scan_f32"], (name, calls)
        y.backward(go[:, :2].contiguous())
        assert calls == ["cspn2d_forward_scan_f32", "cspn2d_backward_scan_f32"], (name, calls)
        assert all(t.grad is not None for t in leaves)


# ---- 5. memory ----
@pytest.mark.gpu
def test_a_training_step_keeps_no_per_step_slice():
    """peak memory over one training step at 64 x 256, C = Cg = 8, four directions, with lam, stays below the bytes of the output and the three
    gradients plus one more [B, D C, H, W] tensor (the inputs and grad_out are allocated before): the backward's workspace is three quarters of
    such a tensor (grad_x of the directions 1 .. 3), and a loop over the 256 columns under autograd would keep 256 slices of each direction"""
    from cspn_amd.spn import linescan_propagate
    C = Cg = 8
    shape = (64, 256)
    x, g, lm, go = _cuda(*_inputs(shape, C, Cg, True))
    leaves = [t.clone().requires_grad_(True) for t in (x, g, lm)]
    linescan_propagate(*leaves[:2], ALL_DIRS, leaves[2]).backward(go)   # warm: symbols bound
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()

    def nbytes(*ts):
        return sum(t.numel() * t.element_size() for t in ts)

    # the bytes asked of the allocator, not the blocks it handed out: a cached block up to 1 MiB larger than the request is handed out whole and
    # counted whole by memory_allocated, which in a warm process is as much as the margin of this budget
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_stats()["requested_bytes.all.current"]   # the inputs and grad_out
    out = linescan_propagate(*leaves[:2], ALL_DIRS, leaves[2])
    out.backward(go)
    torch.cuda.synchronize()
    extra = torch.cuda.memory_stats()["requested_bytes.all.peak"] - before
    budget = nbytes(out) + nbytes(*leaves) + nbytes(out)
    print("scan mem  training step: %d bytes beyond the inputs, %.3g of the budget %d" % (extra, extra / budget, budget))
    assert all(t.grad is not None for t in leaves) and extra < budget


# ---- 6. memory hygiene: every call between guard bands on NaN and on finite poison, and in a stale arena ----
def _hygiene_inputs(name, C, Cg, lam):
    return _cuda(*_inputs(name, C, Cg, lam, seed=5))


def _hygiene_call(C, Cg):
    def call(x, g, lm, go):
        out = F.cspn2d_forward_scan(x, g, ALL_DIRS, lm)
        grads = F.cspn2d_backward_scan(x, g, out, go, ALL_DIRS, lm)
        alone = F.cspn2d_backward_scan(x, g, out, go, ALL_DIRS, lm, False, True, False)[1]
        _, g1, l1, go1 = _select((x, g, lm, go), (1,), C, Cg)
        one = F.cspn2d_forward_scan(x, g1, (1,), l1)
        gone = F.cspn2d_backward_scan(x, g1, one, go1, (1,), l1)
        leaves = [hygiene._leaf(t) for t in (x, g)] + ([hygiene._leaf(lm)] if lm is not None else [])
        y = cspn_amd.LineScan_Propagate(ALL_DIRS, Cg, "clip", "max")(*leaves)
        y.backward(go[:, :C].contiguous())
        return (out,) + tuple(grads) + (alone, one) + tuple(gone) + (y.detach(),) + tuple(t.grad for t in leaves)
    return call


HYGIENE = {}
for _name, _C, _Cg, _lam in (("tall", 2, 1, True), ("wide", 4, 2, False), ("strip", 2, 2, True), ("thin", 2, 1, True), ("flat", 4, 2, False)):
    _H, _W = SHAPES[_name]
    _n = "scan-%dx%d-C%d-Cg%d" % (_H, _W, _C, _Cg)
    HYGIENE[_n] = hygiene.Case(_n, tuple(NEW), "the scan entry points and LineScan_Propagate", 4 * B * 4 * _C * _H * _W,
                               functools.lru_cache(maxsize=None)(functools.partial(_hygiene_inputs, _name, _C, _Cg, _lam)), _hygiene_call(_C, _Cg),
                               lambda: None, "test_scan.py::test_forward_and_gradients_vs_fp64_statement", False, None, None)


def test_the_guarded_cases_stay_out_of_the_shared_table():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True}
    assert not any("scan" in n for c in hygiene.CASES.values() for n in c.covers)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_call_between_guard_bands(name, poison):
    """every output (out, the three gradients) and every workspace lies between guard bands and is poisoned before the call: clean outputs (bitwise
    the unguarded run's, so fully written), intact bands, unchanged inputs"""
    c = HYGIENE[name]
    inputs = c.build()
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, inputs, "cuda", c.plane)
    assert len(session.workspaces) >= 7 and len(session.guards) > len(session.workspaces)
    for o in outs:
        assert o is None or bool(torch.isfinite(o.float()).all()), "poison reached an output"
    memguard.assert_same_outputs(outs, hygiene._clean(c), "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    """the calls of every case through one workspace arena that is never refilled: every result bitwise the clean one"""
    steps = []
    names = list(HYGIENE)
    for name in names + names[:2]:
        c = HYGIENE[name]
        steps.append((name, c.call, c.build()))
    hygiene._run_sequence(steps, max(c.plane for c in HYGIENE.values()))


# ---- 7. a captured graph ----
@pytest.mark.gpu
def test_a_captured_graph_replays_the_eager_bits():
    C, Cg = 4, 2
    shape = (40, 136)
    x, g, lm, go = _cuda(*_inputs(shape, C, Cg, True))
    g2 = _inputs(shape, C, Cg, True, seed=1)[1].cuda()
    ref = _all_outputs(ALL_DIRS, x, g, lm, go)
    ref2 = _all_outputs(ALL_DIRS, x, g2, lm, go)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream, one chain: forward, then backward on its result
        cap = _all_outputs(ALL_DIRS, x, g, lm, go)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        memguard.assert_same_outputs(cap, ref, "replay")
    g.copy_(g2)   # new contents behind the captured pointers
    graph.replay()
    torch.cuda.synchronize()
    memguard.assert_same_outputs(cap, ref2, "replay on new contents")
