"""K x K propagation with per-step attention (cspn2d_*_kxk_dyn_*, cspn_amd/csrc/cspn2d_kxk_dyn.hip, cspn_amd.Dynamic_Propagate):
the affinities are the raw guidance times a per-step, per-ring attention, re-normalised on every step; no modulated or normalised gate is stored.
  CPU  the four symbols, the ABI version, __all__; the byte queries; the argument errors of the absnorm twins; the Python argument errors
  1.   forward, every kept level and the three gradients against the float64 statement of the contract (written here with shifted adds and zero
       padding, gradients from autograd) on the tile grids of test_kxk_tilegrid plus 5 x 7 and 1 x 1, K = 3 / 5 / 7, C = 1 / 2, n = 3, with and
       without sparse, attention all positive and with a quarter of the ring planes negated
  2.   anchors: the identity attention, and the ring attention that makes the step cspn2d_forward_kxk_absnorm's
  3.   <F x, y> == <x, F^T y>; two calls give the same bits
  4.   Dynamic_Propagate gives the functional calls' bits, the three activations against torch's own
  5.   peak memory of a training step leaves no room for n x KK modulated planes
  6.   every call between guard bands on poisoned workspaces and in a stale arena (tests/memguard.py, this file's own table)
  7.   a captured graph of forward + backward replays the eager bits
Bounds (the project's): forward and every kept level max|d| <= 1e-5 max|ref|; gradients helpers.assert_close(rtol=2e-4, atol_frac=5e-6); the adjoint
identity 2e-4 of sum |F x y|.  Each comparison prints its error as a fraction of its bound."""
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
NEW = ["cspn2d_forward_kxk_dyn_f32", "cspn2d_backward_kxk_dyn_f32", "cspn2d_kxk_dyn_workspace_bytes", "cspn2d_backward_kxk_dyn_workspace_bytes"]
RTOL = 1e-5
GTOL, GFLOOR = 2e-4, 5e-6
ATOL_ADJ = 2e-4
B = 2
N_ITER = 3
SHAPES = dict(TILEGRID, small=(5, 7), pixel=(1, 1))
# __all__ as it was before this contract (the list is closed)
ALL = 36


# ---- the float64 statement ----
def _offsets(K):
    R = K // 2
    return [(R - t, R - l) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def _shift(x, dy, dx):
    """y(p) = x(p + (dy, dx)), zero where that lies outside the image"""
    H, W = x.shape[-2:]
    y = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        y[..., y0:y1, x0:x1] = x[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return y


def statement(g, att, x, sparse, K, n):
    """the contract, in the dtype of its arguments -> (H_n, [Ht_1 .. Ht_{n-1}])"""
    R, offs = K // 2, _offsets(K)
    rings = [max(abs(dy), abs(dx)) for dy, dx in offs]
    m = None if sparse is None else (sparse > 0).to(x.dtype)
    H, kept = x, []
    for t in range(n):
        Ht = H if m is None else (1 - m) * H + m * sparse
        if t:
            kept.append(Ht)
        a = att[:, t * (R + 1):(t + 1) * (R + 1)]
        wh = [a[:, r:r + 1] * g[:, k:k + 1] for k, r in enumerate(rings)]
        D = a[:, 0:1] + sum(w.abs() for w in wh)
        w = [v / D for v in wh]
        c = 1 - sum(w)
        H = c * Ht + sum(wk * _shift(Ht, dy, dx) for wk, (dy, dx) in zip(w, offs))
    return H, kept


def _inputs(H, W, K, C, sparse, negated, n=N_ITER, seed=0):
    """guidance (rand + 0.05) * +-1; attention rand + 0.25, with `negated` a quarter of the ring planes negated (the r = 0 planes stay positive:
    D >= 0.25); about 10 % of the pixels measured"""
    R = K // 2
    gen = torch.Generator().manual_seed(1000 * K + 10 * W + C + 7 * seed + (3 if negated else 0))
    g = (torch.rand(B, K * K - 1, H, W, generator=gen) + 0.05) * ((torch.rand(B, K * K - 1, H, W, generator=gen) < 0.5).float() * 2 - 1)
    att = torch.rand(B, n * (R + 1), H, W, generator=gen) + 0.25
    if negated:
        ring_planes = [p for p in range(n * (R + 1)) if p % (R + 1)]
        for p in ring_planes[1::4] or ring_planes[:1]:
            att[:, p] = -att[:, p]
    x = torch.rand(B, C, H, W, generator=gen) * 10
    s = None
    if sparse:
        s = (torch.rand(B, 1, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, H, W, generator=gen) * 10 + 0.1)
        s.view(B, -1)[:, 0] = 3.5   # every image pins at least its first pixel
    go = torch.randn(B, C, H, W, generator=gen)
    return g, att, x, s, go


def _cuda(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def _fwd(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    e = float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-30))
    print("dyn fwd  %-52s %.3g of %g" % (what, e / RTOL, RTOL))
    assert np.isfinite(a).all() and e <= RTOL, "%s: relative error %.3g > %g" % (what, e, RTOL)


def _grad(a, ref, what):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    bound = GFLOOR * max(np.abs(ref).max(), 1e-30) + GTOL * np.abs(ref)
    print("dyn grad %-52s %.3g of the bound" % (what, float((np.abs(a - ref) / bound).max())))
    assert_close(a, ref, what, rtol=GTOL, atol_frac=GFLOOR)


# ---- CPU ----
def test_symbols_are_declared_and_exported_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert int(re.search(r"#define\s+CSPN_ABI_VERSION\s+(\d+)", text).group(1)) == 5
    assert len(cspn_amd.__all__) == ALL and not any("dyn" in n.lower() for n in cspn_amd.__all__)
    assert cspn_amd.Dynamic_Propagate is __import__("cspn_amd.dyspn", fromlist=["x"]).Dynamic_Propagate
    assert callable(F.cspn2d_forward_kxk_dyn) and callable(F.cspn2d_backward_kxk_dyn)


def test_byte_queries():
    fwd, bwd = _lib.late_symbol("cspn2d_kxk_dyn_workspace_bytes"), _lib.late_symbol("cspn2d_backward_kxk_dyn_workspace_bytes")
    hist = _lib.late_symbol("cspn2d_kxk_history_bytes")
    Bq, C, H, W = 2, 3, 10, 13
    L = 4 * Bq * C * H * W
    for K in (3, 5, 7):
        R = K // 2
        for n in (1, 2, 3, 6):
            for s in (0, 1):
                for keep in (0, 1):
                    levels = s + (0 if keep else min(n - 1, 2))
                    assert levels * L <= fwd(Bq, C, H, W, K, n, s, keep) <= levels * (L + 256) and fwd(Bq, C, H, W, K, n, s, keep) % 256 == 0
                parts = (n - 1) * L + 2 * R * 4 * Bq * H * W + s * L
                assert parts <= bwd(Bq, C, H, W, K, n, s) <= parts + 3 * 256 and bwd(Bq, C, H, W, K, n, s) % 256 == 0
            if K != 3:
                assert hist(Bq, C, H, W, K, n) == (n - 1) * L
        for n in (0, -1):
            assert fwd(Bq, C, H, W, K, n, 1, 0) == 0 and bwd(Bq, C, H, W, K, n, 1) == 0
    for K in (1, 4, 9, 0, -3):
        assert fwd(Bq, C, H, W, K, 4, 1, 0) == 0 and bwd(Bq, C, H, W, K, 4, 1) == 0
    for shape in ((0, 3, 10, 13), (2, 0, 10, 13), (2, 3, 0, 13), (2, 3, 10, 0), (-1, 3, 10, 13)):
        assert fwd(*shape, 5, 4, 1, 0) == 0 and bwd(*shape, 5, 4, 1) == 0
    big = (1 << 12, 1 << 8, 1 << 6, 1 << 6)        # B C H W = 2^32
    assert fwd(*big, 5, 3, 0, 0) == 0 and bwd(*big, 5, 3, 0) == 0
    assert fwd(1 << 8, 1, 1 << 10, 1 << 8, 7, 3, 0, 0) == 0 and bwd(1 << 8, 1, 1 << 10, 1 << 8, 7, 3, 0) == 0   # B KK H W > 2^31
    assert fwd(1 << 8, 1, 1 << 10, 1 << 8, 3, 30, 0, 0) == 0 and bwd(1 << 8, 1, 1 << 10, 1 << 8, 3, 30, 0) == 0   # B n (R+1) H W > 2^31


def test_argument_errors_are_those_of_the_absnorm_twins():
    """no call below reaches a launch: every one fails a check (or, needing nothing, returns 0) before the stream is touched"""
    g, a, x, s, o, h, w, gg, ga, gx, go = (ctypes.c_void_p(i << 32) for i in range(1, 12))
    hbytes = 4 * 2 * 8 * 8 * 2
    big = 1 << 22
    # (guidance, att, x, sparse, out, history, history_bytes, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    fwd = [((g, a, x, s, o, None, 0, 2, 1, 8, 8, K, 3, w, big, None), -1) for K in (4, 9, 0, 1)] + [
        ((None, a, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, None, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, None, s, o, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, x, s, None, None, 0, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, x, s, o, None, 0, 0, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, x, s, o, None, 0, 1, 0, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, x, s, o, None, 0, 1, 1, 8, 0, 5, 3, w, big, None), -1),
        ((g, a, x, s, o, None, 0, 2, 1, 8, 8, 5, -1, w, big, None), -1),
        ((g, a, x, s, x, None, 0, 2, 1, 8, 8, 7, 3, w, big, None), -1),      # out aliases x, the guidance, the attention, sparse
        ((g, a, x, s, g, None, 0, 2, 1, 8, 8, 7, 3, w, big, None), -1),
        ((g, a, x, s, a, None, 0, 2, 1, 8, 8, 3, 3, w, big, None), -1),
        ((g, a, x, s, s, None, 0, 2, 1, 8, 8, 3, 3, w, big, None), -1),
        ((g, a, x, s, o, a, big, 2, 1, 8, 8, 5, 3, w, big, None), -1),       # the history aliases the attention, sparse
        ((g, a, x, s, o, s, big, 2, 1, 8, 8, 5, 3, w, big, None), -1),
        ((g, a, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, a, big, None), -1),      # the workspace aliases the attention
        ((g, a, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, None, 0, None), -2),
        ((g, a, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, w, 100, None), -2),
        ((g, a, x, s, o, None, 0, 2, 1, 8, 8, 5, 3, ctypes.c_void_p((7 << 32) + 4), big, None), -2),
        ((g, a, x, s, o, h, 100, 2, 1, 8, 8, 5, 3, w, big, None), -2),
        ((g, a, x, s, o, None, 0, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, big, None), -3),
        ((g, a, x, s, o, None, 0, 1 << 8, 1, 1 << 10, 1 << 8, 7, 3, w, big, None), -3),
        ((g, a, x, s, o, None, 0, 1 << 8, 1, 1 << 10, 1 << 8, 3, 30, w, big, None), -3)]   # the attention planes alone are beyond 2^31 elements
    # (guidance, att, x, sparse, history, history_bytes, grad_out, grad_guidance, grad_att, grad_x, B, C, H, W, K, n_iter, ws, ws_bytes, stream)
    bwd = [((g, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 9, 3, w, big, None), -1),
           ((None, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, None, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, None, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 0, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, None, 0, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),       # the gradients need the history
           ((g, a, x, s, None, 0, go, None, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, 64, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, gg, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),     # two gradients in one place
           ((g, a, x, s, h, hbytes, go, gg, ga, ga, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, ga, gg, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, ga, go, 2, 1, 8, 8, 5, 3, w, big, None), -1),     # a gradient on an input
           ((g, a, x, s, h, hbytes, go, x, ga, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, a, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, s, gx, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, ga, h, 2, 1, 8, 8, 5, 3, w, big, None), -1),
           ((g, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, ga, big, None), -1),    # the workspace on grad_att
           ((g, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, None, 0, None), -2),
           ((g, a, x, s, h, hbytes, go, gg, ga, gx, 2, 1, 8, 8, 5, 3, w, 64, None), -2),
           ((g, a, x, s, h, hbytes, go, gg, ga, gx, 1 << 12, 1 << 8, 1 << 6, 1 << 6, 5, 3, w, big, None), -3),
           ((g, a, x, s, h, hbytes, go, None, None, None, 2, 1, 8, 8, 5, 3, w, big, None), 0)]   # nothing asked for: nothing done
    for name, cases in (("cspn2d_forward_kxk_dyn_f32", fwd), ("cspn2d_backward_kxk_dyn_f32", bwd)):
        f = _lib.late_symbol(name)
        for args, code in cases:
            assert f(*args) == code, (name, args)
            if code:
                assert name.encode() in cspn_amd.load().cspn_last_error()
    # the codes are the absnorm twin's on the arguments the two share (the twin has no att, no sparse and no K = 3)
    twin = _lib.late_symbol("cspn2d_forward_kxk_absnorm_f32")
    for args, code in fwd:
        if args[1] is a and args[11] in (5, 7) and args[12] == 3 and not any(p is not None and p.value in (a.value, s.value) for p in (args[4], args[5], args[13])):
            assert twin(args[0], args[2], *args[4:]) == code, args


def test_python_argument_errors_without_gpu():
    g, a, x = torch.zeros(1, 24, 4, 4), torch.zeros(1, 6, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_dyn(g, a, x, 7, 2)           # 24 channels are not 7 x 7
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_dyn(g, a, x, 5, 3)           # 6 attention planes are 2 steps of 5 x 5
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_dyn(g, a, x, 5, -1)
    with pytest.raises(ValueError):
        F.cspn2d_forward_kxk_dyn(g, a, x, 5, 2, sparse=x)  # sparse is one plane
    with pytest.raises(ValueError):
        F.cspn2d_backward_kxk_dyn(g, a, x, x[:, :1], 5, 2)
    for bad in (torch.float16, torch.bfloat16, torch.float64):
        for i in range(3):
            args = [g, a, x]
            args[i] = args[i].to(bad)
            with pytest.raises(TypeError):
                F.cspn2d_forward_kxk_dyn(*args, 5, 2)
            with pytest.raises(TypeError):
                cspn_amd.Dynamic_Propagate(2, 5)(*args)
        with pytest.raises(TypeError):
            F.cspn2d_forward_kxk_dyn(g, a, x, 5, 2, sparse=x[:, :1].to(bad))
    with pytest.raises(_lib.CspnError):
        F.cspn2d_forward_kxk_dyn(g, a, x, 5, 2)            # no CPU path
    assert F.cspn2d_forward_kxk_dyn(g, a[:, :0], x, 5, 0) is x
    for kw in ({"prop_kernel": 9}, {"attention": "relu"}, {"prop_time": -1}):
        with pytest.raises(ValueError):
            cspn_amd.Dynamic_Propagate(**dict({"prop_time": 2}, **kw))
    m = cspn_amd.Dynamic_Propagate(6)
    assert (m.prop_time, m.prop_kernel, m.attention) == (6, 7, None) and not list(m.parameters())
    assert cspn_amd.Dynamic_Propagate(2, 5)(g, a[:, :0], x, n_iter=0) is x


def test_the_statement_has_the_contracts_anchors():
    """float64, CPU: the identity attention; the ring attention on a non-negative guide is the demo module's step; the formulas of the backward
    (written out here) against autograd"""
    K, n, C, H, W = 5, 2, 2, 6, 9
    R = K // 2
    g, att, x, s, go = (None if t is None else t.double() for t in _inputs(H, W, K, C, True, True, n))
    ident = torch.zeros_like(att)
    ident[:, ::R + 1] = 1
    assert torch.equal(statement(g, ident, x, None, K, n)[0], x)
    ring = 1 - ident
    a = g.abs()
    ref = x
    for _ in range(n):
        ref = sum(a[:, k:k + 1] * _shift(ref, dy, dx) for k, (dy, dx) in enumerate(_offsets(K))) / a.sum(1, keepdim=True)
    assert float((statement(a, ring, x, None, K, n)[0] - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    # the backward as the header states it, one step
    gt, at, xt = g.clone().requires_grad_(True), att[:, :R + 1].clone().requires_grad_(True), x.clone().requires_grad_(True)
    out, _ = statement(gt, at, xt, s, K, 1)
    out.backward(go)
    offs = _offsets(K)
    rings = [max(abs(dy), abs(dx)) for dy, dx in offs]
    m = (s > 0).double()
    Ht = (1 - m) * x + m * s
    wh = [att[:, r:r + 1] * g[:, k:k + 1] for k, r in enumerate(rings)]
    D = att[:, 0:1] + sum(w.abs() for w in wh)
    e = [(go * (_shift(Ht, dy, dx) - Ht)).sum(1, keepdim=True) for dy, dx in offs]
    T = sum(w / D * ek for w, ek in zip(wh, e))
    dwh = [(ek - torch.sign(w) * T) / D for w, ek in zip(wh, e)]
    gatt = [-T / D] + [sum(g[:, k:k + 1] * dwh[k] for k in range(K * K - 1) if rings[k] == r) for r in range(1, R + 1)]
    gg = [att[:, r:r + 1] * d for r, d in zip(rings, dwh)]
    c = 1 - sum(w / D for w in wh)
    gx = (1 - m) * (c * go + sum(_shift(w * go / D, -dy, -dx) for w, (dy, dx) in zip(wh, offs)))
    for mine, auto in ((torch.cat(gatt, 1), at.grad), (torch.cat(gg, 1), gt.grad), (gx, xt.grad)):
        assert float((mine - auto).abs().max()) <= 1e-12 * float(auto.abs().max())


# ---- 1. against the float64 statement ----
_REF = {}


def _reference(name, K, C, sparse, negated):
    """(inputs, H_n, kept levels, dL/dguidance, dL/datt, dL/dx) of the float64 statement, computed once per case"""
    key = (name, K, C, sparse, negated)
    if key not in _REF:
        H, W = SHAPES[name]
        inp = _inputs(H, W, K, C, sparse, negated)
        g, att, x, s, go = (None if t is None else t.double() for t in inp)
        g, att, x = g.requires_grad_(True), att.requires_grad_(True), x.requires_grad_(True)
        out, kept = statement(g, att, x, s, K, N_ITER)
        out.backward(go)
        _REF[key] = (inp, out.detach(), [k.detach() for k in kept], g.grad, att.grad, x.grad)
    return _REF[key]


@pytest.mark.gpu
@pytest.mark.parametrize("negated", [False, True])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_levels_and_gradients_vs_fp64_statement(name, K, C, sparse, negated):
    inp, r_out, r_kept, r_gg, r_ga, r_gx = _reference(name, K, C, sparse, negated)
    g, att, x, s, go = _cuda(*inp)
    H, W = SHAPES[name]
    what = "%s K=%d C=%d%s%s" % (name, K, C, " sparse" if sparse else "", " negated" if negated else "")
    out = F.cspn2d_forward_kxk_dyn(g, att, x, K, N_ITER, s)
    out_h, hist = F.cspn2d_forward_kxk_dyn(g, att, x, K, N_ITER, s, return_history=True)
    assert torch.equal(out, out_h)
    _fwd(out.cpu().numpy(), r_out.numpy(), what + " out")
    levels = hist[:(N_ITER - 1) * B * C * H * W].view(N_ITER - 1, B, C, H, W).cpu()
    for t, ref in enumerate(r_kept):
        _fwd(levels[t].numpy(), ref.numpy(), what + " level %d" % (t + 1))
    gg, ga, gx = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, s, hist)
    _grad(gx.cpu().numpy(), r_gx.numpy(), what + " dL/dx")
    _grad(ga.cpu().numpy(), r_ga.numpy(), what + " dL/datt")
    _grad(gg.cpu().numpy(), r_gg.numpy(), what + " dL/dguidance")
    # without a history the backward runs the forward itself; one gradient alone is the same bits
    gg2, ga2, gx2 = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, s)
    assert torch.equal(gg2, gg) and torch.equal(ga2, ga) and torch.equal(gx2, gx)
    only = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, s, hist, need_guidance=False, need_x=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], ga)
    only = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, s, None, need_att=False, need_x=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], gg)
    only = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, s, None, need_guidance=False, need_att=False)
    assert only[0] is None and only[1] is None and torch.equal(only[2], gx)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 7])
@pytest.mark.parametrize("n", [1, 2, 6])
def test_other_step_counts_vs_fp64_statement(K, n):
    """n = 1 (no level is kept, no adjoint level), n = 2 (one ping-pong level), n = 6 (the module's default), on the guarded path with sparse"""
    H, W = SHAPES["tall"]
    inp = _inputs(H, W, K, 2, True, True, n)
    g, att, x, s, go = (t.double() for t in inp)
    g, att, x = g.requires_grad_(True), att.requires_grad_(True), x.requires_grad_(True)
    r_out, _ = statement(g, att, x, s, K, n)
    r_out.backward(go)
    gd, ad, xd, sd, god = _cuda(*inp)
    what = "tall K=%d n=%d" % (K, n)
    _fwd(F.cspn2d_forward_kxk_dyn(gd, ad, xd, K, n, sd).cpu().numpy(), r_out.detach().numpy(), what + " out")
    gg, ga, gx = F.cspn2d_backward_kxk_dyn(gd, ad, xd, god, K, n, sd)
    _grad(gx.cpu().numpy(), x.grad.numpy(), what + " dL/dx")
    _grad(ga.cpu().numpy(), att.grad.numpy(), what + " dL/datt")
    _grad(gg.cpu().numpy(), g.grad.numpy(), what + " dL/dguidance")


# ---- 2. anchors ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_identity_attention_returns_x_and_grad_out(name, K):
    H, W = SHAPES[name]
    R = K // 2
    g, att, x, _, go = _cuda(*_inputs(H, W, K, 2, False, False))
    att.zero_()
    att[:, ::R + 1] = 1
    out, hist = F.cspn2d_forward_kxk_dyn(g, att, x, K, N_ITER, return_history=True)
    assert torch.equal(out, x)
    gx = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, N_ITER, None, hist)[2]
    assert torch.equal(gx.view(torch.int32), go.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("name", ["wide", "strip"])
def test_ring_attention_on_a_nonnegative_guide_is_the_absnorm_step(name, K):
    H, W = SHAPES[name]
    R = K // 2
    g, att, x, _, _ = _cuda(*_inputs(H, W, K, 2, False, False))
    g = g.abs()
    att.fill_(1)
    att[:, ::R + 1] = 0
    ref = F.cspn2d_forward_kxk_absnorm(g, x, K, N_ITER)
    _fwd(F.cspn2d_forward_kxk_dyn(g, att, x, K, N_ITER).cpu().numpy(), ref.cpu().numpy(), "%s K=%d vs absnorm" % (name, K))


# ---- 3. adjointness, determinism ----
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_step_and_adjoint_step_are_adjoint(name, K, n):
    H, W = SHAPES[name]
    g, att, x, _, y = _cuda(*_inputs(H, W, K, 2, False, True, n))
    fx = F.cspn2d_forward_kxk_dyn(g, att, x, K, n)
    none, none2, bty = F.cspn2d_backward_kxk_dyn(g, att, x, y, K, n, need_guidance=False, need_att=False)
    assert none is None and none2 is None
    lhs, rhs = float((fx.double() * y.double()).sum()), float((x.double() * bty.double()).sum())
    scale = float((fx.double() * y.double()).abs().sum())
    print("dyn adj  %-52s %.3g of the bound" % ("%s K=%d n=%d" % (name, K, n), abs(lhs - rhs) / (ATOL_ADJ * scale)))
    assert np.isfinite(lhs) and np.isfinite(rhs) and scale > 0
    assert abs(lhs - rhs) <= ATOL_ADJ * scale, "<F x, y> = %.9g, <x, F^T y> = %.9g, sum |F x y| = %.6g" % (lhs, rhs, scale)


def _all_outputs(K, n, g, att, x, s, go):
    out, hist = F.cspn2d_forward_kxk_dyn(g, att, x, K, n, s, return_history=True)
    return (out, hist) + tuple(F.cspn2d_backward_kxk_dyn(g, att, x, go, K, n, s, hist))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
def test_two_calls_give_the_same_bits(K):
    H, W = SHAPES["wide"]
    inputs = _cuda(*_inputs(H, W, K, 2, True, True))
    memguard.assert_same_outputs(_all_outputs(K, N_ITER, *inputs), _all_outputs(K, N_ITER, *inputs), "second call")


# ---- 4. the module ----
@pytest.mark.gpu
@pytest.mark.parametrize("attention", [None, "sigmoid", "softmax"])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_module_gives_the_functional_calls_bits(K, attention):
    H, W = SHAPES["tall"]
    R, n = K // 2, N_ITER
    g, att, x, s, go = _cuda(*_inputs(H, W, K, 2, True, True))
    raw = att if attention is None else (att - 0.75) * 3   # the logits a head would emit
    act = {None: lambda t: t, "sigmoid": torch.sigmoid,
           "softmax": lambda t: torch.softmax(t.view(B, n, R + 1, H, W), 2).view(B, n * (R + 1), H, W)}[attention]
    al = raw.clone().requires_grad_(True)
    a = act(al)
    out, hist = F.cspn2d_forward_kxk_dyn(g, a.detach(), x, K, n, s, return_history=True)
    gg, ga, gx = F.cspn2d_backward_kxk_dyn(g, a.detach(), x, go, K, n, s, hist)
    a.backward(ga)
    m = cspn_amd.Dynamic_Propagate(n, K, attention)
    with torch.no_grad():
        assert torch.equal(m(g, raw, x, s), out)
    gr, ar, xr = g.clone().requires_grad_(True), raw.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = m(gr, ar, xr, s)
    assert torch.equal(y.detach(), out)
    y.backward(go)
    assert torch.equal(gr.grad, gg) and torch.equal(xr.grad, gx) and torch.equal(ar.grad, al.grad)
    # n_iter overrides prop_time
    other = cspn_amd.Dynamic_Propagate(9, K, attention)
    with torch.no_grad():
        assert torch.equal(other(g, raw, x, s, n_iter=n), out)
        assert torch.equal(other(g, raw[:, :R + 1], x, s, n_iter=1), F.cspn2d_forward_kxk_dyn(g, act(raw)[:, :R + 1].contiguous(), x, K, 1, s))
    # one gradient alone
    ar = raw.clone().requires_grad_(True)
    m(g, ar, x, s).backward(go)
    assert torch.equal(ar.grad, al.grad)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            m(g.to(dt), raw, x, s)
        with pytest.raises(TypeError):
            m(g, raw.to(dt), x, s)


# ---- 5. memory ----
@pytest.mark.gpu
def test_a_training_step_keeps_no_modulated_gate():
    """peak memory over one training step of the module at 67 x 70, K = 7, n = 6 stays within the inputs, the output, the history, the two workspace
    queries, the three gradients and 1 MiB: the n KK modulated planes of the composed route (10.8 MB here) have no room in that"""
    K, n, C = 7, 6, 1
    H, W = SHAPES["tall"]
    g, att, x, s, go = _cuda(*_inputs(H, W, K, C, True, False, n))
    m = cspn_amd.Dynamic_Propagate(n, K)
    leaves = [t.clone().requires_grad_(True) for t in (g, att, x)]
    m(*leaves, s).backward(go)   # warm: symbols bound
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()

    def nbytes(*ts):
        return sum(t.numel() * t.element_size() for t in ts)

    ws = (_lib.symbol("cspn2d_kxk_dyn_workspace_bytes")(B, C, H, W, K, n, 1, 1) + _lib.symbol("cspn2d_backward_kxk_dyn_workspace_bytes")(B, C, H, W, K, n, 1))
    hist = _lib.symbol("cspn2d_kxk_history_bytes")(B, C, H, W, K, n)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()   # the inputs
    out = m(*leaves, s)
    out.backward(go)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    budget = nbytes(out) + hist + ws + nbytes(*leaves) + (1 << 20)
    print("dyn mem  training step: %d bytes beyond the inputs, %.3g of the budget %d (n KK planes: %d)" % (extra, extra / budget, budget, n * nbytes(g)))
    assert all(t.grad is not None for t in leaves) and extra <= budget and budget < n * nbytes(g)


# ---- 6. memory hygiene: every call between guard bands on NaN and on finite poison, and in a stale arena ----
def _hygiene_inputs(K, H, W, C, sparse):
    return _cuda(*_inputs(H, W, K, C, sparse, True, seed=5))


def _hygiene_call(K):
    def call(g, att, x, s, go):
        n = N_ITER
        out = F.cspn2d_forward_kxk_dyn(g, att, x, K, n, s)
        out2, hist = F.cspn2d_forward_kxk_dyn(g, att, x, K, n, s, return_history=True)
        grads = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, n, s, hist)
        alone = F.cspn2d_backward_kxk_dyn(g, att, x, go, K, n, s, None, False, True, False)[1]
        one = F.cspn2d_forward_kxk_dyn(g, att[:, :K // 2 + 1].contiguous(), x, K, 1, s)
        leaves = [hygiene._leaf(t) for t in (g, att, x)]
        y = cspn_amd.Dynamic_Propagate(n, K, "sigmoid")(*leaves, s)
        y.backward(go)
        return (out, out2, hist) + tuple(grads) + (alone, one, y.detach()) + tuple(t.grad for t in leaves)
    return call


HYGIENE = {}
for _K, _name, _C, _sparse in ((3, "tall", 2, True), (5, "wide", 1, True), (7, "wide", 2, False), (7, "strip", 1, True)):
    _H, _W = SHAPES[_name]
    _n = "kxk-dyn-K%d-%dx%d" % (_K, _H, _W)
    HYGIENE[_n] = hygiene.Case(_n, tuple(NEW), "the kxk_dyn entry points and Dynamic_Propagate", 4 * B * _C * _H * _W,
                               functools.lru_cache(maxsize=None)(functools.partial(_hygiene_inputs, _K, _H, _W, _C, _sparse)), _hygiene_call(_K),
                               lambda: None, "test_kxk_dyn.py::test_forward_levels_and_gradients_vs_fp64_statement", False, None, None)


def test_the_guarded_cases_stay_out_of_the_shared_table():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True}
    assert not any("dyn" in n for c in hygiene.CASES.values() for n in c.covers)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_call_between_guard_bands(name, poison):
    """every output (out, the history, the three gradients) and every workspace lies between guard bands and is poisoned before the call: clean
    outputs (bitwise the unguarded run's, so fully written), intact bands, unchanged inputs"""
    c = HYGIENE[name]
    inputs = c.build()
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, inputs, "cuda", c.plane)
    assert len(session.workspaces) >= 5 and len(session.guards) > len(session.workspaces)
    for o in outs:
        assert o is None or bool(torch.isfinite(o.float()).all()), "poison reached an output"
    memguard.assert_same_outputs(outs, hygiene._clean(c), "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    """the calls of every case through one workspace arena that is never refilled: every result bitwise the clean one"""
    steps = []
    for name in ("kxk-dyn-K7-35x196", "kxk-dyn-K3-67x70", "kxk-dyn-K5-35x196", "kxk-dyn-K7-18x259", "kxk-dyn-K7-35x196"):
        c = HYGIENE[name]
        steps.append((name, c.call, c.build()))
    hygiene._run_sequence(steps, 4 * B * 2 * 35 * 196)


# ---- 7. a captured graph ----
@pytest.mark.gpu
def test_a_captured_graph_replays_the_eager_bits():
    K, n = 5, N_ITER
    H, W = 40, 136
    g, att, x, s, go = _cuda(*_inputs(H, W, K, 2, True, True))
    att2 = _inputs(H, W, K, 2, True, False, seed=1)[1].cuda()
    ref = _all_outputs(K, n, g, att, x, s, go)
    ref2 = _all_outputs(K, n, g, att2, x, s, go)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream, one chain: forward, then backward on its history
        cap = _all_outputs(K, n, g, att, x, s, go)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        memguard.assert_same_outputs(cap, ref, "replay")
    att.copy_(att2)   # new contents behind the captured pointers
    graph.replay()
    torch.cuda.synchronize()
    memguard.assert_same_outputs(cap, ref2, "replay on new contents")
