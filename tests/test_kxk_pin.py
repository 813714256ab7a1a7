"""K x K propagation pinned to the measured depth with a per-pixel confidence (CSPN++ / PENet): the depth-completion and the assembling
contract of the K x K engine with the blend after every step
    H_{t+1} = (1 - m) * step(H_t) + m * sparse,      m = sign(sparse) * pin_conf,      H_0 = blur
(cspn2d_*_kxk_{norm,assemble}_pin; F.cspn2d_*_kxk_{norm,assemble}_pin; the keyword `pin_conf` of Affinity_PropagateKxK and
Affinity_PropagateAssemble).  sparse enters by its value, pin_conf is used as given.
CPU: the float64 statement written twice (padded, with the blend line; shift-based and folded) and its anchors on the existing contract's
     statements, symbols, argument errors of the ABI and of Python, module signatures and reprs, the thinned grid's coverage.
GPU: forward and every gradient against the float64 statement under autograd, bitwise anchors against the existing engine calls, 16-bit
     guidance, gradient subsets, repeatability and misaligned views, guard bands and a stale arena, the modules and the two-pass PENet
     composition, the NaN rule.  Bounds: RTOL and test_backward._check, the project's own."""
import contextlib
import ctypes
import functools
import inspect
import itertools
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
from helpers import rel_err
from test_backward import _check
from test_kxk_dilation import _conf, _offsets, _pads, _shift, torch_kxk_assemble_dil, torch_kxk_norm_dil
from test_kxk_norm import RTOL, _cuda, _misaligned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_forward_kxk_norm_pin", "cspn2d_backward_kxk_norm_pin", "cspn2d_forward_kxk_assemble_pin", "cspn2d_backward_kxk_assemble_pin"]
NORMS = ["8sum", "8sum_abs"]
N_ITER = 5
STEPS = (0, 2, 5)


# ---- the float64 statement, twice ----
def pin_levels_padded(guidance, blur, sparse, pin, K, n, norm, D):
    """the reference's padded normalisation and loop (test_kxk_dilation.torch_kxk_levels_dil) with the blend line of the pinned contract -> [H_0 .. H_n]"""
    c = (K // 2) * D
    P = _pads(K, D)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, c:-c, c:-c]
    gate = gate.unsqueeze(2)
    m = sparse.sign() * pin
    x = blur
    levels = [x]
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, c:-c, c:-c]
        x = (1 - m) * x + m * sparse
        levels.append(x)
    return levels


def pin_levels_folded(guidance, blur, sparse, pin, K, n, norm, D):
    """the contract as the header states it, with shifts and folded: G_k(p) = g_k(p + off_k), wb = G / sum |G|, cc = 1 - sum wb, u = 1 - m,
    w'_k = u wb_k, b = (u cc) blur + m sparse, H' = sum_k w'_k H(p + off_k) + b"""
    off = _offsets(K, D)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    G = torch.stack([_shift(g[:, k], dy, dx) for k, (dy, dx) in enumerate(off)], 1)
    wb = G / G.abs().sum(1, keepdim=True)
    cc = 1 - wb.sum(1, keepdim=True)
    m = sparse.sign() * pin
    u = 1 - m
    b = (u * cc) * blur + m * sparse
    x = blur
    levels = [x]
    for _ in range(n):
        acc = torch.zeros_like(blur)
        for k, (dy, dx) in enumerate(off):
            acc = acc + (u * wb[:, k:k + 1]) * _shift(x, dy, dx)
        x = acc + b
        levels.append(x)
    return levels


def pin_norm(guidance, blur, sparse, pin, K, n, norm, D, levels=pin_levels_padded):
    return levels(guidance, blur, sparse, pin, K, n, norm, D)[-1]


def pin_assemble(guidance, blur, sparse, pin, conf, steps, K, norm, D, levels=pin_levels_padded):
    lv = levels(guidance, blur, sparse, pin, K, steps[-1], norm, D)
    out = conf[:, 0:1] * lv[steps[0]]
    for j in range(1, len(steps)):
        out = out + conf[:, j:j + 1] * lv[steps[j]]
    return out


def _pin_inputs(B, C, H, W, K, planes, seed):
    """raw signed guidance, depths in [0.1, 10), a 10 % mask of `planes` ("shared": one plane, "per": C) with one negative value, pin_conf uniform in [0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, K * K - 1, H, W, generator=gen)
    h = torch.rand(B, C, H, W, generator=gen) * 9.9 + 0.1
    sc = 1 if planes == "shared" else C
    s = (torch.rand(B, sc, H, W, generator=gen) < 0.1).float() * (torch.rand(B, sc, H, W, generator=gen) * 9.9 + 0.1)
    s.view(-1)[min(3, s.numel() - 1)] = -2.5
    p = torch.rand(B, sc, H, W, generator=gen)
    return g, h, s, p


# ---- the GPU grid, thinned: every K and norm at every shape; the dilation, the mask planes and the call rotate so that each of their values meets each shape ----
# the tile is 64 x 16 pixels, the halo at K = 7, D = 2 is 6: one exact tile; the scalar path with seams; 3 x 3 tiles on the vector path; smaller than the halo
SHAPES = [(16, 64), (17, 65), (33, 132), (5, 8)]
CASES = [(K, norm, H, W, (1, 2)[(i + j) % 2], ("shared", "per")[(i // 2 + j) % 2], ("norm", "assemble")[(i // 3 + j) % 2])
         for i, (K, norm) in enumerate(itertools.product((3, 5, 7), NORMS)) for j, (H, W) in enumerate(SHAPES)]
B, C = 2, 3


def _seed(K, norm, H, W, D, planes, call):
    return K * 1000 + W * 10 + D + 100 * NORMS.index(norm)


# ---- CPU ----
@pytest.mark.parametrize("K", [3, 5, 7])
def test_the_two_statements_agree(K):
    for (H, W), norm, planes, D in (((5, 8), "8sum", "shared", 2), ((9, 14), "8sum_abs", "per", 1), ((17, 21), "8sum", "per", 2), ((6, 7), "8sum_abs", "shared", 1)):
        g, h, s, p = (t.double() for t in _pin_inputs(2, 2, H, W, K, planes, seed=K + W))
        a, b = pin_levels_padded(g, h, s, p, K, 3, norm, D), pin_levels_folded(g, h, s, p, K, 3, norm, D)
        for x, y in zip(a, b):
            assert bool(torch.isfinite(x).all()) and float((x - y).abs().max()) <= 1e-12, (H, W)
        cf = _conf(2, 2, H, W, K).double()
        x, y = pin_assemble(g, h, s, p, cf, (1, 3), K, norm, D), pin_assemble(g, h, s, p, cf, (1, 3), K, norm, D, pin_levels_folded)
        assert float((x - y).abs().max()) <= 1e-12
        assert not torch.equal(a[-1], torch_kxk_norm_dil(g, h, s, K, 3, norm, D))   # a soft pin to the measurement is not the hard pin to blur


def _anchor_one(h, s):
    """the inputs of the pin_conf = 1 anchor: sparse >= 0, blur = sparse where sparse > 0"""
    s = s.abs()
    return torch.where(s > 0, s.expand_as(h), h), s


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("statement", [pin_levels_padded, pin_levels_folded])
def test_anchors_of_the_statement(K, statement):
    """pin_conf = 1 on measurements the blur already holds is the existing contract, pin_conf = 0 the contract without a mask: exactly, and the
    same for the assembled sum (the padded statement has the existing statement's operations, so its bits; the folded one agrees to rounding)"""
    exact = statement is pin_levels_padded
    for (H, W), norm, planes, D in (((5, 8), "8sum", "shared", 2), ((9, 14), "8sum_abs", "per", 1), ((17, 21), "8sum", "per", 2)):
        g, h, s, p = (t.double() for t in _pin_inputs(2, 2, H, W, K, planes, seed=K + H))
        cf = _conf(2, 3, H, W, K).double()
        h1, s1 = _anchor_one(h, s)
        pairs = [(pin_norm(g, h1, s1, torch.ones_like(p), K, 4, norm, D, statement), torch_kxk_norm_dil(g, h1, s1, K, 4, norm, D)),
                 (pin_norm(g, h, s, torch.zeros_like(p), K, 4, norm, D, statement), torch_kxk_norm_dil(g, h, None, K, 4, norm, D)),
                 (pin_assemble(g, h1, s1, torch.ones_like(p), cf, (0, 2, 4), K, norm, D, statement), torch_kxk_assemble_dil(g, h1, s1, cf, (0, 2, 4), K, norm, D)),
                 (pin_assemble(g, h, s, torch.zeros_like(p), cf, (0, 2, 4), K, norm, D, statement), torch_kxk_assemble_dil(g, h, None, cf, (0, 2, 4), K, norm, D))]
        for i, (a, b) in enumerate(pairs):
            assert bool(torch.isfinite(b).all())
            assert torch.equal(a, b) if exact else float((a - b).abs().max()) <= 1e-12, (H, W, i)


def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text)
        assert m, "not declared: " + s
        args = m.group(1)
        assert re.search(r"const float\* sparse,\s*const float\* pin_conf", args) and re.search(r"int K,\s*int dilation,\s*int n_iter", args), s
        assert "int gate_dtype" in args and ("backward" not in s or re.search(r"float\* grad_sparse,\s*float\* grad_pin", args)), s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    # the feature's top-level surface is the pin_conf keyword of two exported modules: no new public name
    assert not any("pin" in n for n in cspn_amd.__all__) and not any(hasattr(cspn_amd, s) for s in NEW)
    assert all(callable(getattr(F, s)) for s in NEW)


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    nf, nb, af, ab = (_lib.late_symbol(s) for s in NEW)
    g, x, s, p, o, h, w, gg, gx, cf, gc, gs, gp = (ctypes.c_void_p(i << 32) for i in range(1, 14))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    steps = (ctypes.c_int * 3)(0, 2, 3)
    hb = 4 * 2 * 8 * 8 * 3
    # (.., B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws, ws_bytes, stream) behind each entry's own pointers
    calls = {
        "norm forward": lambda K, D, dt=0, ws=M, s=s, p=p, sc=1: nf(g, dt, x, s, p, o, None, 0, 2, 1, sc, 8, 8, K, D, 3, 0, w, ws, None),
        "norm backward": lambda K, D, dt=0, ws=M, s=s, p=p, sc=1: nb(g, dt, x, s, p, h, hb, o, gg, gx, gs, gp, 2, 1, sc, 8, 8, K, D, 3, 0, w, ws, None),
        "assemble forward": lambda K, D, dt=0, ws=M, s=s, p=p, sc=1: af(g, dt, x, s, p, cf, steps, 3, o, None, 0, 2, 1, sc, 8, 8, K, D, 3, 0, w, ws, None),
        "assemble backward": lambda K, D, dt=0, ws=M, s=s, p=p, sc=1: ab(g, dt, x, s, p, cf, steps, 3, h, hb, o, gg, gx, gc, gs, gp, 2, 1, sc, 8, 8, K, D, 3, 0, w, ws,
                                                                         None),
    }
    for what, call in calls.items():
        # the pin is checked first: before the dilation and before K
        for kw in (dict(s=None), dict(p=None), dict(sc=0), dict(s=None, sc=0)):
            assert call(4, 0, **kw) == -1 and b"the pin needs" in err(), (what, kw)
        for D in (0, 3, -1, 4):
            assert call(5, D) == -1 and b"dilation" in err(), (what, D)
        assert call(4, 0) == -1 and b"dilation" in err(), what
        for D in (1, 2):   # the counterpart's checks are reached, at both dilations
            assert call(4, D) == -1 and b"K must be" in err(), (what, D)
            assert call(5, D, 7) == -1 and b"dtype" in err(), (what, D)
            assert call(5, D, 0, 64) == -2 and b"workspace" in err(), (what, D)
            assert call(5, D, _lib.DTYPES["float16"], 64) == -2, (what, D)
            assert call(5, D, sc=2) == -1 and b"sparse_C" in err(), (what, D)
    assert nf(None, 0, x, s, p, o, None, 0, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"null" in err()
    assert nf(g, 0, x, s, p, p, None, 0, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"alias" in err()   # out on pin_conf
    assert nf(g, 0, x, s, p, o, None, 0, 2, 1, 1, 8, 8, 5, 2, 3, 2, w, M, None) == -1 and b"norm" in err()
    # dL/dpin needs the history as dL/dguidance does; dL/dsparse and dL/dblur do not
    assert nb(g, 0, x, s, p, None, 0, o, None, None, None, gp, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"history" in err()
    assert nb(g, 0, x, s, p, None, 0, o, gg, None, None, None, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"history" in err()
    assert ab(g, 0, x, s, p, cf, steps, 3, None, 0, o, None, None, None, None, gp, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"history" in err()
    assert nb(g, 0, x, s, p, h, hb, o, gg, gx, gs, gs, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"alias" in err()   # grad_pin on grad_sparse
    assert nb(g, 0, x, s, p, h, hb, o, gg, gx, p, gp, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"alias" in err()    # grad_sparse on pin_conf
    assert ab(g, 0, x, s, p, cf, steps, 3, h, hb, o, gg, gx, gc, gs, gx, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"alias" in err()
    bad = (ctypes.c_int * 3)(0, 2, 2)
    assert af(g, 0, x, s, p, cf, bad, 3, o, None, 0, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"steps" in err()
    assert ab(g, 0, x, s, p, None, steps, 3, h, hb, o, gg, gx, gc, gs, gp, 2, 1, 1, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"conf" in err()


def test_python_argument_errors_without_gpu():
    g, h, cf, go = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 2, 6, 9)
    s1, s2, p1, p2 = torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9)
    calls = {
        "nf": lambda s, p, **k: F.cspn2d_forward_kxk_norm_pin(g, h, s, p, 5, 3, **k),
        "nb": lambda s, p, **k: F.cspn2d_backward_kxk_norm_pin(g, h, s, p, go, 5, 3, **k),
        "af": lambda s, p, **k: F.cspn2d_forward_kxk_assemble_pin(g, h, s, p, cf, (1, 3), 5, 3, **k),
        "ab": lambda s, p, **k: F.cspn2d_backward_kxk_assemble_pin(g, h, s, p, cf, (1, 3), go, 5, 3, **k),
    }
    for what, call in calls.items():
        with pytest.raises(ValueError, match="pin_conf"):   # a pin without a sparse_depth
            call(None, p1)
        with pytest.raises(ValueError, match="pin_conf"):   # a sparse_depth without a pin: this is the pinned call
            call(s1, None)
        for s, p in ((s1, p2), (s2, p1)):                   # mismatched plane counts
            with pytest.raises(ValueError, match="pin_conf"):
                call(s, p)
        with pytest.raises(ValueError, match="pin_conf"):   # a wrong shape
            call(s1, torch.rand(1, 1, 6, 8))
        with pytest.raises(ValueError, match="sparse_depth"):   # neither 1 nor C planes
            call(torch.rand(1, 3, 6, 9), torch.rand(1, 3, 6, 9))
        for bad in (0, 3, True, "2", None):
            with pytest.raises(ValueError, match="dilation"):
                call(s1, p1, dilation=bad)
        with pytest.raises(cspn_amd.CspnError):   # a well-formed call on the CPU reaches the engine, which is GPU-only
            call(s2, p2, dilation=2)
    assert F.cspn2d_forward_kxk_norm_pin(g, h, s1, p1, 5, 0) is h
    assert F.cspn2d_forward_kxk_norm_pin(g, h, s1, p1, 5, 0, return_history=True) == (h, None)
    with pytest.raises(ValueError, match="n_iter"):
        F.cspn2d_forward_kxk_assemble_pin(g, h, s1, p1, cf[:, :1], (0,), 5, 0)
    with pytest.raises(ValueError, match="kernel_size"):
        F.cspn2d_forward_kxk_norm_pin(g, h, s1, p1, 4, 3)
    # the modules: a pin without a sparse_depth; the sequence's length; n_iter = 0
    kxk, asm = cspn_amd.Affinity_PropagateKxK(3, 5), cspn_amd.Affinity_PropagateAssemble(3, (5, 5), (1, 3))
    with pytest.raises(ValueError, match="pin_conf"):
        kxk(g, h, None, pin_conf=p1)
    with pytest.raises(ValueError, match="pin_conf"):
        asm([g, g], h, None, pin_conf=p1)
    with pytest.raises(ValueError, match="pin_conf"):
        asm([g, g], h, s1, pin_conf=[p1])
    assert kxk(g, h, s1, n_iter=0, pin_conf=p1) is h and asm([g, g], h, s1, n_iter=0, pin_conf=[p1, p1]) is h
    for call in (lambda: kxk(g, h, s1, pin_conf=p1), lambda: asm([g, g], h, s1, pin_conf=p1), lambda: asm([g, g], h, s2, pin_conf=(p2, p2)),
                 lambda: cspn_amd.Affinity_PropagateKxK(3, 3)(torch.rand(1, 8, 6, 9), h, s1, pin_conf=p1)):   # K = 3, dilation 1: the engine, not the ring
        with pytest.raises(cspn_amd.CspnError):
            call()


def test_signatures_and_unchanged_reprs():
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(F.cspn2d_forward_kxk_norm_pin) == "guidance blur_depth sparse_depth pin_conf kernel_size n_iter norm_type return_history dilation".split()
    assert sig(F.cspn2d_backward_kxk_norm_pin) == ("guidance blur_depth sparse_depth pin_conf grad_out kernel_size n_iter norm_type history need_guidance need_blur "
                                                   "need_sparse need_pin dilation").split()
    assert sig(F.cspn2d_forward_kxk_assemble_pin) == "guidance blur_depth sparse_depth pin_conf conf steps kernel_size n_iter norm_type return_history dilation".split()
    assert sig(F.cspn2d_backward_kxk_assemble_pin) == ("guidance blur_depth sparse_depth pin_conf conf steps grad_out kernel_size n_iter norm_type history need_guidance "
                                                       "need_blur need_conf need_sparse need_pin dilation").split()
    for f in (F.cspn2d_backward_kxk_norm_pin, F.cspn2d_backward_kxk_assemble_pin):
        p = inspect.signature(f).parameters
        assert p["need_sparse"].default is True and p["need_pin"].default is True and p["dilation"].default == 1
    assert sig(cspn_amd.Affinity_PropagateKxK.forward) == "self guidance blur_depth sparse_depth n_iter pin_conf".split()
    assert sig(cspn_amd.Affinity_PropagateAssemble.forward) == "self guidances blur_depth sparse_depth iter_conf kernel_conf n_iter pin_conf".split()
    assert all(inspect.signature(m.forward).parameters["pin_conf"].default is None for m in (cspn_amd.Affinity_PropagateKxK, cspn_amd.Affinity_PropagateAssemble))
    assert sig(cspn_amd.Affinity_PropagateKxK.__init__) == "self prop_time prop_kernel norm_type dilation".split()
    assert sig(cspn_amd.Affinity_PropagateAssemble.__init__) == "self prop_time prop_kernels steps norm_type dilations".split()
    assert repr(cspn_amd.Affinity_PropagateKxK(24, 5)) == "Affinity_PropagateKxK(prop_time=24, prop_kernel=5, norm_type='8sum')"
    assert repr(cspn_amd.Affinity_PropagateKxK(24, 7, "8sum_abs", 2)) == "Affinity_PropagateKxK(prop_time=24, prop_kernel=7, norm_type='8sum_abs', dilation=2)"
    assert repr(cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5))) == \
        "Affinity_PropagateAssemble(prop_time=5, prop_kernels=(3, 5, 7), steps=(0, 2, 5), norm_type='8sum')"
    m = cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5), "8sum", 2)
    assert "dilations=(2, 2, 2)" in repr(m) and list(m.parameters()) == [] and m.state_dict() == {}


def test_the_grid_reaches_every_value_of_every_factor_at_every_shape():
    assert len(CASES) == 24 and {c[2:4] for c in CASES} == set(SHAPES)
    for shape in SHAPES:
        rows = [c for c in CASES if c[2:4] == shape]
        assert {c[0] for c in rows} == {3, 5, 7} and {c[1] for c in rows} == set(NORMS) and {c[4] for c in rows} == {1, 2}
        assert {c[5] for c in rows} == {"shared", "per"} and {c[6] for c in rows} == {"norm", "assemble"}
    for K in (3, 5, 7):
        rows = [c for c in CASES if c[0] == K]
        assert {c[4] for c in rows} == {1, 2} and {c[5] for c in rows} == {"shared", "per"} and {c[6] for c in rows} == {"norm", "assemble"}


def test_every_case_pins_at_least_four_pixels_per_tensor():
    """dL/dpin is exactly 0 where sparse == 0, so a case must hold pixels where it is not: at least 4 per mask tensor, one of them negative"""
    for case in CASES:
        K, norm, H, W, D, planes, call = case
        _, _, s, p = _pin_inputs(B, C, H, W, K, planes, _seed(*case))
        assert int((s != 0).sum()) >= 4 and int((s < 0).sum()) == 1 and float(p.min()) >= 0 and float(p.max()) < 1, case
        assert tuple(s.shape) == tuple(p.shape) == (B, 1 if planes == "shared" else C, H, W)


# ---- GPU ----
@functools.lru_cache(maxsize=None)
def _case(K, norm, H, W, D, planes, call):
    """inputs (each drawn and placed on the device on its own), the float64 statement with its autograd gradients, the engine's results: made once"""
    seed = _seed(K, norm, H, W, D, planes, call)
    g, h, s, p = _pin_inputs(B, C, H, W, K, planes, seed)
    cf = _conf(B, len(STEPS), H, W, seed + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2))
    leaves = [t.double().requires_grad_(True) for t in (g, h, s, p, cf)]
    if call == "norm":
        ref = pin_norm(*leaves[:4], K, N_ITER, norm, D)
    else:
        ref = pin_assemble(*leaves, STEPS, K, norm, D)
    ref.backward(go.double())
    dev = _cuda(g, h, s, p, cf, go)
    gd, hd, sd, pd, cd, god = dev
    if call == "norm":
        out, hist = F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, pd, K, N_ITER, norm, return_history=True, dilation=D)
        gg, gh, gs, gp = F.cspn2d_backward_kxk_norm_pin(gd, hd, sd, pd, god, K, N_ITER, norm, hist, dilation=D)
        grads, ref_grads, names = (gg, gh, gs, gp), [t.grad for t in leaves[:4]], ("dL/dguidance", "dL/dblur", "dL/dsparse", "dL/dpin")
    else:
        out, hist = F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
        gg, gh, gc, gs, gp = F.cspn2d_backward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, god, K, N_ITER, norm, hist, dilation=D)
        grads, names = (gg, gh, gs, gp, gc), ("dL/dguidance", "dL/dblur", "dL/dsparse", "dL/dpin", "dL/dconf")
        ref_grads = [t.grad for t in leaves]
    return dict(dev=dev, ref=ref.detach(), ref_grads=ref_grads, out=out, hist=hist, grads=grads, names=names)


def _forward(c, call, K, norm, D, **kw):
    gd, hd, sd, pd, cd, god = c["dev"]
    if call == "norm":
        return F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, pd, K, N_ITER, norm, dilation=D, **kw)
    return F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, K, N_ITER, norm, dilation=D, **kw)


def _backward(c, call, K, norm, D, history=None, **need):
    """-> (dL/dguidance, dL/dblur, dL/dsparse, dL/dpin[, dL/dconf]), the order of _case's grads"""
    gd, hd, sd, pd, cd, god = c["dev"]
    if call == "norm":
        return F.cspn2d_backward_kxk_norm_pin(gd, hd, sd, pd, god, K, N_ITER, norm, history, dilation=D, **need)
    gg, gh, gc, gs, gp = F.cspn2d_backward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, god, K, N_ITER, norm, history, dilation=D, **need)
    return gg, gh, gs, gp, gc


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,D,planes,call", CASES)
def test_forward_and_every_gradient_vs_fp64_statement(K, norm, H, W, D, planes, call):
    c = _case(K, norm, H, W, D, planes, call)
    assert bool(torch.isfinite(c["ref"]).all())
    e = rel_err(c["out"].cpu().numpy(), c["ref"].numpy())
    print("forward rel_err %.3e" % e)
    assert e <= RTOL
    assert torch.equal(_forward(c, call, K, norm, D), c["out"])   # through the ping-pong levels
    sd = c["dev"][2]
    for got, want, what in zip(c["grads"], c["ref_grads"], c["names"]):
        a, b = got.cpu().numpy().astype(np.float64), want.numpy()
        print("%s: max |engine - statement| / max |statement| = %.3e" % (what, np.abs(a - b).max() / np.abs(b).max()))
        assert _check(a, b, what)
    # where nothing is measured the confidence has no gradient: exactly zero, in the engine and in the statement; elsewhere it has one
    zero = (sd == 0).cpu()
    assert bool((c["grads"][3].cpu()[zero] == 0).all()) and bool((c["ref_grads"][3][zero] == 0).all())
    assert int((c["ref_grads"][3][~zero] != 0).sum()) >= 4 and int((c["grads"][3].cpu()[~zero] != 0).sum()) >= 4
    assert bool((c["grads"][2].cpu()[zero] == 0).all()) and bool((c["ref_grads"][2][zero] == 0).all())
    again = _backward(c, call, K, norm, D)   # without a kept history: runs its own forward
    assert all(memguard.same_bits(a, b) for a, b in zip(again, c["grads"]))
    if call == "assemble":   # the kept levels are the statement's
        gd, hd, sd, pd, cd, god = c["dev"]
        levels = pin_levels_padded(gd.cpu().double(), hd.cpu().double(), sd.cpu().double(), pd.cpu().double(), K, N_ITER, norm, D)
        hist = c["hist"].view(N_ITER, B, C, H, W).cpu()
        for t in range(1, N_ITER + 1):
            assert rel_err(hist[t - 1].numpy(), levels[t].numpy()) <= RTOL, t


# ---- bitwise anchors against the existing engine calls ----
def _anchor_inputs(K, H, W, Cc, planes, seed):
    g, h, s, p = _pin_inputs(B, Cc, H, W, K, planes, seed)
    cf = _conf(B, len(STEPS), H, W, seed + 1)
    go = torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(seed + 2))
    return g, h, s, p, cf, go


ANCHORS = [(K, H, W, D, Cc, planes) for (K, (H, W), D), (Cc, planes) in
           zip(itertools.product((3, 5, 7), ((33, 132), (17, 65)), (1, 2)), itertools.cycle(((3, "per"), (1, "shared"), (3, "shared"))))]


def test_the_anchors_run_both_dilations_on_a_vector_and_a_scalar_shape():
    assert {(a[1:4]) for a in ANCHORS} == {(33, 132, 1), (33, 132, 2), (17, 65, 1), (17, 65, 2)} and {a[0] for a in ANCHORS} == {3, 5, 7}
    assert {a[4:] for a in ANCHORS} == {(3, "per"), (1, "shared"), (3, "shared")}
    for shape in ((33, 132), (17, 65)):
        assert {a[4:] for a in ANCHORS if a[1:3] == shape} == {(3, "per"), (1, "shared"), (3, "shared")}


@pytest.mark.gpu
@pytest.mark.parametrize("K,H,W,D,Cc,planes", ANCHORS)
@pytest.mark.parametrize("norm", NORMS)
def test_unit_confidence_on_measurements_the_blur_holds_is_bitwise_the_existing_contract(K, H, W, D, Cc, planes, norm):
    """pin_conf = 1, sparse >= 0, blur = sparse where sparse > 0: b = (u cc) blur + m sparse is then (u cc + m) blur bit for bit.  out and
    dL/dguidance are the existing call's; the existing dL/dblur, A_0 + (u cc + m) db, is split into dL/dblur = A_0 + (u cc) db and dL/dsparse =
    m sum_c db_c.  With a mask plane per channel, or one channel, the two add up to it bit for bit.  With one plane shared by C = 3 channels
    dL/dsparse holds the sum over the channels: there dL/dblur is compared bit for bit where nothing is measured, and at the measured pixels
    the channel sums of both sides to float32 rounding."""
    g, h, s, p, cf, go = _anchor_inputs(K, H, W, Cc, planes, K * 10 + D)
    h, s = _anchor_one(h, s)
    gd, hd, sd, cd, god = _cuda(g, h, s, cf, go)
    one = torch.ones_like(sd)

    def compare(gb, gs, wb):
        if planes == "per" or Cc == 1:
            assert torch.equal(gb + gs, wb)
            return
        pinned = (sd > 0).expand_as(gb)
        assert torch.equal(gb[~pinned], wb[~pinned]) and bool((gs[sd == 0] == 0).all())
        # float32 roundings between the two sides, with |db_c| <= scale = max|existing dL/dblur| + max|A_0|: one per channel in the existing
        # A_0 + db (each <= 2^-24 scale), Cc - 1 in the sum dL/dsparse holds (each <= 2^-24 of a partial sum <= Cc scale): below Cc^2 2^-24 scale.
        # The sums taken here are float64
        a, b = (gb.double().sum(1, keepdim=True) + gs.double())[sd > 0], wb.double().sum(1, keepdim=True)[sd > 0]
        assert float((a - b).abs().max()) <= Cc * Cc * 2.0 ** -24 * (float(wb.abs().max()) + float(gb.abs().max()))
    out, hist = F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, one, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, N_ITER, norm, return_history=True, dilation=D)
    assert torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gs, gp = F.cspn2d_backward_kxk_norm_pin(gd, hd, sd, one, god, K, N_ITER, norm, hist, dilation=D)
    wg, wb = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, N_ITER, norm, want_hist, dilation=D)
    assert torch.equal(gg, wg)
    compare(gb, gs, wb)
    out, hist = F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, one, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    assert torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gc, gs, gp = F.cspn2d_backward_kxk_assemble_pin(gd, hd, sd, one, cd, STEPS, god, K, N_ITER, norm, hist, dilation=D)
    wg, wb, wc = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, STEPS, god, K, N_ITER, norm, want_hist, dilation=D)
    assert torch.equal(gg, wg) and torch.equal(gc, wc)
    compare(gb, gs, wb)


@pytest.mark.gpu
@pytest.mark.parametrize("K,H,W,D,Cc,planes", ANCHORS)
@pytest.mark.parametrize("norm", NORMS)
def test_zero_confidence_is_bitwise_the_call_without_a_mask(K, H, W, D, Cc, planes, norm):
    """pin_conf = 0: m = 0 and u = 1 whatever sparse holds (its negative value included).  out, dL/dblur and dL/dguidance are those of
    sparse_depth=None and dL/dsparse is all zeros.  With a mask plane per channel (C = 3) the pinned call folds the channels into the batch, as
    the existing contract does with such a mask, and the call without a mask does not: dL/dguidance is then the same sum over the channels in
    another order, compared with _check, and everything else bit for bit."""
    g, h, s, p, cf, go = _anchor_inputs(K, H, W, Cc, planes, K * 10 + D + 5)
    gd, hd, sd, cd, god = _cuda(g, h, s, cf, go)
    zero = torch.zeros_like(sd)

    def same_guidance(gg, wg):
        if planes == "per" and Cc > 1:
            return _check(gg.cpu().numpy().astype(np.float64), wg.cpu().numpy().astype(np.float64), "dL/dguidance")
        return torch.equal(gg, wg)
    out, hist = F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, zero, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_norm(gd, hd, None, K, N_ITER, norm, return_history=True, dilation=D)
    assert torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gs, gp = F.cspn2d_backward_kxk_norm_pin(gd, hd, sd, zero, god, K, N_ITER, norm, hist, dilation=D)
    wg, wb = F.cspn2d_backward_kxk_norm(gd, hd, None, god, K, N_ITER, norm, want_hist, dilation=D)
    assert same_guidance(gg, wg) and torch.equal(gb, wb) and torch.equal(gs, torch.zeros_like(gs)) and bool((gp[sd == 0] == 0).all())
    out, hist = F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, zero, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_assemble(gd, hd, None, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    assert torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gc, gs, gp = F.cspn2d_backward_kxk_assemble_pin(gd, hd, sd, zero, cd, STEPS, god, K, N_ITER, norm, hist, dilation=D)
    wg, wb, wc = F.cspn2d_backward_kxk_assemble(gd, hd, None, cd, STEPS, god, K, N_ITER, norm, want_hist, dilation=D)
    assert same_guidance(gg, wg) and torch.equal(gb, wb) and torch.equal(gc, wc) and torch.equal(gs, torch.zeros_like(gs))


# ---- 16-bit guidance ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,H,W,D,planes,norm", [(3, 33, 132, 2, "per", "8sum"), (5, 17, 65, 1, "shared", "8sum_abs"), (7, 33, 132, 1, "shared", "8sum"),
                                                 (7, 17, 65, 2, "per", "8sum_abs")])
def test_16_bit_guidance_is_bitwise_the_float32_call_on_the_widened_tensor(dtype, K, H, W, D, planes, norm):
    g, h, s, p, cf, go = _anchor_inputs(K, H, W, C, planes, K + D)
    g16, hd, sd, pd, cd, god = _cuda(g.to(dtype), h, s, p, cf, go)
    g32 = g16.float()
    out, hist = F.cspn2d_forward_kxk_norm_pin(g16, hd, sd, pd, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_norm_pin(g32, hd, sd, pd, K, N_ITER, norm, return_history=True, dilation=D)
    assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(hist, want_hist)
    got = F.cspn2d_backward_kxk_norm_pin(g16, hd, sd, pd, god, K, N_ITER, norm, hist, dilation=D)
    ref = F.cspn2d_backward_kxk_norm_pin(g32, hd, sd, pd, god, K, N_ITER, norm, want_hist, dilation=D)
    assert got[0].dtype == dtype and torch.equal(got[0], ref[0].to(dtype))   # the float32 gradient rounded once
    assert all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(got[1:], ref[1:]))
    out, hist = F.cspn2d_forward_kxk_assemble_pin(g16, hd, sd, pd, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    want, want_hist = F.cspn2d_forward_kxk_assemble_pin(g32, hd, sd, pd, cd, STEPS, K, N_ITER, norm, return_history=True, dilation=D)
    assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(hist, want_hist)
    got = F.cspn2d_backward_kxk_assemble_pin(g16, hd, sd, pd, cd, STEPS, god, K, N_ITER, norm, hist, dilation=D)
    ref = F.cspn2d_backward_kxk_assemble_pin(g32, hd, sd, pd, cd, STEPS, god, K, N_ITER, norm, want_hist, dilation=D)
    assert got[0].dtype == dtype and torch.equal(got[0], ref[0].to(dtype))
    assert all(a.dtype == torch.float32 and torch.equal(a, b) for a, b in zip(got[1:], ref[1:]))


# ---- gradient subsets ----
SUBSET_CASES = [CASES[5], CASES[6], CASES[9], CASES[21]]   # (17, 65) and (33, 132); both calls, both plane counts, both dilations


def test_the_subset_cases_cover_both_calls_planes_and_dilations():
    assert {c[6] for c in SUBSET_CASES} == {"norm", "assemble"} and {c[5] for c in SUBSET_CASES} == {"shared", "per"}
    assert {c[4] for c in SUBSET_CASES} == {1, 2} and {c[2:4] for c in SUBSET_CASES} <= {(17, 65), (33, 132)}


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,D,planes,call", SUBSET_CASES)
def test_gradient_subsets(K, norm, H, W, D, planes, call):
    c = _case(K, norm, H, W, D, planes, call)
    flags = ["need_guidance", "need_blur", "need_sparse", "need_pin"] + (["need_conf"] if call == "assemble" else [])
    for i, flag in enumerate(flags):   # every flag alone: bitwise the full call's tensor, with the kept history and (running its own forward) without
        need = {f: f == flag for f in flags}
        for history in (c["hist"], None):
            part = _backward(c, call, K, norm, D, history, **need)
            assert all((t is None) != (j == i) for j, t in enumerate(part)), flag
            assert torch.equal(part[i], c["grads"][i]), (flag, history is None)
    # all off: nothing is launched, no workspace is asked for
    names = []
    launch = F._launch
    F._launch = lambda name, *a, **k: (names.append(name), launch(name, *a, **k))[1]
    try:
        none = _backward(c, call, K, norm, D, None, **{f: False for f in flags})
    finally:
        F._launch = launch
    assert all(t is None for t in none) and names == []


# ---- repeatability, and views one element off a 16-byte boundary with W % 4 == 0: the guarded scalar kernels, the same bits ----
@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,D,planes,call", [CASES[1], CASES[8], CASES[14], CASES[23]])
def test_two_identical_calls_give_identical_bits(K, norm, H, W, D, planes, call):
    c = _case(K, norm, H, W, D, planes, call)
    out, hist = _forward(c, call, K, norm, D, return_history=True)
    grads = _backward(c, call, K, norm, D, hist)
    kept = (N_ITER if call == "assemble" else N_ITER - 1) * out.numel()
    assert memguard.same_bits(out, c["out"]) and memguard.same_bits(hist[:kept], c["hist"][:kept])
    assert all(memguard.same_bits(a, b) for a, b in zip(grads, c["grads"]))


@pytest.mark.gpu
@pytest.mark.parametrize("K,D,planes", [(3, 2, "per"), (5, 1, "shared"), (7, 2, "shared"), (7, 1, "per")])
@pytest.mark.parametrize("H,W", [(16, 64), (33, 132)])
def test_misaligned_views(K, D, planes, H, W):
    norm = "8sum"
    g, h, s, p, cf, go = _anchor_inputs(K, H, W, C, planes, K + W)

    def run(gd, hd, sd, pd, cd, god):
        out = F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, pd, K, N_ITER, norm, dilation=D)
        grads = F.cspn2d_backward_kxk_norm_pin(gd, hd, sd, pd, god, K, N_ITER, norm, dilation=D)
        aout = F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, K, N_ITER, norm, dilation=D)
        agrads = F.cspn2d_backward_kxk_assemble_pin(gd, hd, sd, pd, cd, STEPS, god, K, N_ITER, norm, dilation=D)
        return (out,) + tuple(grads) + (aout,) + tuple(agrads)
    aligned = run(*_cuda(g, h, s, p, cf, go))
    off = [_misaligned(t.cuda()) for t in (g, h, s, p, cf, go)]
    assert all(t.storage_offset() == 1 for t in off)
    memguard.assert_same_outputs(run(*off), aligned, "one element off")
    for i in range(6):   # each tensor alone off its boundary: every VEC condition on its own
        mixed = [_misaligned(t.cuda()) if j == i else t.cuda() for j, t in enumerate((g, h, s, p, cf, go))]
        memguard.assert_same_outputs(run(*mixed), aligned, "tensor %d one element off" % i)
    ref = pin_norm(g.double(), h.double(), s.double(), p.double(), K, N_ITER, norm, D)
    assert rel_err(aligned[0].cpu().numpy(), ref.numpy()) <= RTOL


# ---- memory hygiene: the four pinned calls and both modules between guard bands on NaN and on finite poison, and in a stale arena ----
def _hygiene_inputs(K, H, W, planes, dtype, seed):
    g, h, s, p, cf, go = _anchor_inputs(K, H, W, C, planes, seed)
    return tuple(_cuda(g.to(dtype), h, s, p, cf, go))


def _hygiene_call(K, norm, D):
    n = N_ITER

    def call(g, h, s, p, cf, go):
        out = F.cspn2d_forward_kxk_norm_pin(g, h, s, p, K, n, norm, dilation=D)
        out2, hist = F.cspn2d_forward_kxk_norm_pin(g, h, s, p, K, n, norm, return_history=True, dilation=D)
        grads = F.cspn2d_backward_kxk_norm_pin(g, h, s, p, go, K, n, norm, hist, dilation=D)
        alone = F.cspn2d_backward_kxk_norm_pin(g, h, s, p, go, K, n, norm, None, False, False, True, True, dilation=D)[2:]
        aout = F.cspn2d_forward_kxk_assemble_pin(g, h, s, p, cf, STEPS, K, n, norm, dilation=D)
        aout2, ahist = F.cspn2d_forward_kxk_assemble_pin(g, h, s, p, cf, STEPS, K, n, norm, return_history=True, dilation=D)
        agrads = F.cspn2d_backward_kxk_assemble_pin(g, h, s, p, cf, STEPS, go, K, n, norm, ahist, dilation=D)
        aalone = F.cspn2d_backward_kxk_assemble_pin(g, h, s, p, cf, STEPS, go, K, n, norm, None, False, True, False, True, False, dilation=D)[1::2]
        return (out, out2, hist) + tuple(grads) + tuple(alone) + (aout, aout2, ahist) + tuple(agrads) + tuple(aalone)
    return call


def _modules_inputs(H, W):
    gen = torch.Generator().manual_seed(9 + W)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in (3, 5, 7)]
    _, h, s, p = _pin_inputs(B, 2, H, W, 3, "shared", 10)
    ps = [torch.rand(B, 1, H, W, generator=gen) for _ in range(3)]
    ic = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    kc = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    go = torch.randn(B, 2, H, W, generator=gen)
    return tuple(_cuda(gs[0], gs[1].half(), gs[2], h, s, p, ps[0], ps[1], ps[2], ic, kc, go))


def _modules_call(g3, g5, g7, h, s, p, p3, p5, p7, ic, kc, go):
    """Affinity_PropagateKxK at dilation 2 feeding Affinity_PropagateAssemble at dilations (2, 2, 1), every call with its own pin_conf"""
    leaves = [hygiene._leaf(t) for t in (g3, g5, g7, h, s, p, p3, p5, p7, ic, kc)]
    first = cspn_amd.Affinity_PropagateKxK(3, 5, "8sum", dilation=2)
    second = cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), STEPS, "8sum", dilations=(2, 2, 1))
    y = second(leaves[:3], first(leaves[1], leaves[3], leaves[4], pin_conf=leaves[5]), leaves[4], [leaves[9]] * 3, leaves[10], pin_conf=leaves[6:9])
    y.backward(go)
    return (y.detach(),) + tuple(t.grad for t in leaves)


HYGIENE = {}
for _K, (_H, _W), _planes, _dt, _norm, _D in ((3, (17, 65), "per", torch.float32, "8sum", 2), (5, (33, 132), "shared", torch.bfloat16, "8sum_abs", 1),
                                             (7, (33, 132), "per", torch.float32, "8sum", 1), (7, (17, 65), "shared", torch.float16, "8sum_abs", 2)):
    _name = "kxk-pin-K%d-%dx%d-%s" % (_K, _H, _W, str(_dt).split(".")[1])
    HYGIENE[_name] = hygiene.Case(_name, tuple(NEW), "the _pin entry points at dilation %d" % _D, 4 * B * C * _H * _W,
                                  functools.lru_cache(maxsize=None)(functools.partial(_hygiene_inputs, _K, _H, _W, _planes, _dt, 60 + _K)),
                                  _hygiene_call(_K, _norm, _D), lambda: None, "test_kxk_pin.py::test_forward_and_every_gradient_vs_fp64_statement",
                                  False, None, None)
for _H, _W in ((17, 65), (33, 132)):
    _name = "kxk-pin-modules-%dx%d" % (_H, _W)
    HYGIENE[_name] = hygiene.Case(_name, ("Affinity_PropagateKxK", "Affinity_PropagateAssemble"), "the pinned module feeding the pinned assembling one",
                                  4 * B * 2 * _H * _W, functools.lru_cache(maxsize=None)(functools.partial(_modules_inputs, _H, _W)), _modules_call,
                                  lambda: None, "test_kxk_pin.py::test_penet_composition_vs_fp64_autograd", False, None, None)


def test_the_guarded_cases_stay_out_of_the_shared_table():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True}
    assert not any("pin" in n for c in hygiene.CASES.values() for n in c.covers)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_pinned_call_between_guard_bands(name, poison):
    """every output (out, the history, the five gradients: dL/dsparse and dL/dpin among them) and the workspace lie between guard bands and are
    poisoned before the call: clean outputs (bitwise the unguarded run's, so fully written), intact bands, unchanged inputs"""
    c = HYGIENE[name]
    inputs = c.build()
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, inputs, "cuda", c.plane)
    assert len(session.workspaces) >= 3 and len(session.guards) > len(session.workspaces)
    for o in outs:
        assert o is None or bool(torch.isfinite(o.float()).all()), "poison reached an output"
    memguard.assert_same_outputs(outs, hygiene._clean(c), "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    """the pinned calls of both shapes and the modules through one workspace arena that is never refilled: every result bitwise the clean one"""
    steps = []
    for name in ("kxk-pin-K7-33x132-float32", "kxk-pin-K5-33x132-bfloat16", "kxk-pin-modules-33x132", "kxk-pin-K3-17x65-float32",
                 "kxk-pin-K7-17x65-float16", "kxk-pin-modules-17x65", "kxk-pin-K7-33x132-float32"):
        c = HYGIENE[name]
        steps.append((name, c.call, c.build()))
    hygiene._run_sequence(steps, 4 * B * C * 33 * 132)


# ---- the modules against float64 autograd ----
def _grads_close(got, want, names):
    for a, b, what in zip(got, want, names):
        assert a is not None and _check(a.cpu().numpy().astype(np.float64), b.numpy(), what)


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,D,planes", [(3, "8sum", 17, 65, 1, "shared"), (5, "8sum_abs", 33, 132, 2, "per"), (7, "8sum", 17, 65, 2, "shared"),
                                                 (7, "8sum_abs", 16, 64, 1, "per")])
def test_module_kxk_vs_fp64_autograd(K, norm, H, W, D, planes):
    g, h, s, p = _pin_inputs(B, 2, H, W, K, planes, seed=K + D)
    go = torch.randn(B, 2, H, W, generator=torch.Generator().manual_seed(K))
    leaves = [t.double().requires_grad_(True) for t in (g, h, s, p)]
    ref = pin_norm(*leaves, K, N_ITER, norm, D)
    ref.backward(go.double())
    m = cspn_amd.Affinity_PropagateKxK(N_ITER, K, norm, dilation=D)
    dev = [t.cuda().requires_grad_(True) for t in (g, h, s, p)]
    y = m(dev[0], dev[1], dev[2], pin_conf=dev[3])
    assert "_CSPN2dKxKNormPinFunction" in type(y.grad_fn).__name__   # K = 3 at dilation 1 too: the K x K engine, not the ring
    y.backward(go.cuda())
    assert rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) <= RTOL
    _grads_close([t.grad for t in dev], [t.grad for t in leaves], ("guidance", "blur_depth", "sparse_depth", "pin_conf"))
    with torch.no_grad():
        assert torch.equal(m(dev[0], dev[1], dev[2], pin_conf=dev[3]), y.detach())
        assert torch.equal(y.detach(), F.cspn2d_forward_kxk_norm_pin(dev[0], dev[1], dev[2], dev[3], K, N_ITER, norm, dilation=D))
    # only the confidence is trained: the forward keeps the history for it
    pd = dev[3].detach().clone().requires_grad_(True)
    m(dev[0].detach(), dev[1].detach(), dev[2].detach(), pin_conf=pd).backward(go.cuda())
    assert torch.equal(pd.grad, dev[3].grad)
    # a float16 confidence and sparse depth are widened with a differentiable cast
    p16 = dev[3].detach().half().requires_grad_(True)
    y16 = m(dev[0].detach(), dev[1].detach(), dev[2].detach().half(), pin_conf=p16)
    y16.backward(go.cuda())
    assert y16.dtype == torch.float32 and p16.grad.dtype == torch.float16
    # pin_conf=None is today's module: today's path, today's bits
    with torch.no_grad():
        plain = m(dev[0], dev[1], dev[2])
        if K == 3 and D == 1:
            want = cspn_amd.Affinity_Propagate(N_ITER, 3, norm)(dev[0], dev[1], dev[2])
        else:
            want = F.cspn2d_forward_kxk_norm(dev[0], dev[1], dev[2], K, N_ITER, norm, dilation=D)
        assert torch.equal(plain, want) and not torch.equal(plain, y.detach())


@functools.lru_cache(maxsize=None)
def _modules_case():
    H, W, kernels, norm = 17, 65, (3, 5, 7), "8sum"
    gen = torch.Generator().manual_seed(77)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in kernels + kernels]   # the dilated pass's guidances, then the second pass's
    _, h, s, _ = _pin_inputs(B, 2, H, W, 3, "shared", 78)
    ps = [torch.rand(B, 1, H, W, generator=gen) for _ in kernels + kernels]            # a confidence per kernel size and pass
    ic = [torch.softmax(torch.randn(B, len(STEPS), H, W, generator=gen), 1) for _ in kernels + kernels]
    kc = [torch.softmax(torch.randn(B, len(kernels), H, W, generator=gen), 1) for _ in range(2)]
    go = torch.randn(B, 2, H, W, generator=gen)
    return dict(gs=gs, h=h, s=s, ps=ps, ic=ic, kc=kc, go=go, kernels=kernels, norm=norm)


def _assemble_ref(gs, h, s, ps, ic, kc, c, D):
    return sum(kc[:, k:k + 1] * pin_assemble(gs[k], h, s, ps[k], ic[k], STEPS, K, c["norm"], D) for k, K in enumerate(c["kernels"]))


@pytest.mark.gpu
def test_penet_composition_vs_fp64_autograd():
    """what a PENet port writes: Affinity_PropagateAssemble at dilation 2 feeding the same module at dilation 1, kernels (3, 5, 7), steps (0, 2, 5),
    a pin_conf per kernel size and pass, every input requiring grad (the sparse depth included: both passes pin to it)"""
    c = _modules_case()
    tensors = c["gs"] + [c["h"], c["s"]] + c["ps"] + c["ic"] + c["kc"]
    names = ["dilated guidance%d" % K for K in c["kernels"]] + ["plain guidance%d" % K for K in c["kernels"]] + ["blur_depth", "sparse_depth"] + \
        ["dilated pin_conf%d" % K for K in c["kernels"]] + ["plain pin_conf%d" % K for K in c["kernels"]] + \
        ["dilated iter_conf%d" % K for K in c["kernels"]] + ["plain iter_conf%d" % K for K in c["kernels"]] + ["dilated kernel_conf", "plain kernel_conf"]
    assert len(names) == len(tensors) == 22
    leaves = [t.double().requires_grad_(True) for t in tensors]
    mid = _assemble_ref(leaves[0:3], leaves[6], leaves[7], leaves[8:11], leaves[14:17], leaves[20], c, 2)
    ref = _assemble_ref(leaves[3:6], mid, leaves[7], leaves[11:14], leaves[17:20], leaves[21], c, 1)
    ref.backward(c["go"].double())
    dev = [t.cuda().requires_grad_(True) for t in tensors]
    dilated = cspn_amd.Affinity_PropagateAssemble(N_ITER, c["kernels"], STEPS, c["norm"], dilations=2)
    plain = cspn_amd.Affinity_PropagateAssemble(N_ITER, c["kernels"], STEPS, c["norm"])
    mid_d = dilated(dev[0:3], dev[6], dev[7], dev[14:17], dev[20], pin_conf=dev[8:11])
    y = plain(dev[3:6], mid_d, dev[7], dev[17:20], dev[21], pin_conf=dev[11:14])
    y.backward(c["go"].cuda())
    assert bool(torch.isfinite(ref).all()) and rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) <= RTOL
    _grads_close([t.grad for t in dev], [t.grad for t in leaves], names)
    with torch.no_grad():
        # one tensor for all kernel sizes is the sequence that repeats it
        one = plain(dev[3:6], dev[6], dev[7], dev[17:20], dev[21], pin_conf=dev[11])
        assert torch.equal(one, plain(dev[3:6], dev[6], dev[7], dev[17:20], dev[21], pin_conf=[dev[11]] * 3))
        # pin_conf=None is today's module output: today's Function, today's bits
        today = sum(F.cspn2d_forward_kxk_assemble(dev[3 + k], dev[6], dev[7], dev[17 + k] * dev[21][:, k:k + 1], STEPS, K, N_ITER, c["norm"])
                    for k, K in enumerate(c["kernels"]))
        assert torch.equal(plain(dev[3:6], dev[6], dev[7], dev[17:20], dev[21]), today) and not torch.equal(one, today)
    nodes = repr(plain(dev[3:6], dev[6], dev[7], dev[17:20], dev[21]).grad_fn.next_functions)
    assert "_CSPN2dKxKAssembleFunction" in nodes and "Pin" not in nodes


# ---- the NaN rule ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("D", [1, 2])
def test_a_pixel_without_neighbours_is_nan(K, D):
    """on a 1 x 1 image every neighbour lies outside: S = 0 and wb = 0 / 0, in the engine and in both statements alike (the forward only)"""
    g = torch.randn(B, K * K - 1, 1, 1, generator=torch.Generator().manual_seed(K))
    h = torch.full((B, C, 1, 1), 2.0)
    s = torch.tensor([1.5, 0.0]).view(B, 1, 1, 1)
    p = torch.full((B, 1, 1, 1), 0.25)
    cf = torch.ones(B, 2, 1, 1)
    for norm in NORMS:
        for levels in (pin_levels_padded, pin_levels_folded):
            assert bool(torch.isnan(pin_norm(g.double(), h.double(), s.double(), p.double(), K, 2, norm, D, levels)).all())
        gd, hd, sd, pd, cd = _cuda(g, h, s, p, cf)
        assert bool(torch.isnan(F.cspn2d_forward_kxk_norm_pin(gd, hd, sd, pd, K, 2, norm, dilation=D)).all())
        assert bool(torch.isnan(F.cspn2d_forward_kxk_assemble_pin(gd, hd, sd, pd, cd, (1, 2), K, 2, norm, dilation=D)).all())
