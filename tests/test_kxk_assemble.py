"""Assembling K x K propagation levels per pixel (CSPN++): out = sum_j conf_j H_{s_j} over the levels H_t of the depth-completion contract
(cspn2d_forward_kxk_norm, H_0 = blur_depth), collected iterations s_0 < .. < s_{T-1} = n, conf [B,T,H,W] shared by the C channels;
cspn2d_forward_kxk_assemble / cspn2d_backward_kxk_assemble and the module Affinity_PropagateAssemble.
CPU: the float64 statement is tests/test_kxk_norm.py's torch_kxk_norm unrolled so that it keeps every level (each level is checked to be that
     statement's result, exactly); symbols, byte counts, the C and the Python argument errors, the module's constructor.
GPU: forward and the three gradients against the statement and its float64 autograd, at the bounds tests/test_kxk_norm.py uses (RTOL; _check);
     bitwise anchors to the existing engine (T = 1 and conf = 1 is cspn2d_forward_kxk_norm / cspn2d_backward_kxk_norm; 16-bit guidance is the
     float32 call on the widened tensor); every entry point between guard bands on poisoned buffers (tests/memguard.py); the module.
Shapes around the 64 x 16 tile: W = 67 (guarded scalar kernels, both tile seams), W = 68 (16-byte kernels, the seam at column 64), and W = 68
at a misaligned address (scalar kernels on a width the vector kernels would take).

The memory-hygiene cases of the new calls are entered into the table of tests/test_memory_hygiene.py (its case()), which requires one for every
public name, and run from here under its helpers."""
import contextlib
import ctypes
import functools
import os
import re

import pytest
import torch

import cspn_amd
import memguard
import test_memory_hygiene as hygiene
from cspn_amd import _lib
from cspn_amd import functional as F
from helpers import rel_err
from test_backward import _check
from test_kxk_norm import RTOL, _cuda, _inputs, _misaligned, _pads, torch_kxk_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_kxk_assemble_workspace_bytes", "cspn2d_kxk_assemble_history_bytes", "cspn2d_backward_kxk_assemble_workspace_bytes",
       "cspn2d_forward_kxk_assemble_f32", "cspn2d_forward_kxk_assemble_g16", "cspn2d_backward_kxk_assemble_f32", "cspn2d_backward_kxk_assemble_g16"]
N_ITER = 5


# ---- the float64 statement: torch_kxk_norm (tests/test_kxk_norm.py) unrolled ----
def torch_kxk_levels(guidance, blur, sparse, K, n, norm):
    """torch_kxk_norm's loop, statement for statement, keeping every level -> [H_0 .. H_n]"""
    R = K // 2
    P = _pads(K)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, R:-R, R:-R]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    levels = [x]
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, R:-R, R:-R]
        if m is not None:
            x = (1 - m) * x + m * blur
        levels.append(x)
    return levels


def torch_kxk_assemble(guidance, blur, sparse, conf, steps, K, norm):
    levels = torch_kxk_levels(guidance, blur, sparse, K, steps[-1], norm)
    out = conf[:, 0:1] * levels[steps[0]]
    for j in range(1, len(steps)):
        out = out + conf[:, j:j + 1] * levels[steps[j]]
    return out


def _conf(B, T, H, W, seed):
    """positive and deliberately not normalised: a dropped or doubled level shows"""
    return torch.rand(B, T, H, W, generator=torch.Generator().manual_seed(seed))


# ---- CPU ----
def test_unrolled_statement_keeps_the_levels_of_torch_kxk_norm():
    for K, norm, sparse in ((3, "8sum", "shared"), (5, "8sum_abs", None), (7, "8sum", "per")):
        g, h, s = (t.double() if t is not None else None for t in _inputs(2, 2, 9, 11, K, sparse, seed=K))
        levels = torch_kxk_levels(g, h, s, K, 4, norm)
        assert len(levels) == 5 and levels[0] is h
        for t in range(5):
            assert torch.equal(levels[t], torch_kxk_norm(g, h, s, K, t, norm)), (K, t)
        conf = _conf(2, 3, 9, 11, 1).double()
        want = conf[:, 0:1] * levels[0] + conf[:, 1:2] * levels[2] + conf[:, 2:3] * levels[4]
        assert torch.equal(torch_kxk_assemble(g, h, s, conf, (0, 2, 4), K, norm), want)


def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert {"cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble", "Affinity_PropagateAssemble"} <= set(cspn_amd.__all__)
    for n in ("cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble", "Affinity_PropagateAssemble"):
        assert callable(getattr(cspn_amd, n))


def test_byte_counts():
    wsb = _lib.late_symbol("cspn2d_kxk_assemble_workspace_bytes")
    hb = _lib.late_symbol("cspn2d_kxk_assemble_history_bytes")
    bwb = _lib.late_symbol("cspn2d_backward_kxk_assemble_workspace_bytes")
    norm_bwb = _lib.late_symbol("cspn2d_backward_kxk_norm_workspace_bytes")
    B, C, H, W = 2, 3, 10, 13
    L = B * C * H * W
    for n in (1, 2, 4, 24):
        assert hb(B, C, H, W, 5, n) == 4 * n * L    # H_1 .. H_n: H_n is not the output
    assert hb(B, C, H, W, 5, 0) == 0 and hb(B, C, H, W, 9, 4) == 0 and hb(0, C, H, W, 5, 4) == 0 and hb(B, C, H, -1, 5, 4) == 0
    for K in (3, 5, 7):
        fold = 4 * (B * (K * K - 1) * H * W + L)
        assert wsb(B, C, 0, H, W, K, 1) >= fold and wsb(B, C, 1, H, W, K, 4) >= fold + 2 * 4 * L
        assert wsb(B, C, C, H, W, K, 1) >= 4 * (B * C * (K * K - 1) * H * W + L)
        for sc in (0, 1, C):
            for n in (1, 2, 5):
                assert bwb(B, C, sc, H, W, K, n) >= norm_bwb(B, C, sc, H, W, K, n) + 4 * L
                assert bwb(B, C, sc, H, W, K, n) % 256 == 0
    for f in (wsb, bwb):
        assert f(B, C, 0, H, W, 5, 0) == 0 and f(B, C, 0, H, W, 9, 4) == 0 and f(0, C, 0, H, W, 5, 4) == 0 and f(B, C, 2, H, W, 5, 4) == 0
        assert f(1 << 12, 1 << 8, 0, 1 << 6, 1 << 6, 5, 3) == 0   # 2^32 elements


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    fwd = _lib.late_symbol("cspn2d_forward_kxk_assemble_f32")
    bwd = _lib.late_symbol("cspn2d_backward_kxk_assemble_f32")
    f16 = _lib.late_symbol("cspn2d_forward_kxk_assemble_g16")
    b16 = _lib.late_symbol("cspn2d_backward_kxk_assemble_g16")
    g, x, s, cf, o, h, w, gg, gx, gc, go = (ctypes.c_void_p(i << 32) for i in range(1, 12))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    st = _ints(1, 3)
    # forward: (guidance, blur, sparse, conf, steps, T, out, history, history_bytes, B, C, sparse_C, H, W, K, n_iter, norm, ws, ws_bytes, stream)
    def f(guidance=g, blur=x, sparse=None, conf=cf, steps=st, T=2, out=o, hist=None, hbytes=0, B=2, C=1, sc=0, H=8, W=8, K=5, n=3, norm=0, ws=w,
          wsb=M, call=fwd, pre=()):
        return call(guidance, *pre, blur, sparse, conf, steps, T, out, hist, hbytes, B, C, sc, H, W, K, n, norm, ws, wsb, None)
    for name in ("guidance", "blur", "conf", "steps", "out"):
        assert f(**{name: None}) == -1 and name.encode() in err() and b"NULL" in err(), name
    for K in (1, 2, 4, 9, 0):
        assert f(K=K) == -1 and b"K must be" in err()
    for norm in (2, 3, -1):
        assert f(norm=norm) == -1 and b"norm" in err()
    assert f(sparse=s, sc=0) == -1 and b"sparse_C" in err()
    assert f(C=3, sc=2, sparse=s) == -1 and b"sparse_C" in err()
    for shape in (dict(B=0), dict(C=0), dict(H=0), dict(W=-2)):
        assert f(**shape) == -1 and b"bad shape" in err()
    for n in (0, -1):
        assert f(n=n, steps=_ints(0), T=1) == -1 and b"n_iter" in err()
    for T in (0, -1, 5):   # 1 <= T <= n_iter + 1 = 4
        assert f(T=T, steps=_ints(0, 1, 2, 3, 4)) == -1 and b"T must be" in err()
    for bad in ((3, 3), (2, 1), (-1, 3), (0, 0)):
        assert f(steps=_ints(*bad)) == -1 and b"steps" in err(), bad
    assert f(steps=_ints(0, 1, 1, 3), T=4) == -1 and b"strictly increasing" in err()
    for bad in ((1, 2), (0, 4)):
        assert f(steps=_ints(*bad)) == -1 and b"steps[T-1]" in err(), bad
    assert f(steps=_ints(0, 1, 2, 3), T=4, wsb=100) == -2     # T = n_iter + 1 is allowed: the next check is reached
    # views of 2^31 elements or more
    assert f(B=1 << 12, C=1 << 8, H=1 << 6, W=1 << 6) == -1 and b"blur" in err()
    assert f(B=1 << 8, H=1 << 10, W=1 << 8, K=7) == -1 and b"guidance" in err()
    assert f(B=1 << 8, C=4, sc=4, sparse=s, H=1 << 10, W=1 << 8, K=3) == -1 and b"guidance" in err()
    assert f(B=1 << 7, H=1 << 10, W=1 << 10, K=3, n=24, T=16, steps=_ints(*range(9, 25))) == -1 and b"conf" in err()   # 16 planes against the guidance's 8
    # out aliasing an input, the history or the workspace on an input
    for name, ptr in (("blur", x), ("conf", cf), ("guidance", ctypes.c_void_p(g.value + 64))):
        assert f(out=ptr) == -1 and b"alias" in err(), name
    assert f(sparse=s, sc=1, out=s) == -1 and b"alias" in err()
    assert f(hist=cf, hbytes=M) == -1 and b"alias" in err()
    assert f(ws=ctypes.c_void_p(cf.value + 256)) == -1 and b"alias" in err()
    # workspace and history
    assert f(ws=None, wsb=0) == -2 and b"workspace" in err()
    assert f(wsb=100) == -2 and b"workspace" in err()
    assert f(hist=h, hbytes=M, wsb=100) == -2                                  # with a history the fold still needs room
    assert f(ws=ctypes.c_void_p(w.value + 4)) == -2 and b"aligned" in err()
    assert f(hist=h, hbytes=4 * 2 * 8 * 8 * 3 - 4) == -2 and b"history" in err()   # n levels, not n - 1
    # the 16-bit form: the same checks, the dtype and the alignment of the 16-bit tensor
    assert f(call=f16, pre=(1,), conf=None) == -1 and b"conf" in err()
    assert f(call=f16, pre=(3,)) == -1 and b"dtype" in err()
    assert f(call=f16, pre=(2,), guidance=ctypes.c_void_p(g.value + 1)) == -1 and b"aligned" in err()
    assert f(call=f16, pre=(2,), steps=_ints(2, 2)) == -1 and b"steps" in err()
    # backward: (guidance, blur, sparse, conf, steps, T, history, history_bytes, grad_out, grad_guidance, grad_blur, grad_conf, B, C, sparse_C, H, W,
    #            K, n_iter, norm, ws, ws_bytes, stream)
    hb = 4 * 2 * 8 * 8 * 3

    def b(guidance=g, blur=x, sparse=None, conf=cf, steps=st, T=2, hist=h, hbytes=hb, grad_out=go, gg=gg, gx=gx, gc=gc, B=2, C=1, sc=0, H=8, W=8, K=5,
          n=3, norm=0, ws=w, wsb=M, call=bwd, pre=()):
        return call(guidance, *pre, blur, sparse, conf, steps, T, hist, hbytes, grad_out, gg, gx, gc, B, C, sc, H, W, K, n, norm, ws, wsb, None)
    for name in ("guidance", "blur", "conf", "steps", "grad_out"):
        assert b(**{name: None}) == -1 and name.encode() in err() and b"NULL" in err(), name
    assert b(K=9) == -1 and b"K must be" in err()
    assert b(norm=2) == -1 and b"norm" in err()
    assert b(C=2, sc=2, sparse=None) == -1 and b"sparse_C" in err()
    assert b(T=5, steps=_ints(0, 1, 2, 3, 4)) == -1 and b"T must be" in err()
    assert b(steps=_ints(3, 1)) == -1 and b"steps" in err()
    assert b(steps=_ints(1, 2)) == -1 and b"steps[T-1]" in err()
    assert b(B=1 << 12, C=1 << 8, H=1 << 6, W=1 << 6) == -1 and b"blur" in err()
    assert b(hist=None, hbytes=0) == -1 and b"history" in err()
    assert b(hbytes=hb - 4) == -1 and b"history" in err()
    assert b(hist=None, hbytes=0, gg=None) == -1 and b"history" in err()          # grad_conf alone needs it
    assert b(hist=None, hbytes=0, gg=None, gc=None, wsb=64) == -2                  # grad_blur alone does not: the next check is reached
    for kw in (dict(gg=x), dict(gx=x), dict(gc=x), dict(gc=cf), dict(gx=go), dict(gg=h), dict(gc=h), dict(gx=cf), dict(gg=gx), dict(gx=gc), dict(gg=gc),
               dict(gc=ctypes.c_void_p(g.value + 64)), dict(ws=ctypes.c_void_p(go.value + 256)), dict(ws=ctypes.c_void_p(gc.value))):
        assert b(**kw) == -1 and b"alias" in err(), kw
    assert b(sparse=s, sc=1, gx=s) == -1 and b"alias" in err()
    assert b(ws=None, wsb=0) == -2 and b"workspace" in err()
    assert b(wsb=64) == -2
    assert b(ws=ctypes.c_void_p(w.value + 128)) == -2 and b"aligned" in err()
    assert b(call=b16, pre=(7,)) == -1 and b"dtype" in err()
    assert b(call=b16, pre=(1,), gg=ctypes.c_void_p(gg.value + 1)) == -1 and b"aligned" in err()
    assert b(call=b16, pre=(1,), grad_out=None) == -1 and b"grad_out" in err()
    assert b(gg=None, gx=None, gc=None, hist=None, hbytes=0) == 0                  # nothing asked for: nothing is enqueued


def test_python_argument_errors_without_gpu():
    g5, h, s = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9)
    cf = torch.rand(1, 2, 6, 9)
    f, b = F.cspn2d_forward_kxk_assemble, F.cspn2d_backward_kxk_assemble
    for steps in ((), (3, 3), (2, 1, 3), (-1, 3), (1, 2), (0, 4), (1.0, 3), (True, 3), 3, None, (1, 2, 3)):
        with pytest.raises(ValueError, match="steps|conf"):
            f(g5, h, s, cf, steps, 5, 3)
    with pytest.raises(ValueError, match="steps"):
        b(g5, h, s, cf, (3, 1), torch.rand(1, 2, 6, 9), 5, 3)
    with pytest.raises(ValueError, match="n_iter"):
        f(g5, h, s, cf[:, :1], (0,), 5, 0)
    for bad in (torch.rand(1, 3, 6, 9), torch.rand(1, 2, 6, 8), torch.rand(2, 2, 6, 9), torch.rand(2, 6, 9)):
        with pytest.raises(ValueError, match="conf"):
            f(g5, h, s, bad, (1, 3), 5, 3)
        with pytest.raises(ValueError, match="conf"):
            b(g5, h, s, bad, (1, 3), torch.rand(1, 2, 6, 9), 5, 3)
    for ks in (4, 9, True):
        with pytest.raises(ValueError, match="kernel_size"):
            f(g5, h, s, cf, (1, 3), ks, 3)
    with pytest.raises(ValueError, match="norm_type"):
        f(g5, h, s, cf, (1, 3), 5, 3, "none")
    with pytest.raises(ValueError, match="guidance"):
        f(torch.rand(1, 8, 6, 9), h, s, cf, (1, 3), 5, 3)
    with pytest.raises(ValueError, match="sparse_depth"):
        f(g5, h, torch.rand(1, 3, 6, 9), cf, (1, 3), 5, 3)
    with pytest.raises(ValueError, match="grad_out"):
        b(g5, h, s, cf, (1, 3), torch.rand(1, 1, 6, 9), 5, 3)
    for name in ("guidance", "blur", "sparse", "conf"):   # tensors on different devices
        args = dict(guidance=g5, blur=h, sparse=s, conf=cf)
        args[name] = args[name].to("meta")
        with pytest.raises(ValueError, match="same device"):
            f(args["guidance"], args["blur"], args["sparse"], args["conf"], (1, 3), 5, 3)
    with pytest.raises(ValueError, match="same device"):
        b(g5, h, s, cf, (1, 3), torch.rand(1, 2, 6, 9, device="meta"), 5, 3)
    for args in ((g5.numpy(), h, s, cf), (g5, h.numpy(), s, cf), (g5, h, s, cf.numpy()), (g5, h, s, None)):
        with pytest.raises(TypeError):
            f(*args, (1, 3), 5, 3)
    with pytest.raises(TypeError):
        b(g5, h, s, cf.numpy(), (1, 3), torch.rand(1, 2, 6, 9), 5, 3)
    # well-formed, but on the CPU: the engine is GPU-only and has no CPU path
    with pytest.raises(cspn_amd.CspnError):
        f(g5, h, s, cf, (1, 3), 5, 3)
    with pytest.raises(cspn_amd.CspnError):
        b(g5, h, s, cf, (1, 3), torch.rand(1, 2, 6, 9), 5, 3)
    with pytest.raises(cspn_amd.CspnError):
        cspn_amd.Affinity_PropagateAssemble(3, (5,), (1, 3))([g5], h, s, [cf])


def test_module_constructor_and_identity():
    m = cspn_amd.Affinity_PropagateAssemble(24)
    assert (m.prop_time, m.prop_kernels, m.steps, m.norm_type) == (24, (3, 5, 7), (24,), "8sum")
    m = cspn_amd.Affinity_PropagateAssemble(24, [5, 7], [6, 12, 18, 24], "8sum_abs")
    assert (m.prop_kernels, m.steps, m.norm_type) == ((5, 7), (6, 12, 18, 24), "8sum_abs")
    assert "prop_time=24" in m.extra_repr() and "(5, 7)" in m.extra_repr() and "(6, 12, 18, 24)" in m.extra_repr() and "8sum_abs" in repr(m)
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}
    for bad in ((), (4,), (3, 9), (5, 1)):
        with pytest.raises(AssertionError):
            cspn_amd.Affinity_PropagateAssemble(24, bad)
    for bad in ((), (6, 6, 24), (12, 6, 24), (6, 12), (-1, 24), (6.0, 24), (25,)):
        with pytest.raises(AssertionError):
            cspn_amd.Affinity_PropagateAssemble(24, (5,), bad)
    for nt in ("none", "abs", "8SUM"):
        with pytest.raises(AssertionError):
            cspn_amd.Affinity_PropagateAssemble(24, (5,), None, nt)
    g5, g7, h = torch.rand(1, 24, 6, 9), torch.rand(1, 48, 6, 9), torch.rand(1, 2, 6, 9)
    assert m([g5, g7], h, n_iter=0) is h                                      # n_iter == 0: the very same tensor
    assert cspn_amd.Affinity_PropagateAssemble(0, (5, 7))([g5, g7], h) is h
    with pytest.raises(ValueError, match="one entry per kernel size"):
        m([g5], h)
    with pytest.raises(ValueError, match="one entry per kernel size"):
        m([g5, g7], h, None, [torch.rand(1, 4, 6, 9)])
    with pytest.raises(ValueError, match="kernel_conf"):
        m([g5, g7], h, None, None, torch.rand(1, 3, 6, 9))


# ---- GPU ----
# every K with every steps, and across the rows: W = 67 / 68 / 68 misaligned, C 1 / 3, no mask / one mask / a mask per channel, both norms
_ROWS = [((5,), "w67", 1, None, "8sum"), ((0, 2, 5), "w68", 3, "shared", "8sum_abs"), ((1, 2, 3, 4, 5), "mis", 3, "per", "8sum"),
         ((5,), "w68", 3, "per", "8sum_abs"), ((0, 2, 5), "mis", 3, None, "8sum"), ((1, 2, 3, 4, 5), "w67", 1, "shared", "8sum_abs")]
_SHAPES = ["w67", "w68", "mis"]
CASES = [(K, steps, _SHAPES[(_SHAPES.index(shape) + i) % 3], C, sparse, norm)
         for i, K in enumerate((3, 5, 7)) for steps, shape, C, sparse, norm in _ROWS]
# beyond the issue's list: level 0 and level 1 collected by the same step; a single step (no adjoint level, no ping-pong level)
EDGES = [(5, (0, 1, 5), "w67", 3, "per", "8sum", 5), (7, (0, 1), "w68", 1, "shared", "8sum_abs", 1), (3, (1,), "mis", 3, None, "8sum", 1),
         (5, (0, 1, 2), "w68", 1, None, "8sum", 2)]


def _place(shape, *ts):
    return [None if t is None else (_misaligned(t.cuda()) if shape == "mis" else t.cuda()) for t in ts]


@functools.lru_cache(maxsize=None)
def _case(K, steps, shape, C, sparse, norm, n=N_ITER):
    """the inputs, the float64 statement with its autograd gradients, and the engine's results: made once, shared by the tests below, never written"""
    B, H, W = 2, 19, 67 if shape == "w67" else 68
    seed = K * 100 + len(steps) * 10 + C + W
    g, h, s = _inputs(B, C, H, W, K, sparse, seed)
    cf = _conf(B, len(steps), H, W, seed + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2))
    gt, ht, ct = (t.double().requires_grad_(True) for t in (g, h, cf))
    ref = torch_kxk_assemble(gt, ht, s.double() if s is not None else None, ct, steps, K, norm)
    ref.backward(go.double())
    dev = _place(shape, g, h, s, cf, go)
    gd, hd, sd, cd, god = dev
    out, hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, n, norm, return_history=True)
    grads = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, n, norm, hist)
    return dict(dev=dev, ref=ref.detach(), ref_grads=(gt.grad, ht.grad, ct.grad), out=out, hist=hist, grads=grads)


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm", CASES)
def test_forward_vs_fp64_statement(K, steps, shape, C, sparse, norm):
    c = _case(K, steps, shape, C, sparse, norm)
    assert bool(torch.isfinite(c["ref"]).all())   # these inputs give no zero abs-sum
    e = rel_err(c["out"].cpu().numpy(), c["ref"].numpy())
    print("forward rel_err %.3e" % e)
    assert e <= RTOL
    gd, hd, sd, cd, _ = c["dev"]
    assert torch.equal(F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, N_ITER, norm), c["out"])   # through the ping-pong levels: the same bits
    # the history is H_1 .. H_n
    B, _, H, W = hd.shape
    levels = torch_kxk_levels(gd.cpu().double(), hd.cpu().double(), sd.cpu().double() if sd is not None else None, K, N_ITER, norm)
    hist = c["hist"].view(N_ITER, B, C, H, W).cpu()
    for t in range(1, N_ITER + 1):
        assert rel_err(hist[t - 1].numpy(), levels[t].numpy()) <= RTOL, t


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm", CASES)
def test_three_gradients_vs_fp64_autograd(K, steps, shape, C, sparse, norm):
    c = _case(K, steps, shape, C, sparse, norm)
    for got, want, what in zip(c["grads"], c["ref_grads"], ("dL/dguidance", "dL/dblur", "dL/dconf")):
        assert _check(got.cpu().numpy(), want.numpy(), what)
    gd, hd, sd, cd, god = c["dev"]
    # without a passed-in history: the same bits
    again = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm)
    assert all(torch.equal(a, b) for a, b in zip(again, c["grads"]))
    # each need_* flag off in turn: None there, the others unchanged bit for bit
    for off in range(3):
        need = [i != off for i in range(3)]
        part = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, c["hist"] if off != 1 else None, *need)
        for i in range(3):
            assert (part[i] is None) if i == off else torch.equal(part[i], c["grads"][i]), (off, i)
    assert F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, None, False, False, False) == (None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm,n", EDGES)
def test_edge_steps_vs_fp64_statement(K, steps, shape, C, sparse, norm, n):
    c = _case(K, steps, shape, C, sparse, norm, n)
    assert bool(torch.isfinite(c["ref"]).all())
    assert rel_err(c["out"].cpu().numpy(), c["ref"].numpy()) <= RTOL
    for got, want, what in zip(c["grads"], c["ref_grads"], ("dL/dguidance", "dL/dblur", "dL/dconf")):
        assert _check(got.cpu().numpy(), want.numpy(), what)
    gd, hd, sd, cd, god = c["dev"]
    only_blur = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, n, norm, None, False, True, False)
    assert only_blur[0] is None and only_blur[2] is None and torch.equal(only_blur[1], c["grads"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape,C,sparse,norm", [("w67", 3, "per", "8sum"), ("w68", 1, "shared", "8sum_abs"), ("mis", 3, None, "8sum")])
def test_one_step_and_unit_confidence_is_bitwise_the_norm_engine(K, shape, C, sparse, norm):
    B, H, W, n = 2, 19, 67 if shape == "w67" else 68, N_ITER
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K + W)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3))
    gd, hd, sd, god = _place(shape, g, h, s, go)
    ones = torch.ones(B, 1, H, W, device="cuda")
    out, hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, ones, (n,), K, n, norm, return_history=True)
    want, want_hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True)
    assert torch.equal(out, want) and torch.equal(F.cspn2d_forward_kxk_assemble(gd, hd, sd, ones, (n,), K, n, norm), want)
    L = out.numel()
    assert torch.equal(hist[:(n - 1) * L], want_hist[:(n - 1) * L]) and torch.equal(hist[(n - 1) * L:n * L].view_as(out), want)
    gg, gb, gc = F.cspn2d_backward_kxk_assemble(gd, hd, sd, ones, (n,), god, K, n, norm, hist)
    wg, wb = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, want_hist)
    assert torch.equal(gg, wg) and torch.equal(gb, wb)
    assert _check(gc.cpu().numpy(), (go.double() * want.cpu().double()).sum(1, keepdim=True).numpy(), "dL/dconf")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm", [(3, (0, 2, 5), "w68", 3, "per", "8sum"), (5, (1, 2, 3, 4, 5), "w67", 1, "shared", "8sum_abs"),
                                                        (7, (0, 2, 5), "mis", 3, None, "8sum"), (7, (5,), "w68", 3, "shared", "8sum_abs")])
def test_16_bit_guidance_is_bitwise_the_float32_call_on_the_widened_tensor(dtype, K, steps, shape, C, sparse, norm):
    B, H, W, n = 2, 19, 67 if shape == "w67" else 68, N_ITER
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K)
    cf = _conf(B, len(steps), H, W, K + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(K + 2))
    g16, hd, sd, cd, god = _place("w", g.to(dtype), h, s, cf, go)
    if shape == "mis":   # a 16-bit view at an address that is no multiple of 8
        buf = torch.empty(g16.numel() + 1, dtype=dtype, device="cuda")
        buf[1:].view(g16.shape).copy_(g16)
        g16 = buf[1:].view(g16.shape)
        assert g16.data_ptr() % 8 != 0
    g32 = g16.float()
    out, hist = F.cspn2d_forward_kxk_assemble(g16, hd, sd, cd, steps, K, n, norm, return_history=True)
    want, want_hist = F.cspn2d_forward_kxk_assemble(g32, hd, sd, cd, steps, K, n, norm, return_history=True)
    assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gc = F.cspn2d_backward_kxk_assemble(g16, hd, sd, cd, steps, god, K, n, norm, hist)
    wg, wb, wc = F.cspn2d_backward_kxk_assemble(g32, hd, sd, cd, steps, god, K, n, norm, want_hist)
    assert gg.dtype == dtype and torch.equal(gg, wg.to(dtype)) and torch.equal(gb, wb) and torch.equal(gc, wc)
    # a 16-bit conf, blur_depth or sparse_depth is widened with one cast
    out16 = F.cspn2d_forward_kxk_assemble(g16, hd.to(dtype), sd.to(dtype) if sd is not None else None, cd.to(dtype), steps, K, n, norm)
    assert torch.equal(out16, F.cspn2d_forward_kxk_assemble(g16, hd.to(dtype).float(), sd.to(dtype).float() if sd is not None else None,
                                                            cd.to(dtype).float(), steps, K, n, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm", [CASES[1], CASES[8], CASES[16]])
def test_two_identical_calls_give_identical_bits(K, steps, shape, C, sparse, norm):
    c = _case(K, steps, shape, C, sparse, norm)
    gd, hd, sd, cd, god = c["dev"]
    out, hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, N_ITER, norm, return_history=True)
    grads = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, hist)
    assert torch.equal(out, c["out"]) and torch.equal(hist, c["hist"])
    assert all(torch.equal(a, b) for a, b in zip(grads, c["grads"]))


# ---- memory hygiene: every new entry point between guard bands, on NaN and on finite poison (tests/memguard.py) ----
def _hygiene_inputs(K, steps, W, C, sparse, dtype, seed):
    B, H = 2, 19
    g, h, s = _inputs(B, C, H, W, K, sparse, seed)
    cf = _conf(B, len(steps), H, W, seed + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2))
    return tuple(_cuda(g.to(dtype), h, s, cf, go))


def _hygiene_call(K, steps, norm):
    n = steps[-1]

    def call(g, h, s, cf, go):
        out = F.cspn2d_forward_kxk_assemble(g, h, s, cf, steps, K, n, norm)
        out2, hist = F.cspn2d_forward_kxk_assemble(g, h, s, cf, steps, K, n, norm, return_history=True)
        gg, gb, gc = F.cspn2d_backward_kxk_assemble(g, h, s, cf, steps, go, K, n, norm, hist)
        alone = F.cspn2d_backward_kxk_assemble(g, h, s, cf, steps, go, K, n, norm, None, False, True, False)[1]   # (no history, no fold's adjoint)
        return out, out2, hist, gg, gb, gc, alone
    return call


def _module_call(kernels, steps, norm):
    def call(g3, g5, g7, h, s, ic, kc, go):
        leaves = [hygiene._leaf(t) for t in (g3, g5, g7, h, ic, kc)]
        m = cspn_amd.Affinity_PropagateAssemble(steps[-1], kernels, steps, norm)
        y = m(leaves[:3], leaves[3], s, [leaves[4]] * 3, leaves[5])
        assert type(y.grad_fn).__name__ == "AddBackward0" and "_CSPN2dKxKAssembleFunction" in type(y.grad_fn.next_functions[1][0]).__name__
        y.backward(go)
        return (y.detach(),) + tuple(t.grad for t in leaves)
    return call


def _module_inputs():
    B, C, H, W = 2, 2, 19, 68
    gen = torch.Generator().manual_seed(9)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in (3, 5, 7)]
    _, h, s = _inputs(B, C, H, W, 3, "shared", 10)
    ic = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    kc = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    go = torch.randn(B, C, H, W, generator=gen)
    return tuple(_cuda(gs[0], gs[1].half(), gs[2], h, s, ic, kc, go))


_PINNED = "test_kxk_assemble.py::test_forward_vs_fp64_statement, ::test_three_gradients_vs_fp64_autograd"
for _K, _steps, _W, _C, _sparse, _dt, _norm in ((3, (0, 2, 5), 67, 3, "per", torch.float32, "8sum"), (5, (1, 2, 3, 4, 5), 68, 1, "shared", torch.bfloat16, "8sum_abs"),
                                               (7, (0, 2, 5), 68, 3, None, torch.float32, "8sum"), (7, (5,), 67, 3, "shared", torch.float16, "8sum_abs")):
    hygiene.case("kxk-assemble-K%d-W%d-T%d-%s" % (_K, _W, len(_steps), str(_dt).split(".")[1]), ("cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble"),
                 "inferred from the width, not asserted: %s kernels; forward through the ping-pong levels, forward into the history H_1 .. H_n, backward from it, "
                 "dL/dblur alone" % ("vector" if _W % 4 == 0 else "guarded scalar"),
                 4 * 2 * _C * 19 * _W, functools.partial(_hygiene_inputs, _K, _steps, _W, _C, _sparse, _dt, 40 + _K), _hygiene_call(_K, _steps, _norm),
                 lambda: None, _PINNED)
hygiene.case("module-Affinity_PropagateAssemble", "Affinity_PropagateAssemble",
             "one _CSPN2dKxKAssembleFunction per kernel size under the sum (asserted on the output's graph), kernel_conf multiplied into iter_conf by torch",
             4 * 2 * 2 * 19 * 68, _module_inputs, _module_call((3, 5, 7), (0, 2, 5), "8sum"), lambda: None, "test_kxk_assemble.py::test_module_vs_fp64_autograd")
HYGIENE = [n for n in hygiene.CASES if n.startswith("kxk-assemble-") or n == "module-Affinity_PropagateAssemble"]


def test_the_hygiene_table_covers_the_new_names():
    covered = {n for name in HYGIENE for n in hygiene.CASES[name].covers}
    assert covered == {"cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble", "Affinity_PropagateAssemble"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", HYGIENE)
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_entry_point_between_guard_bands(name, poison):
    """out, the workspace and the history lie between guard bands and are poisoned before the call: clean outputs (bitwise the unguarded run's),
    intact bands, unchanged inputs.  The first collected level writes out and does not read it."""
    c = hygiene.CASES[name]
    inputs = c.build()
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, inputs, "cuda", c.plane)
    assert len(session.workspaces) >= 3 and len(session.guards) > len(session.workspaces)
    for o in outs:
        assert o is None or bool(torch.isfinite(o.float()).all()), "poison reached an output"
    memguard.assert_same_outputs(outs, hygiene._clean(c), "poison %r" % poison)


# ---- the module ----
@functools.lru_cache(maxsize=None)
def _module_case():
    B, C, H, W, n, steps, kernels, norm = 2, 2, 19, 67, N_ITER, (0, 2, 5), (3, 5, 7), "8sum"
    gen = torch.Generator().manual_seed(77)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in kernels]
    _, h, s = _inputs(B, C, H, W, 3, "shared", 78)
    ic = [torch.softmax(torch.randn(B, len(steps), H, W, generator=gen), 1) for _ in kernels]   # the module's inputs: it applies no softmax itself
    kc = torch.softmax(torch.randn(B, len(kernels), H, W, generator=gen), 1)
    go = torch.randn(B, C, H, W, generator=gen)
    leaves = [t.double().requires_grad_(True) for t in gs + [h] + ic + [kc]]
    ics, kcs = leaves[4:7], leaves[7]
    ref = sum(kcs[:, k:k + 1] * torch_kxk_assemble(leaves[k], leaves[3], s.double(), ics[k], steps, K, norm) for k, K in enumerate(kernels))
    ref.backward(go.double())
    return dict(cpu=(gs, h, s, ic, kc, go), ref=ref.detach(), ref_grads=[t.grad for t in leaves], kernels=kernels, steps=steps, norm=norm, n=n)


def _run_module(c):
    gs, h, s, ic, kc, go = c["cpu"]
    leaves = [t.cuda().requires_grad_(True) for t in gs + [h] + ic + [kc]]
    m = cspn_amd.Affinity_PropagateAssemble(c["n"], c["kernels"], c["steps"], c["norm"])
    y = m(leaves[:3], leaves[3], s.cuda(), leaves[4:7], leaves[7])
    y.backward(go.cuda())
    return y.detach(), [t.grad for t in leaves]


@pytest.mark.gpu
def test_module_vs_fp64_autograd():
    c = _module_case()
    y, grads = _run_module(c)
    assert bool(torch.isfinite(c["ref"]).all()) and rel_err(y.cpu().numpy(), c["ref"].numpy()) <= RTOL
    names = ["guidance3", "guidance5", "guidance7", "blur_depth", "iter_conf3", "iter_conf5", "iter_conf7", "kernel_conf"]
    for got, want, what in zip(grads, c["ref_grads"], names):
        assert got is not None and _check(got.cpu().numpy(), want.numpy(), what)
    # on a non-default stream: the same bits
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        y2, grads2 = _run_module(c)
    st.synchronize()
    assert torch.equal(y2, y) and all(torch.equal(a, b) for a, b in zip(grads2, grads))
    # iter_conf None is ones, kernel_conf None no factor: the plain sum of the three propagations' last levels
    gs, h, s, _, _, _ = c["cpu"]
    with torch.no_grad():
        m = cspn_amd.Affinity_PropagateAssemble(c["n"], c["kernels"], None, c["norm"])
        plain = m([g.cuda() for g in gs], h.cuda(), s.cuda())
        want = sum(F.cspn2d_forward_kxk_norm(g.cuda(), h.cuda(), s.cuda(), K, c["n"], c["norm"]) for g, K in zip(gs, c["kernels"]))
        only_alpha = m([g.cuda() for g in gs], h.cuda(), s.cuda(), None, torch.full((2, 3, 19, 67), 0.5, device="cuda"))
    assert rel_err(plain.cpu().numpy(), want.cpu().numpy()) <= 1e-6 and rel_err(only_alpha.cpu().numpy(), 0.5 * want.cpu().numpy()) <= 1e-6
