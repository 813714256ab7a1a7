"""Dilated K x K propagation (dilated CSPN++, the first pass of PENet's refinement): the depth-completion and the assembling contract of the
K x K engine with the neighbour offset of gate channel k = (t, l) scaled by a dilation D in {1, 2},
    off_k = D * (K//2 - t, K//2 - l),
and nothing else changed (cspn2d_*_kxk_{norm,assemble}_dil; the keyword `dilation` of the four functional calls and of the two modules).
The float64 statement is tests/test_kxk_norm.py::torch_kxk_norm with ZeroPad2d (l D, (K-1-l) D, t D, (K-1-t) D) and the crop R D.
CPU: the statement (D = 1: torch_kxk_norm bit for bit; D = 2: an independently written shift-based definition; the NaN row of a 3 x 1 image),
     symbols, byte counts, argument errors, constructors and reprs.
GPU: forward and gradients against the statement at D = 2 over the shapes at which a 64 x 16 tile with a halo of up to 6 can go wrong, the
     assembling contract, D = 1 through the new entry points bitwise the old ones, 16-bit guidance, misaligned views, repeatability, guard bands
     and a stale arena, the modules and the PENet composition against float64 autograd.  Bounds: RTOL and _check, the project's own."""
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
from test_backward import GFLOOR, _check
from test_kxk_norm import RTOL, _cuda, _inputs, _misaligned, torch_kxk_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_forward_kxk_norm_dil", "cspn2d_backward_kxk_norm_dil", "cspn2d_forward_kxk_assemble_dil", "cspn2d_backward_kxk_assemble_dil"]
NORMS = ["8sum", "8sum_abs"]
N_ITER = 5


# ---- the float64 statement ----
def _offsets(K, D):
    R = K // 2
    return [(D * (R - t), D * (R - l)) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def _pads(K, D):
    R = K // 2
    return [(l * D, (K - 1 - l) * D, t * D, (K - 1 - t) * D) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def torch_kxk_levels_dil(guidance, blur, sparse, K, n, norm, D):
    """torch_kxk_norm's statements with the dilated pads and crop, keeping every level -> [H_0 .. H_n]"""
    c = (K // 2) * D
    P = _pads(K, D)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    gate = torch.stack([torch.nn.functional.pad(g[:, k], P[k]) for k in range(len(P))], 1)
    gate = gate / gate.abs().sum(1, keepdim=True)
    gsum = gate.sum(1, keepdim=True)[:, :, c:-c, c:-c]
    gate = gate.unsqueeze(2)
    m = sparse.sign() if sparse is not None else None
    x = blur
    levels = [x]
    for _ in range(n):
        xp = torch.stack([torch.nn.functional.pad(x, P[k]) for k in range(len(P))], 1)
        x = (1.0 - gsum) * blur + (gate * xp).sum(1)[:, :, c:-c, c:-c]
        if m is not None:
            x = (1 - m) * x + m * blur
        levels.append(x)
    return levels


def torch_kxk_norm_dil(guidance, blur, sparse, K, n, norm, D):
    return torch_kxk_levels_dil(guidance, blur, sparse, K, n, norm, D)[-1]


def torch_kxk_assemble_dil(guidance, blur, sparse, conf, steps, K, norm, D):
    levels = torch_kxk_levels_dil(guidance, blur, sparse, K, steps[-1], norm, D)
    out = conf[:, 0:1] * levels[steps[0]]
    for j in range(1, len(steps)):
        out = out + conf[:, j:j + 1] * levels[steps[j]]
    return out


def _shift(x, dy, dx):
    """y(p) = x(p + (dy, dx)), zero where that lies outside the image"""
    H, W = x.shape[-2:]
    y = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        y[..., y0:y1, x0:x1] = x[..., y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return y


def shift_kxk_norm(guidance, blur, sparse, K, n, norm, D):
    """the contract as the header states it, written with shifts: G_k(p) = g_k(p + off_k), wb = G / sum |G|, c = 1 - sum wb,
    H' = sum_k u wb_k H(p + off_k) + (u c + m) blur"""
    off = _offsets(K, D)
    g = guidance.abs() if norm == "8sum_abs" else guidance
    G = torch.stack([_shift(g[:, k], dy, dx) for k, (dy, dx) in enumerate(off)], 1)
    wb = G / G.abs().sum(1, keepdim=True)
    c = 1 - wb.sum(1, keepdim=True)
    m = sparse.sign() if sparse is not None else torch.zeros_like(blur[:, :1])
    u = 1 - m
    x = blur
    for _ in range(n):
        acc = torch.zeros_like(blur)
        for k, (dy, dx) in enumerate(off):
            acc = acc + u * wb[:, k:k + 1] * _shift(x, dy, dx)
        x = acc + (u * c + m) * blur
    return x


def _conf(B, T, H, W, seed):
    return torch.rand(B, T, H, W, generator=torch.Generator().manual_seed(seed))


# ---- CPU ----
@pytest.mark.parametrize("K", [3, 5, 7])
def test_statement_at_dilation_1_is_torch_kxk_norm_bit_for_bit(K):
    for (H, W), norm, sparse in (((2, 1), "8sum", None), ((3, 5), "8sum_abs", "shared"), ((17, 66), "8sum", "per")):
        g, h, s = (t.double() if t is not None else None for t in _inputs(2, 2, H, W, K, sparse, seed=K + W))
        a, b = torch_kxk_norm_dil(g, h, s, K, 3, norm, 1), torch_kxk_norm(g, h, s, K, 3, norm)
        assert memguard.same_bits(a, b), (H, W)


@pytest.mark.parametrize("K", [3, 5, 7])
def test_statement_at_dilation_2_is_the_shift_based_definition(K):
    for (H, W), norm, sparse in (((5, 8), "8sum", None), ((9, 14), "8sum_abs", "shared"), ((17, 21), "8sum", "per")):
        g, h, s = (t.double() if t is not None else None for t in _inputs(2, 2, H, W, K, sparse, seed=K + W))
        a, b = torch_kxk_norm_dil(g, h, s, K, 3, norm, 2), shift_kxk_norm(g, h, s, K, 3, norm, 2)
        assert bool(torch.isfinite(a).all()) and float((a - b).abs().max()) <= 1e-12, (H, W)


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("norm", NORMS)
def test_the_nan_row_of_a_3_by_1_image(K, norm):
    """every neighbour of the middle row lies outside the image at D = 2: 0 / 0, as the reference's torch.div; the other rows have one"""
    g, h, _ = (t.double() for t in _inputs(2, 2, 3, 1, K, "shared", seed=K))
    for f in (torch_kxk_norm_dil, shift_kxk_norm):
        nan = torch.isnan(f(g, h, None, K, 2, norm, 2))
        assert bool(nan[:, :, 1].all()) and not bool(nan[:, :, 0].any()) and not bool(nan[:, :, 2].any())
    assert bool(torch.isfinite(torch_kxk_norm_dil(g, h, None, K, 2, norm, 1)).all())


def test_new_symbols_are_exported_declared_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text)
        assert m, "not declared: " + s
        assert re.search(r"int K,\s*int dilation,\s*int n_iter", m.group(1)) and "int gate_dtype" in m.group(1), s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.late_symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert not any("dil" in n for n in cspn_amd.__all__)   # no new public name: the keyword on the four calls and the two modules


def test_byte_counts_do_not_depend_on_the_dilation():
    """no byte query takes a dilation, and the existing ones return what they returned: the fold, the levels, the history"""
    lib = cspn_amd.load()
    assert not any(hasattr(lib, n) for n in ("cspn2d_kxk_norm_dil_workspace_bytes", "cspn2d_kxk_norm_workspace_bytes_dil",
                                             "cspn2d_kxk_assemble_workspace_bytes_dil", "cspn2d_backward_kxk_norm_workspace_bytes_dil"))
    B, C, H, W, n = 2, 3, 10, 13, 4
    L = B * C * H * W
    lv = lambda x: (x + 63) // 64 * 64   # noqa: E731  (kxk_level_floats)
    r256 = lambda x: (x + 255) // 256 * 256   # noqa: E731
    for K in (3, 5, 7):
        fold = lv(B * (K * K - 1) * H * W) + lv(L)
        assert _lib.late_symbol("cspn2d_kxk_norm_workspace_bytes")(B, C, 1, H, W, K, n) == 4 * (fold + 2 * lv(L))
        assert _lib.late_symbol("cspn2d_kxk_norm_history_bytes")(B, C, H, W, K, n) == 4 * L * (n - 1)
        assert _lib.late_symbol("cspn2d_backward_kxk_norm_workspace_bytes")(B, C, 1, H, W, K, n) == 4 * 2 * fold + r256(4 * L * (n - 1))
        assert _lib.late_symbol("cspn2d_kxk_assemble_workspace_bytes")(B, C, 1, H, W, K, n) == 4 * (fold + 2 * lv(L))
        assert _lib.late_symbol("cspn2d_kxk_assemble_history_bytes")(B, C, H, W, K, n) == 4 * L * n
        assert _lib.late_symbol("cspn2d_backward_kxk_assemble_workspace_bytes")(B, C, 1, H, W, K, n) == 4 * 2 * fold + r256(4 * L * (n - 1)) + 4 * lv(L)


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    nf, nb, af, ab = (_lib.late_symbol(s) for s in NEW)
    g, x, s, o, h, w, gg, gx, cf, gc = (ctypes.c_void_p(i << 32) for i in range(1, 11))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    steps = (ctypes.c_int * 3)(0, 2, 3)
    hb = 4 * 2 * 8 * 8 * 3
    # (.., B, C, sparse_C, H, W, K, dilation, n_iter, norm, ws, ws_bytes, stream) behind each entry's own pointers
    calls = {
        "norm forward": lambda K, D, dt=0, ws=M: nf(g, dt, x, None, o, None, 0, 2, 1, 0, 8, 8, K, D, 3, 0, w, ws, None),
        "norm backward": lambda K, D, dt=0, ws=M: nb(g, dt, x, None, h, hb, o, gg, gx, 2, 1, 0, 8, 8, K, D, 3, 0, w, ws, None),
        "assemble forward": lambda K, D, dt=0, ws=M: af(g, dt, x, None, cf, steps, 3, o, None, 0, 2, 1, 0, 8, 8, K, D, 3, 0, w, ws, None),
        "assemble backward": lambda K, D, dt=0, ws=M: ab(g, dt, x, None, cf, steps, 3, h, hb, o, gg, gx, gc, 2, 1, 0, 8, 8, K, D, 3, 0, w, ws, None),
    }
    for what, call in calls.items():
        for D in (0, 3, -1, 4):
            assert call(5, D) == -1 and b"dilation" in err(), (what, D)
        assert call(4, 0) == -1 and b"dilation" in err(), what   # the dilation is checked first
        # the counterpart's checks are reached, at both dilations: K, the gate dtype, the workspace
        for D in (1, 2):
            assert call(4, D) == -1 and b"K must be" in err(), (what, D)
            assert call(5, D, 7) == -1 and b"dtype" in err(), (what, D)
            assert call(5, D, 0, 64) == -2 and b"workspace" in err(), (what, D)
            assert call(5, D, _lib.DTYPES["float16"], 64) == -2, (what, D)
    assert nf(None, 0, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"null" in err()
    assert nf(g, 0, x, None, x, None, 0, 2, 1, 0, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"alias" in err()
    assert nf(g, 0, x, None, o, None, 0, 2, 1, 0, 8, 8, 5, 2, 3, 2, w, M, None) == -1 and b"norm" in err()
    assert nb(g, 0, x, None, None, 0, o, gg, gx, 2, 1, 0, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"history" in err()
    bad = (ctypes.c_int * 3)(0, 2, 2)
    assert af(g, 0, x, None, cf, bad, 3, o, None, 0, 2, 1, 0, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"steps" in err()
    assert ab(g, 0, x, None, None, steps, 3, h, hb, o, gg, gx, gc, 2, 1, 0, 8, 8, 5, 2, 3, 0, w, M, None) == -1 and b"conf" in err()


BAD_DILATIONS = (0, 3, -1, True, 2.0, "2", None)


def test_python_argument_errors_without_gpu():
    g, h, s, cf = torch.rand(1, 24, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9)
    go = torch.rand(1, 2, 6, 9)
    for bad in BAD_DILATIONS:
        with pytest.raises(ValueError, match="dilation"):
            F.cspn2d_forward_kxk_norm(g, h, s, 5, 3, dilation=bad)
        with pytest.raises(ValueError, match="dilation"):
            F.cspn2d_backward_kxk_norm(g, h, s, go, 5, 3, dilation=bad)
        with pytest.raises(ValueError, match="dilation"):
            F.cspn2d_forward_kxk_assemble(g, h, s, cf, (1, 3), 5, 3, dilation=bad)
        with pytest.raises(ValueError, match="dilation"):
            F.cspn2d_backward_kxk_assemble(g, h, s, cf, (1, 3), go, 5, 3, dilation=bad)
    # the other checks are those of dilation 1; a well-formed call on the CPU reaches the engine, which is GPU-only
    with pytest.raises(ValueError, match="kernel_size"):
        F.cspn2d_forward_kxk_norm(g, h, s, 4, 3, dilation=2)
    with pytest.raises(ValueError, match="steps"):
        F.cspn2d_forward_kxk_assemble(g, h, s, cf, (3, 1), 5, 3, dilation=2)
    for call in (lambda: F.cspn2d_forward_kxk_norm(g, h, s, 5, 3, dilation=2), lambda: F.cspn2d_backward_kxk_norm(g, h, s, go, 5, 3, dilation=2),
                 lambda: F.cspn2d_forward_kxk_assemble(g, h, s, cf, (1, 3), 5, 3, dilation=2),
                 lambda: cspn_amd.Affinity_PropagateKxK(3, 5, dilation=2)(g, h, s),
                 lambda: cspn_amd.Affinity_PropagateKxK(3, 3, dilation=2)(torch.rand(1, 8, 6, 9), h, s),   # K = 3 dilated: the engine, not the ring
                 lambda: cspn_amd.Affinity_PropagateAssemble(3, (5,), (1, 3), dilations=2)([g], h, s)):
        with pytest.raises(cspn_amd.CspnError):
            call()
    assert F.cspn2d_forward_kxk_norm(g, h, s, 5, 0, dilation=2) is h
    # existing signatures used positionally stay: dilation is the trailing keyword
    for f, before in ((F.cspn2d_forward_kxk_norm, "guidance blur_depth sparse_depth kernel_size n_iter norm_type return_history"),
                      (F.cspn2d_backward_kxk_norm, "guidance blur_depth sparse_depth grad_out kernel_size n_iter norm_type history need_guidance need_blur"),
                      (F.cspn2d_forward_kxk_assemble, "guidance blur_depth sparse_depth conf steps kernel_size n_iter norm_type return_history"),
                      (F.cspn2d_backward_kxk_assemble,
                       "guidance blur_depth sparse_depth conf steps grad_out kernel_size n_iter norm_type history need_guidance need_blur need_conf")):
        p = inspect.signature(f).parameters
        assert list(p) == before.split() + ["dilation"] and p["dilation"].default == 1, f.__name__


def test_module_constructors_and_reprs():
    m = cspn_amd.Affinity_PropagateKxK(24, 5)
    assert m.dilation == 1 and repr(m) == "Affinity_PropagateKxK(prop_time=24, prop_kernel=5, norm_type='8sum')"
    m = cspn_amd.Affinity_PropagateKxK(24, 7, "8sum_abs", 2)
    assert m.dilation == 2 and "dilation=2" in repr(m) and list(m.parameters()) == [] and m.state_dict() == {}
    assert cspn_amd.Affinity_PropagateKxK(24, 3, dilation=2).dilation == 2
    a = cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5))
    assert a.dilations == (1, 1, 1)
    assert repr(a) == "Affinity_PropagateAssemble(prop_time=5, prop_kernels=(3, 5, 7), steps=(0, 2, 5), norm_type='8sum')"
    assert repr(cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5), "8sum", (1, 1, 1))) == repr(a)
    a = cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5), "8sum_abs", 2)
    assert a.dilations == (2, 2, 2) and "dilations=(2, 2, 2)" in repr(a)
    a = cspn_amd.Affinity_PropagateAssemble(5, (3, 3, 7), None, dilations=[2, 1, 2])   # the same kernel size at two dilations
    assert a.dilations == (2, 1, 2) and a.prop_kernels == (3, 3, 7) and list(a.parameters()) == []
    for bad in BAD_DILATIONS:
        with pytest.raises((ValueError, AssertionError)):
            cspn_amd.Affinity_PropagateKxK(24, 5, "8sum", bad)
        with pytest.raises((ValueError, AssertionError)):
            cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), None, "8sum", bad)
        with pytest.raises((ValueError, AssertionError)):
            cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), None, "8sum", (1, bad, 2))
    for wrong_length in ((2, 2), (1, 2, 1, 2), ()):
        with pytest.raises((ValueError, AssertionError)):
            cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), None, "8sum", wrong_length)


# ---- GPU ----
# the tile is 64 x 16 pixels, the halo at K = 7, D = 2 is 6: one exact tile; four tiles, W % 4 != 0 (scalar path), seams; 3 x 3 tiles on the vector
# path with the halo across both seams; an image smaller than the halo; the NaN row
SHAPES = [(16, 64), (17, 65), (33, 132), (5, 8), (3, 1)]
# every K and norm at every shape; C, n and the mask rotate so that each value meets each shape and each K
CASES = [(K, norm, H, W, (1, 3)[(i + j) % 2], (1, 2, 5)[(i + 2 * j) % 3], (None, "shared", "per")[(i // 2 + j) % 3])
         for i, (K, norm) in enumerate(itertools.product((3, 5, 7), NORMS)) for j, (H, W) in enumerate(SHAPES)]


def test_the_grid_reaches_every_value_of_every_factor():
    assert {c[0] for c in CASES} == {3, 5, 7} and {c[1] for c in CASES} == set(NORMS) and {c[2:4] for c in CASES} == set(SHAPES)
    assert {c[4] for c in CASES} == {1, 3} and {c[5] for c in CASES} == {1, 2, 5} and {c[6] for c in CASES} == {None, "shared", "per"}
    for shape in SHAPES:
        rows = [c for c in CASES if c[2:4] == shape]
        assert {c[0] for c in rows} == {3, 5, 7} and {c[1] for c in rows} == set(NORMS)


def _split_nans(got, want, what):
    """the NaN pattern must be the same; -> both with zeros there"""
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all(), "%s: NaN at %d elements, the statement at %d" % (what, gn.sum(), wn.sum())
    return np.where(gn, 0.0, got), np.where(wn, 0.0, want)


def _check_dguidance_3x1(got, want, dev, n):
    """dL/dguidance on the 3 x 1 image, where a relative measure has nothing to hold on to.  Rows 0 and 2 have exactly one neighbour inside the
    image (each other), so wb = g / |g| = +-1 whatever g is and the gradient is exactly zero: dG = (dwb - sign(G) wb dwb) / S, two equal terms of
    size <= n max|grad_out| max|blur| / min|g|.  The float64 autograd returns its own roundoff there (asserted: <= 1e-12); the engine is held to
    the project's absolute floor GFLOOR times the size of the two terms.  At the NaN row the contract defines no gradient: the padded statement
    gives NaN for n >= 2 (0 x NaN in its padded product) and 0 for n = 1, the shift-based statement 0 throughout; the engine gathers from
    outside the image there.  So that row is not compared for this tensor; out and dL/dblur are, NaN pattern and values."""
    got, want = got.detach().double().cpu().numpy()[:, :, (0, 2)], want.numpy()[:, :, (0, 2)]
    g, h, _, go = dev
    assert np.isfinite(got).all() and np.isfinite(want).all() and np.abs(want).max() <= 1e-12
    size = n * float(go.abs().max()) * float(h.abs().max()) / float(g.abs().min())
    print("dL/dguidance on 3 x 1: max |engine| %.3e, max |float64 autograd| %.3e, bound %.3e" % (np.abs(got).max(), np.abs(want).max(), GFLOOR * size))
    assert np.abs(got).max() <= GFLOOR * size


@functools.lru_cache(maxsize=None)
def _case(K, norm, H, W, C, n, sparse, D=2):
    """inputs (each drawn and placed on the device on its own), the float64 statement with its autograd gradients, the engine's results: made once"""
    B = 2
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K * 1000 + W * 10 + n)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(n + H))
    gt, ht = g.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = torch_kxk_norm_dil(gt, ht, s.double() if s is not None else None, K, n, norm, D)
    ref.backward(go.double())
    dev = _cuda(g, h, s, go)
    gd, hd, sd, god = dev
    out, hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True, dilation=D)
    grads = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, hist, dilation=D)
    return dict(dev=dev, ref=ref.detach(), ref_grads=(gt.grad, ht.grad), out=out, hist=hist, grads=grads)


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,C,n,sparse", CASES)
def test_forward_and_gradients_vs_fp64_statement(K, norm, H, W, C, n, sparse):
    c = _case(K, norm, H, W, C, n, sparse)
    assert bool(torch.isnan(c["ref"]).any()) == ((H, W) == (3, 1))
    got, want = _split_nans(c["out"], c["ref"], "out")
    e = rel_err(got, want)
    print("forward rel_err %.3e" % e)
    assert e <= RTOL
    gd, hd, sd, god = c["dev"]
    assert memguard.same_bits(F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, dilation=2), c["out"])   # through the ping-pong levels
    if (H, W) == (3, 1):
        _check_dguidance_3x1(c["grads"][0], c["ref_grads"][0], c["dev"], n)
    else:
        assert _check(*_split_nans(c["grads"][0], c["ref_grads"][0], "dL/dguidance"), "dL/dguidance")
    assert _check(*_split_nans(c["grads"][1], c["ref_grads"][1], "dL/dblur"), "dL/dblur")
    # the same without a kept history
    again = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, dilation=2)
    assert all(memguard.same_bits(a, b) for a, b in zip(again, c["grads"]))
    if (H, W) != (3, 1):   # dilation 2 is not dilation 1
        assert not torch.equal(F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm), c["out"])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("need_guidance,need_blur", [(True, False), (False, True), (False, False)])
def test_gradient_subsets(K, need_guidance, need_blur):
    args = (K, "8sum_abs", 17, 65, 3, 5, "per")
    c = _case(*args)
    gd, hd, sd, god = c["dev"]
    gg, gh = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, 5, "8sum_abs", need_guidance=need_guidance, need_blur=need_blur, dilation=2)
    assert (gg is None) != need_guidance and (gh is None) != need_blur
    assert (gg is None or torch.equal(gg, c["grads"][0])) and (gh is None or torch.equal(gh, c["grads"][1]))
    m = cspn_amd.Affinity_PropagateKxK(5, K, "8sum_abs", dilation=2)
    gl, hl = gd.clone().requires_grad_(need_guidance), hd.clone().requires_grad_(need_blur)
    y = m(gl, hl, sd)
    assert torch.equal(y.detach(), c["out"])
    if need_guidance or need_blur:
        y.backward(god)
        assert (gl.grad is not None) == need_guidance and (hl.grad is not None) == need_blur
        assert (gl.grad is None or torch.equal(gl.grad, c["grads"][0])) and (hl.grad is None or torch.equal(hl.grad, c["grads"][1]))


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W,C,n,sparse", [CASES[1], CASES[12], CASES[22], CASES[29]])
def test_two_identical_calls_give_identical_bits(K, norm, H, W, C, n, sparse):
    c = _case(K, norm, H, W, C, n, sparse)
    gd, hd, sd, god = c["dev"]
    out, hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True, dilation=2)
    grads = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, hist, dilation=2)
    kept = (n - 1) * out.numel()   # H_1 .. H_{n-1}; with n = 1 the history is an unwritten placeholder
    assert memguard.same_bits(out, c["out"]) and memguard.same_bits(hist[:kept], c["hist"][:kept])
    assert all(memguard.same_bits(a, b) for a, b in zip(grads, c["grads"]))


# ---- the assembling contract at D = 2: the steps of tests/test_kxk_assemble.py; shapes, C, masks and norms rotate ----
ASSEMBLE = [(K, steps, (17, 65, 16, 64, 33, 132)[2 * ((i + j) % 3):][:2], (1, 3)[(i + j) % 2], (None, "shared", "per")[(i + 2 * j) % 3], NORMS[(i + j) % 2])
            for i, K in enumerate((3, 5, 7)) for j, steps in enumerate(((0, 2, 5), (1, 5), (5,)))]


@functools.lru_cache(maxsize=None)
def _assemble_case(K, steps, shape, C, sparse, norm):
    B, (H, W) = 2, shape
    seed = K * 100 + len(steps) * 10 + C + W
    g, h, s = _inputs(B, C, H, W, K, sparse, seed)
    cf = _conf(B, len(steps), H, W, seed + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2))
    gt, ht, ct = (t.double().requires_grad_(True) for t in (g, h, cf))
    ref = torch_kxk_assemble_dil(gt, ht, s.double() if s is not None else None, ct, steps, K, norm, 2)
    ref.backward(go.double())
    dev = _cuda(g, h, s, cf, go)
    gd, hd, sd, cd, god = dev
    out, hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, N_ITER, norm, return_history=True, dilation=2)
    grads = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, hist, dilation=2)
    return dict(dev=dev, ref=ref.detach(), ref_grads=(gt.grad, ht.grad, ct.grad), out=out, hist=hist, grads=grads)


@pytest.mark.gpu
@pytest.mark.parametrize("K,steps,shape,C,sparse,norm", ASSEMBLE)
def test_assemble_forward_and_three_gradients_vs_fp64_autograd(K, steps, shape, C, sparse, norm):
    c = _assemble_case(K, steps, shape, C, sparse, norm)
    assert bool(torch.isfinite(c["ref"]).all())
    e = rel_err(c["out"].cpu().numpy(), c["ref"].numpy())
    print("forward rel_err %.3e" % e)
    assert e <= RTOL
    gd, hd, sd, cd, god = c["dev"]
    assert torch.equal(F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, N_ITER, norm, dilation=2), c["out"])
    B, _, H, W = hd.shape
    levels = torch_kxk_levels_dil(gd.cpu().double(), hd.cpu().double(), sd.cpu().double() if sd is not None else None, K, N_ITER, norm, 2)
    hist = c["hist"].view(N_ITER, B, C, H, W).cpu()
    for t in range(1, N_ITER + 1):
        assert rel_err(hist[t - 1].numpy(), levels[t].numpy()) <= RTOL, t
    for got, want, what in zip(c["grads"], c["ref_grads"], ("dL/dguidance", "dL/dblur", "dL/dconf")):
        assert _check(got.cpu().numpy(), want.numpy(), what)
    again = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, dilation=2)   # runs its own forward for the history
    assert all(torch.equal(a, b) for a, b in zip(again, c["grads"]))
    for off in range(3):
        need = [i != off for i in range(3)]
        part = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, N_ITER, norm, c["hist"], *need, dilation=2)
        for i in range(3):
            assert (part[i] is None) if i == off else torch.equal(part[i], c["grads"][i]), (off, i)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("H,W,C,sparse,norm", [(17, 65, 3, "per", "8sum"), (33, 132, 1, "shared", "8sum_abs")])
def test_one_step_and_unit_confidence_is_bitwise_the_dilated_norm_call(K, H, W, C, sparse, norm):
    B, n = 2, N_ITER
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K + W)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3))
    gd, hd, sd, god = _cuda(g, h, s, go)
    ones = torch.ones(B, 1, H, W, device="cuda")
    out, hist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, ones, (n,), K, n, norm, return_history=True, dilation=2)
    want, want_hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True, dilation=2)
    assert torch.equal(out, want) and torch.equal(F.cspn2d_forward_kxk_assemble(gd, hd, sd, ones, (n,), K, n, norm, dilation=2), want)
    L = out.numel()
    assert torch.equal(hist[:(n - 1) * L], want_hist[:(n - 1) * L]) and torch.equal(hist[(n - 1) * L:n * L].view_as(out), want)
    gg, gb, _ = F.cspn2d_backward_kxk_assemble(gd, hd, sd, ones, (n,), god, K, n, norm, hist, dilation=2)
    wg, wb = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, want_hist, dilation=2)
    assert torch.equal(gg, wg) and torch.equal(gb, wb)


# ---- dilation 1 through the new entry points ----
def _always_dil(stem, dt, dilation):
    """F._kxk_entry without its shortcut: every call goes to the _dil entry point, dilation 1 included"""
    F.check_dilation(dilation)
    return stem + "_dil", (0 if dt is None else dt,), (dilation,)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,H,W,C,sparse,norm,steps", [(3, 17, 65, 3, "per", "8sum", (0, 2, 5)), (5, 33, 132, 1, "shared", "8sum_abs", (1, 5)),
                                                      (7, 17, 65, 3, None, "8sum", (5,)), (7, 16, 64, 1, "shared", "8sum_abs", (0, 2, 5))])
def test_dilation_1_through_the_new_entry_points_is_bitwise_the_existing_ones(monkeypatch, dtype, K, H, W, C, sparse, norm, steps):
    B, n = 2, N_ITER
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K + H)
    cf = _conf(B, len(steps), H, W, K)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(K))
    gd, hd, sd, cd, god = _cuda(g.to(dtype), h, s, cf, go)

    def run():
        out, hist = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, return_history=True, dilation=1)
        plain = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, dilation=1)
        grads = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, hist, dilation=1)
        aout, ahist = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, n, norm, return_history=True, dilation=1)
        aplain = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, n, norm, dilation=1)
        agrads = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, n, norm, ahist, dilation=1)
        return (out, hist, plain) + tuple(grads) + (aout, ahist, aplain) + tuple(agrads)
    old = run()
    names = []
    launch = F._launch
    monkeypatch.setattr(F, "_launch", lambda name, *a, **k: (names.append(name), launch(name, *a, **k))[1])
    assert len(run()) == len(old) and names and not any(nm.endswith("_dil") for nm in names)   # dilation 1 calls the entry points used before
    del names[:]
    monkeypatch.setattr(F, "_kxk_entry", _always_dil)
    new = run()
    assert sorted(set(names)) == sorted(NEW)
    assert old[3].dtype == dtype
    memguard.assert_same_outputs(new, old, "dilation 1 through the _dil entry points")


# ---- 16-bit guidance at D = 2 ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K,H,W,C,sparse,norm,steps", [(3, 33, 132, 3, "per", "8sum", (0, 2, 5)), (5, 17, 65, 1, "shared", "8sum_abs", (1, 5)),
                                                      (7, 33, 132, 3, None, "8sum", (5,)), (7, 17, 65, 2, "shared", "8sum_abs", (0, 2, 5))])
def test_16_bit_guidance_is_bitwise_the_float32_call_on_the_widened_tensor(dtype, K, H, W, C, sparse, norm, steps):
    B, n = 2, N_ITER
    g, h, s = _inputs(B, C, H, W, K, sparse, seed=K)
    cf = _conf(B, len(steps), H, W, K + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(K + 2))
    g16, hd, sd, cd, god = _cuda(g.to(dtype), h, s, cf, go)
    g32 = g16.float()
    out, hist = F.cspn2d_forward_kxk_norm(g16, hd, sd, K, n, norm, return_history=True, dilation=2)
    want, want_hist = F.cspn2d_forward_kxk_norm(g32, hd, sd, K, n, norm, return_history=True, dilation=2)
    assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb = F.cspn2d_backward_kxk_norm(g16, hd, sd, god, K, n, norm, hist, dilation=2)
    wg, wb = F.cspn2d_backward_kxk_norm(g32, hd, sd, god, K, n, norm, want_hist, dilation=2)
    assert gg.dtype == dtype and torch.equal(gg, wg.to(dtype)) and torch.equal(gb, wb)   # the float32 gradient rounded once
    out, hist = F.cspn2d_forward_kxk_assemble(g16, hd, sd, cd, steps, K, n, norm, return_history=True, dilation=2)
    want, want_hist = F.cspn2d_forward_kxk_assemble(g32, hd, sd, cd, steps, K, n, norm, return_history=True, dilation=2)
    assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(hist, want_hist)
    gg, gb, gc = F.cspn2d_backward_kxk_assemble(g16, hd, sd, cd, steps, god, K, n, norm, hist, dilation=2)
    wg, wb, wc = F.cspn2d_backward_kxk_assemble(g32, hd, sd, cd, steps, god, K, n, norm, want_hist, dilation=2)
    assert gg.dtype == dtype and torch.equal(gg, wg.to(dtype)) and torch.equal(gb, wb) and torch.equal(gc, wc)


# ---- views one element off a 16-byte boundary with W % 4 == 0: the guarded scalar kernels, the same bits ----
@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("H,W", [(16, 64), (33, 132)])
def test_misaligned_views(K, H, W):
    B, C, n, norm, steps = 2, 2, N_ITER, "8sum", (0, 2, 5)
    g, h, s = _inputs(B, C, H, W, K, "per", seed=K + W)
    cf = _conf(B, len(steps), H, W, K)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(2))

    def run(gd, hd, sd, cd, god):
        out = F.cspn2d_forward_kxk_norm(gd, hd, sd, K, n, norm, dilation=2)
        grads = F.cspn2d_backward_kxk_norm(gd, hd, sd, god, K, n, norm, dilation=2)
        aout = F.cspn2d_forward_kxk_assemble(gd, hd, sd, cd, steps, K, n, norm, dilation=2)
        agrads = F.cspn2d_backward_kxk_assemble(gd, hd, sd, cd, steps, god, K, n, norm, dilation=2)
        return (out,) + tuple(grads) + (aout,) + tuple(agrads)
    aligned = run(*_cuda(g, h, s, cf, go))
    off = [_misaligned(t.cuda()) for t in (g, h, s, cf, go)]
    assert all(t.storage_offset() == 1 for t in off)
    memguard.assert_same_outputs(run(*off), aligned, "one element off")
    ref = torch_kxk_norm_dil(g.double(), h.double(), s.double(), K, n, norm, 2)
    assert rel_err(aligned[0].cpu().numpy(), ref.numpy()) <= RTOL
    # a 16-bit guidance at an address that is no multiple of 8
    buf = torch.empty(g.numel() + 1, dtype=torch.bfloat16, device="cuda")
    g16 = buf[1:].view(g.shape)
    g16.copy_(g)
    assert g16.data_ptr() % 8 != 0
    gd, hd, sd, cd, god = off
    want = run(g16.float(), hd, sd, cd, god)
    got = run(g16, hd, sd, cd, god)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b.to(a.dtype)), i


# ---- memory hygiene: the four dilated calls and both modules between guard bands on NaN and on finite poison, and in a stale arena ----
def _hygiene_inputs(K, H, W, C, sparse, dtype, steps, seed):
    B = 2
    g, h, s = _inputs(B, C, H, W, K, sparse, seed)
    cf = _conf(B, len(steps), H, W, seed + 1)
    go = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed + 2))
    return tuple(_cuda(g.to(dtype), h, s, cf, go))


def _hygiene_call(K, steps, norm):
    n = steps[-1]

    def call(g, h, s, cf, go):
        out = F.cspn2d_forward_kxk_norm(g, h, s, K, n, norm, dilation=2)
        out2, hist = F.cspn2d_forward_kxk_norm(g, h, s, K, n, norm, return_history=True, dilation=2)
        gg, gb = F.cspn2d_backward_kxk_norm(g, h, s, go, K, n, norm, hist, dilation=2)
        alone = F.cspn2d_backward_kxk_norm(g, h, s, go, K, n, norm, None, False, True, dilation=2)[1]
        aout = F.cspn2d_forward_kxk_assemble(g, h, s, cf, steps, K, n, norm, dilation=2)
        aout2, ahist = F.cspn2d_forward_kxk_assemble(g, h, s, cf, steps, K, n, norm, return_history=True, dilation=2)
        ag, ab, ac = F.cspn2d_backward_kxk_assemble(g, h, s, cf, steps, go, K, n, norm, ahist, dilation=2)
        aalone = F.cspn2d_backward_kxk_assemble(g, h, s, cf, steps, go, K, n, norm, None, False, True, False, dilation=2)[1]
        return out, out2, hist, gg, gb, alone, aout, aout2, ahist, ag, ab, ac, aalone
    return call


def _modules_inputs(H, W):
    B, C = 2, 2
    gen = torch.Generator().manual_seed(9 + W)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in (3, 5, 7)]
    _, h, s = _inputs(B, C, H, W, 3, "shared", 10)
    ic = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    kc = torch.softmax(torch.randn(B, 3, H, W, generator=gen), 1)
    go = torch.randn(B, C, H, W, generator=gen)
    return tuple(_cuda(gs[0], gs[1].half(), gs[2], h, s, ic, kc, go))


def _modules_call(g3, g5, g7, h, s, ic, kc, go):
    """Affinity_PropagateKxK at dilation 2 feeding Affinity_PropagateAssemble at dilations (2, 2, 1)"""
    leaves = [hygiene._leaf(t) for t in (g3, g5, g7, h, ic, kc)]
    first = cspn_amd.Affinity_PropagateKxK(3, 5, "8sum", dilation=2)
    second = cspn_amd.Affinity_PropagateAssemble(5, (3, 5, 7), (0, 2, 5), "8sum", dilations=(2, 2, 1))
    y = second(leaves[:3], first(leaves[1], leaves[3], s), s, [leaves[4]] * 3, leaves[5])
    y.backward(go)
    return (y.detach(),) + tuple(t.grad for t in leaves)


HYGIENE = {}
for _K, _steps, (_H, _W), _C, _sparse, _dt, _norm in ((3, (0, 2, 5), (17, 65), 3, "per", torch.float32, "8sum"), (5, (1, 5), (33, 132), 1, "shared", torch.bfloat16, "8sum_abs"),
                                                      (7, (0, 2, 5), (33, 132), 3, None, torch.float32, "8sum"), (7, (5,), (17, 65), 3, "shared", torch.float16, "8sum_abs")):
    _name = "kxk-dilation-K%d-%dx%d-%s" % (_K, _H, _W, str(_dt).split(".")[1])
    HYGIENE[_name] = hygiene.Case(_name, ("cspn2d_forward_kxk_norm", "cspn2d_backward_kxk_norm", "cspn2d_forward_kxk_assemble", "cspn2d_backward_kxk_assemble"),
                                  "the _dil entry points at dilation 2", 4 * 2 * _C * _H * _W,
                                  functools.lru_cache(maxsize=None)(functools.partial(_hygiene_inputs, _K, _H, _W, _C, _sparse, _dt, _steps, 60 + _K)),
                                  _hygiene_call(_K, _steps, _norm), lambda: None, "test_kxk_dilation.py::test_forward_and_gradients_vs_fp64_statement",
                                  False, None, None)
for _H, _W in ((17, 65), (33, 132)):
    _name = "kxk-dilation-modules-%dx%d" % (_H, _W)
    HYGIENE[_name] = hygiene.Case(_name, ("Affinity_PropagateKxK", "Affinity_PropagateAssemble"), "the dilated module feeding the assembling one",
                                  4 * 2 * 2 * _H * _W, functools.lru_cache(maxsize=None)(functools.partial(_modules_inputs, _H, _W)), _modules_call,
                                  lambda: None, "test_kxk_dilation.py::test_modules_vs_fp64_autograd", False, None, None)


def test_the_guarded_cases_stay_out_of_the_shared_table():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_dilated_call_between_guard_bands(name, poison):
    """out, the workspace and the history lie between guard bands and are poisoned before the call: clean outputs (bitwise the unguarded run's),
    intact bands, unchanged inputs.  The wider halo is where a read outside the image's planes would show."""
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
    """the dilated calls of both shapes and the modules through one workspace arena that is never refilled: every result bitwise the clean one"""
    steps = []
    for name in ("kxk-dilation-K7-33x132-float32", "kxk-dilation-K5-33x132-bfloat16", "kxk-dilation-modules-33x132", "kxk-dilation-K3-17x65-float32",
                 "kxk-dilation-K7-17x65-float16", "kxk-dilation-modules-17x65", "kxk-dilation-K7-33x132-float32"):
        c = HYGIENE[name]
        steps.append((name, c.call, c.build()))
    hygiene._run_sequence(steps, 4 * 2 * 3 * 33 * 132)


# ---- the modules against float64 autograd ----
def _grads_close(got, want, names):
    for a, b, what in zip(got, want, names):
        assert a is not None and _check(a.cpu().numpy(), b.numpy(), what)


@pytest.mark.gpu
@pytest.mark.parametrize("K,norm,H,W", [(3, "8sum", 17, 65), (5, "8sum_abs", 33, 132), (7, "8sum", 17, 65)])
def test_module_kxk_vs_fp64_autograd(K, norm, H, W):
    g, h, s = _inputs(2, 2, H, W, K, "shared", seed=K)
    go = torch.randn(2, 2, H, W, generator=torch.Generator().manual_seed(K))
    gt, ht = g.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = torch_kxk_norm_dil(gt, ht, s.double(), K, 5, norm, 2)
    ref.backward(go.double())
    m = cspn_amd.Affinity_PropagateKxK(5, K, norm, dilation=2)
    gd, hd = g.cuda().requires_grad_(True), h.cuda().requires_grad_(True)
    y = m(gd, hd, s.cuda())
    assert "_CSPN2dKxKNormFunction" in type(y.grad_fn).__name__   # K = 3 too: the K x K engine, not the ring
    y.backward(go.cuda())
    assert rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) <= RTOL
    _grads_close((gd.grad, hd.grad), (gt.grad, ht.grad), ("guidance", "blur_depth"))
    with torch.no_grad():
        assert torch.equal(m(gd, hd, s.cuda()), y.detach())
        assert torch.equal(y.detach(), F.cspn2d_forward_kxk_norm(gd, hd, s.cuda(), K, 5, norm, dilation=2))


@functools.lru_cache(maxsize=None)
def _modules_case():
    B, C, H, W, n, steps, kernels, norm = 2, 2, 17, 65, N_ITER, (0, 2, 5), (3, 5, 7), "8sum"
    gen = torch.Generator().manual_seed(77)
    gs = [torch.randn(B, K * K - 1, H, W, generator=gen) for K in kernels + kernels]   # the dilated pass's guidances, then the second pass's
    _, h, s = _inputs(B, C, H, W, 3, "shared", 78)
    ic = [torch.softmax(torch.randn(B, len(steps), H, W, generator=gen), 1) for _ in kernels + kernels]
    kc = [torch.softmax(torch.randn(B, len(kernels), H, W, generator=gen), 1) for _ in range(2)]
    go = torch.randn(B, C, H, W, generator=gen)
    return dict(gs=gs, h=h, s=s, ic=ic, kc=kc, go=go, kernels=kernels, steps=steps, norm=norm, n=n)


def _assemble_ref(gs, h, s, ic, kc, c, dilations):
    return sum(kc[:, k:k + 1] * torch_kxk_assemble_dil(gs[k], h, s, ic[k], c["steps"], K, c["norm"], dilations[k]) for k, K in enumerate(c["kernels"]))


@pytest.mark.gpu
def test_modules_vs_fp64_autograd():
    """Affinity_PropagateAssemble at dilations (2, 2, 1), and the composition a PENet port writes: the module at dilation 2 feeding the one at 1"""
    c = _modules_case()
    names = ["guidance%d" % K for K in c["kernels"]] + ["blur_depth"] + ["iter_conf%d" % K for K in c["kernels"]] + ["kernel_conf"]
    # one module, mixed dilations
    leaves = [t.double().requires_grad_(True) for t in c["gs"][:3] + [c["h"]] + c["ic"][:3] + [c["kc"][0]]]
    ref = _assemble_ref(leaves[:3], leaves[3], c["s"].double(), leaves[4:7], leaves[7], c, (2, 2, 1))
    ref.backward(c["go"].double())
    dev = [t.cuda().requires_grad_(True) for t in c["gs"][:3] + [c["h"]] + c["ic"][:3] + [c["kc"][0]]]
    m = cspn_amd.Affinity_PropagateAssemble(c["n"], c["kernels"], c["steps"], c["norm"], dilations=(2, 2, 1))
    y = m(dev[:3], dev[3], c["s"].cuda(), dev[4:7], dev[7])
    y.backward(c["go"].cuda())
    assert bool(torch.isfinite(ref).all()) and rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) <= RTOL
    _grads_close([t.grad for t in dev], [t.grad for t in leaves], names)
    # the PENet composition: dilation 2, then dilation 1, each with its own guidances and confidences
    leaves = [t.double().requires_grad_(True) for t in c["gs"] + [c["h"]] + c["ic"] + c["kc"]]
    mid = _assemble_ref(leaves[0:3], leaves[6], c["s"].double(), leaves[7:10], leaves[13], c, (2, 2, 2))
    ref = _assemble_ref(leaves[3:6], mid, c["s"].double(), leaves[10:13], leaves[14], c, (1, 1, 1))
    ref.backward(c["go"].double())
    dev = [t.cuda().requires_grad_(True) for t in c["gs"] + [c["h"]] + c["ic"] + c["kc"]]
    dilated = cspn_amd.Affinity_PropagateAssemble(c["n"], c["kernels"], c["steps"], c["norm"], dilations=2)
    plain = cspn_amd.Affinity_PropagateAssemble(c["n"], c["kernels"], c["steps"], c["norm"])
    y = plain(dev[3:6], dilated(dev[0:3], dev[6], c["s"].cuda(), dev[7:10], dev[13]), c["s"].cuda(), dev[10:13], dev[14])
    y.backward(c["go"].cuda())
    assert bool(torch.isfinite(ref).all()) and rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) <= RTOL
    both = ["dilated " + n for n in names[:3]] + ["plain " + n for n in names[:3]] + ["blur_depth"] + ["dilated " + n for n in names[4:7]] + \
           ["plain " + n for n in names[4:7]] + ["dilated kernel_conf", "plain kernel_conf"]
    _grads_close([t.grad for t in dev], [t.grad for t in leaves], both)
