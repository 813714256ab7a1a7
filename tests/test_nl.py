"""Non-local propagation with learned offsets (cspn2d_*_nl*, cspn_amd/csrc/cspn2d_nl.hip, cspn_amd/nlspn.py): the seven entry points, the four
functions of cspn_amd.functional and the module NonLocal_Propagate against a float64 statement of the contract.

The statement (bases / bil / nl_levels) is the contract of include/cspn_amd.h written in torch: the fractions come from the OFFSET, the integer
part is added in integer arithmetic, a corner outside the image contributes 0.  Bounds: helpers.RTOL on the forward, test_backward._check on every
gradient -- the same statement evaluated in float32 stays below 7e-7 in the forward and below 5 % of _check's bound in every gradient on these inputs.

The backward is the engine's first path that is NOT run-to-run bitwise: the adjoint of the gather is a scatter with float atomics, whose sums
depend on arrival order in their last bits.  So backward results are compared within _check (with the statement, and with each other), never bit
for bit; the forward and the sampling operator are compared bit for bit.

Offsets on the GPU are finite.  NaN and infinite offsets are covered by the kernel's inside-test (!(y0 >= 0 && y0 < H) on clamped integers,
cspn2d_nl.hip: tap_of), not by a run."""
import contextlib
import ctypes
import functools
import inspect
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
from cspn_amd import nlspn
from helpers import RTOL, rel_err
from test_backward import _check
from test_kxk_norm import _cuda, _misaligned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_nl_workspace_bytes", "cspn2d_nl_history_bytes", "cspn2d_forward_nl_f32", "cspn2d_backward_nl_workspace_bytes", "cspn2d_backward_nl_f32",
       "cspn2d_nl_sample_f32", "cspn2d_nl_sample_backward_f32"]
FUNCS = ["cspn2d_forward_nl", "cspn2d_backward_nl", "cspn2d_nl_sample", "cspn2d_nl_sample_backward"]
B, N_ITER = 2, 4
# smaller than a tile; one exact forward tile (64 x 16) on the vector path; the scalar path with seams; 3 x 3 forward tiles on the vector path
SHAPES = [(5, 8), (16, 64), (17, 65), (33, 132)]
KINDS = ["normal", "integer", "hot", "huge"]
MODES = ["AS", "ASS", "TC", "TGASS"]
GAMMA = 0.15   # affinity_gamma of the module tests: scale = 1.2, so that the abs-sum of tanh(g) / scale falls on both sides of the max(., 1)


# ---- the float64 statement ----
def bases(K):
    R = K // 2
    return [(t - R, l - R) for t in range(K) for l in range(K) if (t, l) != (R, R)]


def bil(F_, dy, dx, by, bx):                      # F_ [B,C,H,W], dy/dx [B,H,W]
    Bn, C, H, W = F_.shape
    fy0, fx0 = dy.floor(), dx.floor()
    fy, fx = dy - fy0, dx - fx0
    lim = float(H + W + 8)
    y0 = torch.arange(H).view(1, H, 1) + by + fy0.clamp(-lim, lim).long()
    x0 = torch.arange(W).view(1, 1, W) + bx + fx0.clamp(-lim, lim).long()
    out = 0
    for cy, wy in ((y0, 1 - fy), (y0 + 1, fy)):
        for cx, wx in ((x0, 1 - fx), (x0 + 1, fx)):
            ok = (cy >= 0) & (cy < H) & (cx >= 0) & (cx < W)
            idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).view(Bn, 1, H * W).expand(Bn, C, H * W)
            out = out + (wy * wx * ok).unsqueeze(1) * F_.reshape(Bn, C, H * W).gather(2, idx).view(Bn, C, H, W)
    return out


def bil_grid(F_, dy, dx, by, bx):
    """the same sample through grid_sample(align_corners=True, padding_mode='zeros') on the absolute coordinate p + base + d"""
    Bn, C, H, W = F_.shape
    y = torch.arange(H, dtype=F_.dtype).view(1, H, 1) + by + dy
    x = torch.arange(W, dtype=F_.dtype).view(1, 1, W) + bx + dx
    grid = torch.stack((2 * x / max(W - 1, 1) - 1, 2 * y / max(H - 1, 1) - 1), -1)
    return torch.nn.functional.grid_sample(F_, grid, mode="bilinear", padding_mode="zeros", align_corners=True)


def nl_levels(aff, off, x, sparse, n, K=3, sample=bil):
    m = None if sparse is None else (sparse > 0).to(x.dtype)
    c = 1 - aff.sum(1, keepdim=True)
    h, levels = x, [x]
    for _ in range(n):
        ht = h if m is None else (1 - m) * h + m * sparse
        h = c * ht + sum(aff[:, k:k + 1] * sample(ht, off[:, 2 * k], off[:, 2 * k + 1], by, bx) for k, (by, bx) in enumerate(bases(K)))
        levels.append(h)
    return levels


def sample_all(off, f, K=3, sample=bil):
    return torch.cat([sample(f, off[:, 2 * k], off[:, 2 * k + 1], by, bx) for k, (by, bx) in enumerate(bases(K))], 1)


def ref_normalize(mode, g, off, conf, scale, K=3):
    """the module's three steps as formulas: squash, confidence, abs-sum"""
    KK = K * K - 1
    a = g
    if mode == "TC":
        a = torch.tanh(g) / KK
    elif mode == "TGASS":
        a = torch.tanh(g) / (scale + 1e-8)
    if conf is not None:
        a = a * sample_all(off, conf, K)
    if mode == "TC":
        return a
    S = a.abs().sum(1, keepdim=True) + 1e-4
    if mode != "AS":
        S = torch.maximum(S, torch.ones_like(S))
    return a / S


def _offsets(kind, H, W, gen):
    d = torch.randn(B, 16, H, W, generator=gen) * 1.5
    if kind == "integer":      # weights exactly 0 or 1: the derivative convention at integer coordinates shows
        d = d.round()
    elif kind == "hot":        # every neighbour of every pixel reads (H//2 + 0.25, W//2 + 0.5): all adds of a step land on four addresses
        y = torch.arange(H, dtype=torch.float32).view(1, H, 1)
        x = torch.arange(W, dtype=torch.float32).view(1, 1, W)
        for k, (by, bx) in enumerate(bases(3)):
            d[:, 2 * k] = (H // 2 + 0.25) - y - by
            d[:, 2 * k + 1] = (W // 2 + 0.5) - x - bx
    elif kind == "huge":       # a fifth of the entries at +-1e9: far outside, and far outside what an int holds after the base is added
        far = torch.rand(B, 16, H, W, generator=gen) < 0.2
        sign = (torch.rand(B, 16, H, W, generator=gen) < 0.5).float() * 2 - 1
        d = torch.where(far, sign * 1e9, d)
    return d


def _inputs(H, W, C, sparse, kind, seed):
    """aff randn * 0.2, the offsets of `kind`, values in [0.1, 10), a 10 % mask with values in [0.1, 5.1], grad_out randn"""
    gen = torch.Generator().manual_seed(seed)
    aff = torch.randn(B, 8, H, W, generator=gen) * 0.2
    off = _offsets(kind, H, W, gen)
    x = torch.rand(B, C, H, W, generator=gen) * 9.9 + 0.1
    s = (torch.rand(B, 1, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, H, W, generator=gen) * 5 + 0.1) if sparse else None
    go = torch.randn(B, C, H, W, generator=gen)
    return aff, off, x, s, go


# the grid, thinned: every kind with and without a mask at every shape; C alternates so that both counts meet every shape, kind and mask setting
CASES = [(H, W, (1, 3)[(i + j + sp) % 2], bool(sp), kind) for i, (H, W) in enumerate(SHAPES) for j, kind in enumerate(KINDS) for sp in (0, 1)]


def _seed(H, W, C, sparse, kind):
    return 7000 + 10 * W + 100 * KINDS.index(kind) + C + (50 if sparse else 0)


# =================================================================================================================================== CPU
def test_the_two_forms_of_the_statement_agree():
    gen = torch.Generator().manual_seed(1)
    H, W, C, n = 17, 33, 3, 4
    aff = (torch.randn(B, 8, H, W, generator=gen) * 0.2).double()
    off = (torch.randn(B, 16, H, W, generator=gen) * 1.5).double()
    x = (torch.rand(B, C, H, W, generator=gen) * 9.9 + 0.1).double()
    s = ((torch.rand(B, 1, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, H, W, generator=gen) * 5 + 0.1)).double()
    go = torch.randn(B, C, H, W, generator=gen).double()
    res = []
    for sample in (bil, bil_grid):
        leaves = [t.clone().requires_grad_(True) for t in (aff, off, x)]
        out = nl_levels(*leaves, s, n, sample=sample)[-1]
        out.backward(go)
        res.append([out.detach()] + [t.grad for t in leaves])
    for a, b, what in zip(res[0], res[1], ("out", "grad_aff", "grad_offset", "grad_x")):
        assert rel_err(a.numpy(), b.numpy()) <= 1e-12, what


def test_zero_offsets_are_the_shifted_sum_over_a_zero_padded_plane():
    gen = torch.Generator().manual_seed(2)
    H, W, C, n = 9, 14, 2, 3
    aff = (torch.randn(B, 8, H, W, generator=gen) * 0.2).double()
    x = torch.rand(B, C, H, W, generator=gen).double()
    h = x
    for _ in range(n):
        pad = torch.nn.functional.pad(h, (1, 1, 1, 1))
        h = (1 - aff.sum(1, keepdim=True)) * h + sum(aff[:, k:k + 1] * pad[:, :, 1 + by:1 + by + H, 1 + bx:1 + bx + W] for k, (by, bx) in enumerate(bases(3)))
    assert torch.equal(nl_levels(aff, torch.zeros(B, 16, H, W, dtype=torch.float64), x, None, n)[-1], h)
    # the base is the deformable convolution's: neighbour 0 lies up and to the left, the opposite of the K x K engine's (1, 1)
    assert bases(3) == [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def test_new_symbols_are_exported_declared_and_the_surface_is_as_agreed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text)
        assert m, "not declared: " + s
        assert "int K" in m.group(1), s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    # the package's __all__ is what it was (its names are tied to the shared hygiene table); the module is importable from the package, the
    # functions are cspn_amd.functional's
    assert len(cspn_amd.__all__) == 36 and not any("nl" in n.lower().split("_") or "NonLocal" in n for n in cspn_amd.__all__)
    assert cspn_amd.NonLocal_Propagate is nlspn.NonLocal_Propagate
    assert all(callable(getattr(F, f)) for f in FUNCS) and not any(hasattr(cspn_amd, f) for f in FUNCS)
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(F.cspn2d_forward_nl) == "aff offset x sparse_depth n_iter kernel_size return_history".split()
    assert sig(F.cspn2d_backward_nl) == "aff offset x sparse_depth grad_out n_iter kernel_size history need_aff need_offset need_x".split()
    assert sig(F.cspn2d_nl_sample) == "offset f kernel_size".split()
    assert sig(F.cspn2d_nl_sample_backward) == "offset f grad_out kernel_size need_f need_offset".split()
    assert sig(nlspn.NonLocal_Propagate.forward) == "self affinity offset feat confidence sparse_depth n_iter".split()
    assert sig(nlspn.NonLocal_Propagate.__init__) == "self prop_time prop_kernel affinity affinity_gamma preserve_input".split()


def test_byte_queries():
    ws, hb, bws = (_lib.symbol(s) for s in ("cspn2d_nl_workspace_bytes", "cspn2d_nl_history_bytes", "cspn2d_backward_nl_workspace_bytes"))
    Bq, C, H, W = 2, 3, 17, 65
    L = Bq * C * H * W
    level = 4 * ((L + 63) // 64 * 64)
    # forward: the pinned H_0 (with sparse) and the ping-pong pair; nothing for one unmasked step
    for n, plain, masked in ((0, 0, 0), (1, 0, 1), (2, 1, 2), (3, 2, 2), (18, 2, 2)):
        assert ws(Bq, C, H, W, 3, n, 0) == plain * level and ws(Bq, C, H, W, 3, n, 1) == masked * level, n
        assert hb(Bq, C, H, W, 3, n) == 4 * L * max(n - 1, 0), n
        assert bws(Bq, C, H, W, 3, n, 0) == max(n - 1, 0) * level and bws(Bq, C, H, W, 3, n, 1) == (n if n else 0) * level, n
    for q in (ws, bws):
        for bad in ((0, C, H, W, 3, 4), (Bq, 0, H, W, 3, 4), (Bq, C, 0, W, 3, 4), (Bq, C, H, 0, 3, 4), (Bq, C, H, W, 5, 4), (Bq, C, H, W, 7, 4), (Bq, C, H, W, 3, -1),
                    (1, 1, 1 << 16, 1 << 15, 3, 4)):
            assert q(*bad, 1) == 0, bad
    assert hb(Bq, C, H, W, 5, 4) == 0 and hb(0, C, H, W, 3, 4) == 0 and hb(Bq, C, H, W, 3, -1) == 0


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    fw, bw, sm, sb = (_lib.symbol(s) for s in ("cspn2d_forward_nl_f32", "cspn2d_backward_nl_f32", "cspn2d_nl_sample_f32", "cspn2d_nl_sample_backward_f32"))
    a, o, x, s, out, h, w, go, ga, gd, gx, f, gf = (ctypes.c_void_p(i << 32) for i in range(1, 14))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    hb = 4 * 2 * 8 * 8 * 3
    shape = (2, 1, 8, 8)

    def fwd(a=a, o=o, x=x, s=s, out=out, h=None, hb=0, shape=shape, K=3, n=4, w=w, wb=M):
        return fw(a, o, x, s, out, h, hb, *shape, K, n, w, wb, None)

    def bwd(a=a, o=o, x=x, s=s, h=h, hb=hb, go=go, ga=ga, gd=gd, gx=gx, shape=shape, K=3, n=4, w=w, wb=M):
        return bw(a, o, x, s, h, hb, go, ga, gd, gx, *shape, K, n, w, wb, None)

    for call in (fwd, bwd):
        for kw in (dict(a=None), dict(o=None), dict(x=None)):
            assert call(**kw) == -1 and b"null" in err(), kw
        for bad in ((0, 1, 8, 8), (2, 0, 8, 8), (2, 1, 0, 8), (2, 1, 8, -1)):
            assert call(shape=bad) == -1 and b"shape" in err(), bad
        assert call(n=-1) == -1 and b"n_iter" in err()
        for K in (5, 7, 1, 4):
            assert call(K=K) == -3 and b"K" in err(), K
        for big in ((1, 1, 1 << 16, 1 << 15), (1, 40, 1 << 13, 1 << 13)):   # B 2KK H W, then B C H W alone, above 2^31 - 1
            assert call(shape=big) == -3 and b"too large" in err(), big
        assert call(wb=64) == -2 and b"workspace" in err()
        assert call(w=None) == -2 and b"workspace" in err()
        assert call(w=ctypes.c_void_p((7 << 32) + 16)) == -2 and b"aligned" in err()
    assert fwd(out=None) == -1 and b"null" in err()
    assert bwd(go=None) == -1 and b"null" in err()
    # a history that is too small; out, history or the workspace on an input or on each other
    assert fwd(h=h, hb=hb - 4) == -2 and b"history" in err()
    assert fwd(out=x) == -1 and b"alias" in err()
    assert fwd(out=s) == -1 and b"alias" in err()
    assert fwd(h=a, hb=hb) == -1 and b"alias" in err()
    assert fwd(h=out, hb=hb) == -1 and b"alias" in err()
    assert fwd(w=o) == -1 and b"alias" in err()
    assert fwd(w=out) == -1 and b"alias" in err()
    # the backward: grad_aff and grad_offset need the history where n_iter >= 2; grad_x does not
    assert bwd(h=None, hb=0) == -1 and b"history" in err()
    assert bwd(h=None, hb=0, ga=None) == -1 and b"history" in err()
    assert bwd(hb=hb - 4) == -1 and b"history" in err()
    assert bwd(ga=gx) == -1 and b"alias" in err()
    assert bwd(gd=ga) == -1 and b"alias" in err()
    assert bwd(gx=go) == -1 and b"alias" in err()
    assert bwd(ga=h) == -1 and b"alias" in err()
    assert bwd(w=ga) == -1 and b"alias" in err()
    assert bwd(ga=None, gd=None, gx=None) == 0   # nothing asked for: nothing to do
    # the sampling operator
    assert sm(None, f, out, 2, 8, 8, 3, None) == -1 and b"null" in err()
    assert sm(o, f, None, 2, 8, 8, 3, None) == -1 and b"null" in err()
    assert sm(o, f, out, 2, 8, 8, 5, None) == -3 and b"K" in err()
    assert sm(o, f, out, 2, 0, 8, 3, None) == -1 and b"shape" in err()
    assert sm(o, f, f, 2, 8, 8, 3, None) == -1 and b"alias" in err()
    assert sb(o, f, None, gf, gd, 2, 8, 8, 3, None) == -1 and b"null" in err()
    assert sb(o, f, go, gf, gd, 2, 8, 8, 7, None) == -3 and b"K" in err()
    assert sb(o, f, go, gf, gf, 2, 8, 8, 3, None) == -1 and b"alias" in err()
    assert sb(o, f, go, f, gd, 2, 8, 8, 3, None) == -1 and b"alias" in err()
    assert sb(o, f, go, None, None, 2, 8, 8, 3, None) == 0


def test_python_argument_errors_without_gpu():
    a, o, x, s, go = torch.rand(1, 8, 6, 9), torch.rand(1, 16, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9)
    f, gk = torch.rand(1, 1, 6, 9), torch.rand(1, 8, 6, 9)
    calls = {
        "forward": lambda a=a, o=o, x=x, s=s, n=3, **k: F.cspn2d_forward_nl(a, o, x, s, n, **k),
        "backward": lambda a=a, o=o, x=x, s=s, n=3, **k: F.cspn2d_backward_nl(a, o, x, s, go, n, **k),
    }
    for what, call in calls.items():
        for kw in (dict(a=torch.rand(1, 7, 6, 9)), dict(a=torch.rand(1, 24, 6, 9)), dict(o=torch.rand(1, 8, 6, 9)), dict(o=torch.rand(1, 18, 6, 9)),
                   dict(x=torch.rand(1, 2, 6, 8)), dict(x=torch.rand(2, 2, 6, 9)), dict(x=torch.rand(2, 6, 9))):
            with pytest.raises(ValueError):
                call(**kw)
        for K in (5, 7, 4, "3", True):
            with pytest.raises(ValueError, match="kernel_size"):
                call(kernel_size=K)
        for dt in (torch.float16, torch.bfloat16, torch.float64):
            for name in ("a", "o", "x", "s"):
                with pytest.raises(TypeError, match="float32"):
                    call(**{name: dict(a=a, o=o, x=x, s=s)[name].to(dt)})
        for bad in (torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 8), torch.rand(1, 6, 9)):
            with pytest.raises(ValueError, match="sparse_depth"):
                call(s=bad)
        with pytest.raises(ValueError, match="n_iter"):
            call(n=-1)
        with pytest.raises(cspn_amd.CspnError):   # a well-formed call on the CPU reaches the engine, which is GPU-only
            call()
        with pytest.raises(cspn_amd.CspnError):
            call(s=None)
    with pytest.raises(TypeError, match="float32"):
        F.cspn2d_backward_nl(a, o, x, s, go.double(), 3)
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_backward_nl(a, o, x, s, torch.rand(1, 3, 6, 9), 3)
    assert F.cspn2d_forward_nl(a, o, x, s, 0) is x and F.cspn2d_forward_nl(a, o, x, None, 0, return_history=True) == (x, None)
    # the sampling operator
    for call in (lambda **k: F.cspn2d_nl_sample(k.pop("o", o), k.pop("f", f), **k), lambda **k: F.cspn2d_nl_sample_backward(k.pop("o", o), k.pop("f", f), gk, **k)):
        with pytest.raises(ValueError):
            call(o=torch.rand(1, 8, 6, 9))
        with pytest.raises(ValueError, match="f "):
            call(f=torch.rand(1, 2, 6, 9))
        with pytest.raises(ValueError, match="kernel_size"):
            call(kernel_size=5)
        with pytest.raises(TypeError, match="float32"):
            call(f=f.half())
        with pytest.raises(TypeError, match="float32"):
            call(o=o.double())
        with pytest.raises(cspn_amd.CspnError):
            call()
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_nl_sample_backward(o, f, torch.rand(1, 16, 6, 9))
    # the module
    m = cspn_amd.NonLocal_Propagate(3)
    g = torch.rand(1, 8, 6, 9)
    for conf in (torch.rand(1, 6, 9), torch.rand(6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 8)):
        with pytest.raises(ValueError, match="confidence"):
            m(g, o, x, conf)
    with pytest.raises(ValueError, match="affinity"):
        m(torch.rand(1, 24, 6, 9), o, x)
    with pytest.raises(ValueError, match="offset"):
        m(g, torch.rand(1, 8, 6, 9), x)
    with pytest.raises(ValueError, match="n_iter"):
        m(g, o, x, n_iter=-1)
    with pytest.raises(TypeError, match="float32"):
        m(g, o, x.double())
    assert m(g, o, x, n_iter=0) is x and cspn_amd.NonLocal_Propagate(0)(g, o, x, f, s) is x
    with pytest.raises(cspn_amd.CspnError):
        m(g, o, x, None, s)


def test_module_constructor_repr_and_state():
    m = cspn_amd.NonLocal_Propagate(18)
    assert repr(m) == "NonLocal_Propagate(prop_time=18, prop_kernel=3, affinity='TGASS', affinity_gamma=0.5, preserve_input=True)"
    assert list(m.state_dict()) == ["scale"] and [n for n, _ in m.named_parameters()] == ["scale"]
    assert tuple(m.scale.shape) == (1,) and float(m.scale.detach()) == 0.5 * 8 and m.scale.requires_grad
    assert float(cspn_amd.NonLocal_Propagate(6, 3, "TGASS", 0.25).scale.detach()) == 2.0
    for mode in ("AS", "ASS", "TC"):
        m = cspn_amd.NonLocal_Propagate(6, 3, mode, preserve_input=False)
        assert m.state_dict() == {} and list(m.parameters()) == [] and list(m.buffers()) == []
        assert repr(m) == "NonLocal_Propagate(prop_time=6, prop_kernel=3, affinity=%r, affinity_gamma=0.5, preserve_input=False)" % mode
    for bad in (5, 7, 1):
        with pytest.raises(ValueError, match="prop_kernel"):
            cspn_amd.NonLocal_Propagate(6, bad)
    with pytest.raises(ValueError, match="affinity"):
        cspn_amd.NonLocal_Propagate(6, 3, "8sum")
    with pytest.raises(ValueError, match="prop_time"):
        cspn_amd.NonLocal_Propagate(-1)


@pytest.mark.parametrize("mode", MODES)
def test_the_four_normalisations_against_their_formulas(mode):
    gen = torch.Generator().manual_seed(3)
    g = (torch.randn(2, 8, 7, 11, generator=gen) * 0.2).double()
    m = cspn_amd.NonLocal_Propagate(3, 3, mode, GAMMA).double()
    got = m.normalize(g)
    S = g.abs().sum(1, keepdim=True)
    scale = m.scale.detach() if mode == "TGASS" else torch.tensor([GAMMA * 8], dtype=torch.float64)   # (a float32 parameter, widened)
    assert abs(float(scale) - GAMMA * 8) < 1e-7
    t = torch.tanh(g) / (scale + 1e-8)
    T = t.abs().sum(1, keepdim=True)
    want = {"AS": g / (S + 1e-4), "ASS": g / torch.clamp(S + 1e-4, min=1.0), "TC": torch.tanh(g) / 8, "TGASS": t / torch.clamp(T + 1e-4, min=1.0)}[mode]
    assert rel_err(got.detach().numpy(), want.numpy()) <= 1e-14
    assert rel_err(ref_normalize(mode, g, None, None, scale).numpy(), want.numpy()) <= 1e-14
    if mode in ("ASS", "TGASS"):   # both sides of the max are drawn
        pre = (T if mode == "TGASS" else S) + 1e-4
        assert int((pre > 1).sum()) >= 10 and int((pre < 1).sum()) >= 10


def test_the_grid_reaches_every_value_of_every_factor_at_every_shape():
    assert len(CASES) == 32 and len(set(CASES)) == 32
    for shape in SHAPES:
        rows = [c for c in CASES if c[:2] == shape]
        assert {c[4] for c in rows} == set(KINDS) and {c[3] for c in rows} == {False, True} and {c[2] for c in rows} == {1, 3}
        for kind in KINDS:
            assert {(c[2], c[3]) for c in rows if c[4] == kind} in ({(1, False), (3, True)}, {(3, False), (1, True)})
    for kind in KINDS:
        rows = [c for c in CASES if c[4] == kind]
        assert {(c[2], c[3]) for c in rows} == {(1, False), (1, True), (3, False), (3, True)}


def test_the_offset_kinds_are_what_they_say():
    for H, W in SHAPES:
        gen = torch.Generator().manual_seed(5)
        d = _offsets("integer", H, W, gen)
        assert torch.equal(d, d.round()) and float(d.abs().max()) >= 2
        d = _offsets("hot", H, W, gen).double()
        y = torch.arange(H).view(1, H, 1) + 0.0
        x = torch.arange(W).view(1, 1, W) + 0.0
        for k, (by, bx) in enumerate(bases(3)):   # exact in float32: every pixel and neighbour lands on the same point
            assert bool((y + by + d[:, 2 * k] == H // 2 + 0.25).all()) and bool((x + bx + d[:, 2 * k + 1] == W // 2 + 0.5).all())
        d = _offsets("huge", H, W, gen)
        frac = float((d.abs() == 1e9).float().mean())
        assert 0.1 < frac < 0.3 and bool((d == 1e9).any()) and bool((d == -1e9).any())
    for c in CASES:
        s = _inputs(*c, _seed(*c))[3]
        assert (s is None) == (not c[3]) and (s is None or (int((s > 0).sum()) >= 2 and float(s.max()) <= 5.1 and float(s[s > 0].min()) >= 0.1))


# =================================================================================================================================== GPU
def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _pinned(level, s):
    return level if s is None else torch.where(s > 0, s, level)


@functools.lru_cache(maxsize=None)
def _case(H, W, C, sparse, kind, n=N_ITER):
    """inputs (each drawn and placed on the device on its own), the float64 statement with its autograd gradients, the engine's results: made once"""
    aff, off, x, s, go = _inputs(H, W, C, sparse, kind, _seed(H, W, C, sparse, kind))
    leaves = [t.double().requires_grad_(True) for t in (aff, off, x)]
    levels = nl_levels(*leaves, None if s is None else s.double(), n)
    if n:
        levels[-1].backward(go.double())
    dev = _cuda(aff, off, x, s, go)
    ad, od, xd, sd, god = dev
    out, hist = F.cspn2d_forward_nl(ad, od, xd, sd, n, return_history=True)
    grads = F.cspn2d_backward_nl(ad, od, xd, sd, god, n, history=hist)
    return dict(dev=dev, levels=[t.detach() for t in levels], ref_grads=[t.grad for t in leaves], out=out, hist=hist, grads=grads, sparse=s)


NAMES = ("grad_aff", "grad_offset", "grad_x")


def _grads_close(got, want, names=NAMES):
    for a, b, what in zip(got, want, names):
        a, b = _np64(a), _np64(b)
        print("%s: max |engine - statement| / max |statement| = %.3e" % (what, np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)))
        assert _check(a, b, what)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,sparse,kind", CASES)
def test_forward_and_every_gradient_vs_fp64_statement(H, W, C, sparse, kind):
    c = _case(H, W, C, sparse, kind)
    ref = c["levels"][-1]
    assert bool(torch.isfinite(ref).all())
    e = rel_err(c["out"].cpu().numpy(), ref.numpy())
    print("forward rel_err %.3e" % e)
    assert e <= RTOL
    ad, od, xd, sd, god = c["dev"]
    assert torch.equal(F.cspn2d_forward_nl(ad, od, xd, sd, N_ITER), c["out"])   # through the ping-pong levels: the same bits
    hist = c["hist"].view(N_ITER - 1, B, C, H, W).cpu()
    for t in range(1, N_ITER):   # the kept levels are the statement's, pinned as the next step reads them
        want = _pinned(c["levels"][t], None if c["sparse"] is None else c["sparse"].double())
        assert rel_err(hist[t - 1].numpy(), want.numpy()) <= RTOL, t
    _grads_close(c["grads"], c["ref_grads"])
    if sparse:   # a pinned pixel passes no gradient to x
        assert bool((c["grads"][2].cpu()[(c["sparse"] > 0).expand(B, C, H, W)] == 0).all())
    _grads_close(F.cspn2d_backward_nl(ad, od, xd, sd, god, N_ITER), c["ref_grads"])   # without a kept history: runs its own forward


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("sparse", [False, True])
def test_the_edges_of_the_history_and_workspace_queries_and_every_gradient_subset(n, sparse):
    H, W, C, kind = 17, 65, 3, "normal"
    c = _case(H, W, C, sparse, kind, n)
    ad, od, xd, sd, god = c["dev"]
    if n == 0:
        assert F.cspn2d_forward_nl(ad, od, xd, sd, 0) is xd and c["hist"] is None
        ga, gd, gx = c["grads"]
        assert torch.equal(gx, god) and not bool(ga.any()) and not bool(gd.any())
        return
    assert rel_err(c["out"].cpu().numpy(), c["levels"][-1].numpy()) <= RTOL
    assert torch.equal(F.cspn2d_forward_nl(ad, od, xd, sd, n), c["out"])
    assert (c["hist"].numel() == (n - 1) * B * C * H * W) if n >= 2 else (c["hist"].numel() == 1)
    _grads_close(c["grads"], c["ref_grads"])
    for need in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):
        for history in (None, c["hist"]):
            got = F.cspn2d_backward_nl(ad, od, xd, sd, god, n, 3, history, *map(bool, need))
            assert [g is not None for g in got] == list(map(bool, need))
            _grads_close([g for g in got if g is not None], [r for r, k in zip(c["ref_grads"], need) if k], [w for w, k in zip(NAMES, need) if k])
    assert F.cspn2d_backward_nl(ad, od, xd, sd, god, n, 3, None, False, False, False) == (None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,sparse,kind", [CASES[3], CASES[12], CASES[21], CASES[30]])
def test_the_forward_twice_gives_identical_bits_and_the_backward_twice_agrees(H, W, C, sparse, kind):
    """The forward gathers and writes each element once: run-to-run bitwise.  The backward is NOT required to be: its adjoint is a scatter with float
    atomics, and a float sum depends on the order its terms arrive in; two runs agree within the bound that ties either of them to the statement."""
    c = _case(H, W, C, sparse, kind)
    ad, od, xd, sd, god = c["dev"]
    out, hist = F.cspn2d_forward_nl(ad, od, xd, sd, N_ITER, return_history=True)
    assert memguard.same_bits(out, c["out"]) and memguard.same_bits(hist, c["hist"])
    again = F.cspn2d_backward_nl(ad, od, xd, sd, god, N_ITER, history=hist)
    _grads_close(again, c["grads"])
    _grads_close(again, c["ref_grads"])


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(16, 64), (33, 132), (17, 65)])
@pytest.mark.parametrize("sparse", [False, True])
def test_misaligned_views_and_an_odd_width(H, W, sparse):
    """views one element off a 16-byte boundary (and, at 17 x 65, a width that is no multiple of 4) take the guarded scalar forward kernels: the forward's
    bits are those of the aligned call, the backward agrees within _check (it is not bitwise even against itself)"""
    C = 3
    c = _case(H, W, C, sparse, "normal")
    tensors = [t.cpu() if t is not None else None for t in c["dev"]]

    def run(ad, od, xd, sd, god):
        out, hist = F.cspn2d_forward_nl(ad, od, xd, sd, N_ITER, return_history=True)
        return (out, hist, F.cspn2d_forward_nl(ad, od, xd, sd, N_ITER)), F.cspn2d_backward_nl(ad, od, xd, sd, god, N_ITER, history=hist)
    off = [None if t is None else _misaligned(t.cuda()) for t in tensors]
    assert all(t is None or t.storage_offset() == 1 for t in off)
    variants = [off] + [[(_misaligned(t.cuda()) if j == i else t.cuda()) if t is not None else None for j, t in enumerate(tensors)] for i in range(5)]
    for v in variants:   # all five off their boundary, then each alone: every VEC condition on its own
        fwd, bwd = run(*v)
        memguard.assert_same_outputs(fwd, (c["out"], c["hist"], c["out"]), "misaligned")
        _grads_close(bwd, c["grads"])
        _grads_close(bwd, c["ref_grads"])


@functools.lru_cache(maxsize=None)
def _sample_case(H, W, kind):
    gen = torch.Generator().manual_seed(300 + W + KINDS.index(kind))
    off = _offsets(kind, H, W, gen)
    f = torch.rand(B, 1, H, W, generator=gen) * 2 - 0.5
    go = torch.randn(B, 8, H, W, generator=gen)
    leaves = [t.double().requires_grad_(True) for t in (off, f)]
    ref = sample_all(*leaves)
    ref.backward(go.double())
    return _cuda(off, f, go), ref.detach(), [t.grad for t in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sampling_operator_vs_bil(H, W, kind):
    (od, fd, god), ref, (rgo, rgf) = _sample_case(H, W, kind)
    out = F.cspn2d_nl_sample(od, fd)
    assert rel_err(out.cpu().numpy(), ref.numpy()) <= RTOL
    assert memguard.same_bits(F.cspn2d_nl_sample(od, fd), out)
    gf, gd = F.cspn2d_nl_sample_backward(od, fd, god)
    _grads_close((gf, gd), (rgf, rgo), ("grad_f", "grad_offset"))
    gf2, none = F.cspn2d_nl_sample_backward(od, fd, god, need_offset=False)
    none2, gd2 = F.cspn2d_nl_sample_backward(od, fd, god, need_f=False)
    assert none is None and none2 is None and memguard.same_bits(gd2, gd)   # grad_offset is written once: bitwise
    _grads_close((gf2,), (rgf,), ("grad_f",))
    for t in (od, fd, god):   # a view one element off its boundary: the same kernels (one pixel per lane), the same forward bits
        args = [_misaligned(u) if u is t else u for u in (od, fd, god)]
        assert memguard.same_bits(F.cspn2d_nl_sample(args[0], args[1]), out)
        _grads_close(F.cspn2d_nl_sample_backward(*args), (rgf, rgo), ("grad_f", "grad_offset"))


# ---- the module against float64 autograd through the statement and the normalisation formulas ----
def _module_inputs(H, W, C, seed):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(B, 8, H, W, generator=gen) * 0.2
    off = torch.randn(B, 16, H, W, generator=gen) * 1.5
    x = torch.rand(B, C, H, W, generator=gen) * 9.9 + 0.1
    conf = torch.rand(B, 1, H, W, generator=gen)
    s = (torch.rand(B, 1, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, H, W, generator=gen) * 5 + 0.1)
    go = torch.randn(B, C, H, W, generator=gen)
    return g, off, x, conf, s, go


def _module_ref(mode, g, off, x, conf, s, go, use_conf, preserve, n, gamma=GAMMA):
    leaves = [t.double().requires_grad_(True) for t in (g, off, x, conf)]
    scale = torch.full((1,), gamma * 8, dtype=torch.float64, requires_grad=True)
    aff = ref_normalize(mode, leaves[0], leaves[1], leaves[3] if use_conf else None, scale)
    out = nl_levels(aff, leaves[1], leaves[2], s.double() if preserve else None, n)[-1]
    out.backward(go.double())
    grads = [t.grad for t in leaves]
    return out.detach(), grads[:3] + ([grads[3]] if use_conf else []) + ([scale.grad] if mode == "TGASS" else [])


def _module_run(mode, g, off, x, conf, s, go, use_conf, preserve, n):
    m = cspn_amd.NonLocal_Propagate(n, 3, mode, GAMMA, preserve).cuda()
    leaves = [hygiene._leaf(t) for t in (g, off, x, conf)]
    y = m(leaves[0], leaves[1], leaves[2], leaves[3] if use_conf else None, s)
    y.backward(go)
    return y.detach(), [t.grad for t in leaves[:3]] + ([leaves[3].grad] if use_conf else []) + ([m.scale.grad] if mode == "TGASS" else [])


MODULE_NAMES = ("dL/daffinity", "dL/doffset", "dL/dfeat", "dL/dconfidence or dL/dscale", "dL/dscale")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_conf", [False, True])
@pytest.mark.parametrize("preserve", [False, True])
def test_module_vs_fp64_autograd(mode, use_conf, preserve):
    H, W, C = ((17, 65), (33, 132))[MODES.index(mode) % 2 ^ int(use_conf)] + (2,)
    cpu = _module_inputs(H, W, C, 40 + MODES.index(mode))
    ref, ref_grads = _module_ref(mode, *cpu, use_conf, preserve, N_ITER)
    y, grads = _module_run(mode, *_cuda(*cpu), use_conf, preserve, N_ITER)
    assert rel_err(y.cpu().numpy(), ref.numpy()) <= RTOL
    assert len(grads) == len(ref_grads) == 3 + int(use_conf) + int(mode == "TGASS") and all(g is not None for g in grads)
    _grads_close(grads, ref_grads, MODULE_NAMES)
    if not use_conf:   # a confidence that is not given gets no gradient, and the mask is the sparse_depth's where it is preserved
        with torch.no_grad():
            m = cspn_amd.NonLocal_Propagate(N_ITER, 3, mode, GAMMA, preserve).cuda()
            g, off, x, conf, s, go = _cuda(*cpu)
            assert memguard.same_bits(m(g, off, x, None, s), y)                      # without autograd: the same engine calls, the same bits
            assert memguard.same_bits(m(g, off, x, None, s if preserve else None), y)  # preserve_input=False ignores the sparse_depth


# ---- memory hygiene: every new function and the module between guard bands on NaN and on finite poison, and in a stale arena.  Forward outputs are
# compared bitwise with the clean run; backward outputs with the float64 statement (they are not bitwise from run to run) ----
N_FWD = 4   # out, out (with a history), the history, the sampled confidence: bitwise; everything behind them: gradients


def _hygiene_inputs(H, W, C, sparse, kind, seed):
    aff, off, x, s, go = _inputs(H, W, C, sparse, kind, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    f = torch.rand(B, 1, H, W, generator=gen)
    gk = torch.randn(B, 8, H, W, generator=gen)
    return tuple(_cuda(aff, off, x, s, go, f, gk))


def _hygiene_call(aff, off, x, s, go, f, gk):
    n = N_ITER
    out = F.cspn2d_forward_nl(aff, off, x, s, n)
    out2, hist = F.cspn2d_forward_nl(aff, off, x, s, n, return_history=True)
    smp = F.cspn2d_nl_sample(off, f)
    grads = F.cspn2d_backward_nl(aff, off, x, s, go, n, history=hist)
    alone = F.cspn2d_backward_nl(aff, off, x, s, go, n, 3, None, False, True, False)[1:2]   # runs its own forward; no grad_x: the sweep stops at A_1
    one = F.cspn2d_backward_nl(aff, off, x, s, go, 1)                                       # one step: no history, the workspace is the pinned H_0 alone
    sg = F.cspn2d_nl_sample_backward(off, f, gk)
    return (out, out2, hist, smp) + tuple(grads) + tuple(alone) + tuple(one) + tuple(sg)


@functools.lru_cache(maxsize=None)
def _hygiene_ref(name):
    aff, off, x, s, go, f, gk = (None if t is None else t.cpu().double() for t in HYGIENE[name].build())

    def grads(n):
        leaves = [t.clone().requires_grad_(True) for t in (aff, off, x)]
        nl_levels(*leaves, s, n)[-1].backward(go)
        return [t.grad for t in leaves]
    full, one = grads(N_ITER), grads(1)
    leaves = [t.clone().requires_grad_(True) for t in (off, f)]
    sample_all(*leaves).backward(gk)
    return full + full[1:2] + one + [leaves[1].grad, leaves[0].grad]


def _module_hygiene_inputs(H, W):
    return tuple(_cuda(*_module_inputs(H, W, 2, 77 + W)))


def _module_hygiene_call(g, off, x, conf, s, go):
    """both affinity modes with state or a kink, with a confidence and a preserved input"""
    outs, grads = [], []
    for mode in ("TGASS", "AS"):
        y, gr = _module_run(mode, g, off, x, conf, s, go, True, True, N_ITER)
        outs.append(y)
        grads += gr
    return tuple(outs) + (None, None) + tuple(grads)   # (two forward outputs; padded to N_FWD)


@functools.lru_cache(maxsize=None)
def _module_hygiene_ref(name):
    cpu = [t.cpu() for t in HYGIENE[name].build()]
    return sum((_module_ref(mode, *cpu, True, True, N_ITER)[1] for mode in ("TGASS", "AS")), [])


HYGIENE, HYGIENE_REF = {}, {}
for _H, _W, _C, _sp, _kind in ((17, 65, 3, True, "normal"), (33, 132, 1, True, "huge"), (33, 132, 3, False, "integer"), (16, 64, 1, True, "hot")):
    _name = "nl-%dx%d-C%d-%s-%s" % (_H, _W, _C, "masked" if _sp else "plain", _kind)
    HYGIENE[_name] = hygiene.Case(_name, tuple(FUNCS), "the non-local entry points", 4 * B * max(_C, 16) * _H * _W,
                                  functools.lru_cache(maxsize=None)(functools.partial(_hygiene_inputs, _H, _W, _C, _sp, _kind, 900 + _W + _C)),
                                  _hygiene_call, lambda: None, "test_nl.py::test_forward_and_every_gradient_vs_fp64_statement", False, None, None)
    HYGIENE_REF[_name] = _hygiene_ref
for _H, _W in ((17, 65), (33, 132)):
    _name = "nl-module-%dx%d" % (_H, _W)
    HYGIENE[_name] = hygiene.Case(_name, ("NonLocal_Propagate",), "the module with a confidence and a preserved input", 4 * B * 16 * _H * _W,
                                  functools.lru_cache(maxsize=None)(functools.partial(_module_hygiene_inputs, _H, _W)), _module_hygiene_call,
                                  lambda: None, "test_nl.py::test_module_vs_fp64_autograd", False, None, None)
    HYGIENE_REF[_name] = _module_hygiene_ref
_CLEAN = {}


def test_the_guarded_cases_stay_out_of_the_shared_table():
    assert not set(HYGIENE) & set(hygiene.CASES) and {c.plane > 0 for c in HYGIENE.values()} == {True} and set(HYGIENE) == set(HYGIENE_REF)
    shared = {n for c in hygiene.CASES.values() for n in c.covers}
    assert not shared & (set(FUNCS) | {"NonLocal_Propagate"})
    assert {n for c in HYGIENE.values() for n in c.covers} == set(FUNCS) | {"NonLocal_Propagate"}
    # the module reaches the engine through cspn_amd.functional alone, so memguard's patch of that module's names covers its buffers
    src = inspect.getsource(nlspn)
    for alloc in ("torch.empty", "torch.zeros", ".new_empty", ".new_zeros", "_workspace"):
        assert alloc not in src, alloc


def _clean_forward(name):
    """the forward outputs of the clean (unpatched) run, made once per case; made twice first: the forward's claim of run-to-run bitwise results"""
    if name not in _CLEAN:
        c = HYGIENE[name]
        a, b = c.call(*c.build()), c.call(*c.build())
        torch.cuda.synchronize()
        memguard.assert_same_outputs(b[:N_FWD], a[:N_FWD], "second clean run")
        _CLEAN[name] = a[:N_FWD]
    return _CLEAN[name]


def _assert_outputs(name, outs, what):
    for o in outs:
        assert o is None or bool(torch.isfinite(o.float()).all()), "%s: poison reached an output" % what
    memguard.assert_same_outputs(outs[:N_FWD], _clean_forward(name), what)
    want = HYGIENE_REF[name](name)
    assert len(outs) - N_FWD == len(want)
    for i, (a, b) in enumerate(zip(outs[N_FWD:], want)):
        assert _check(_np64(a), _np64(b), "%s: gradient %d" % (what, i))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_every_call_between_guard_bands(name, poison):
    """every output, history and workspace lies between guard bands and is poisoned before the call: intact bands, unchanged inputs, forward outputs
    bitwise the unguarded run's (so fully written), gradients the float64 statement's (a poisoned adjoint level that the scatter added into, instead
    of one the memset had zeroed first, would show here)"""
    c = HYGIENE[name]
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, c.call, c.build(), "cuda", c.plane)
    assert len(session.workspaces) >= 3 and len(session.guards) > len(session.workspaces)
    _assert_outputs(name, outs, "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    """the calls of every shape and the module through ONE workspace arena, sized to the largest request and never refilled: each call finds what the
    calls before it left, and still returns the clean forward bits and the statement's gradients"""
    order = ["nl-33x132-C3-plain-integer", "nl-33x132-C1-masked-huge", "nl-module-33x132", "nl-17x65-C3-masked-normal", "nl-16x64-C1-masked-hot",
             "nl-module-17x65", "nl-33x132-C3-plain-integer"]
    plane = 4 * B * 16 * 33 * 132
    with contextlib.ExitStack() as stack:   # guarded first: this pass has the sizes
        session = memguard.patched(stack, "zero", plane_bytes=plane)
        for name in order:
            HYGIENE[name].call(*HYGIENE[name].build())
            session.check()
        sizes = [n for _, n in session.workspaces]
    assert sizes and max(sizes) > 0
    arena = memguard.Arena(max(sizes), "cuda", plane)
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "stale", arena=arena, plane_bytes=plane)
        for i, name in enumerate(order):
            inputs = HYGIENE[name].build()
            snap = memguard.snapshot(*inputs)
            outs = HYGIENE[name].call(*inputs)
            session.check()
            snap.assert_unchanged()
            _assert_outputs(name, outs, "step %d (%s) in the stale arena" % (i + 1, name))
    assert arena.taken > 0
