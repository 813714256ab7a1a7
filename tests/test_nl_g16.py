"""fp16 / bf16 affinities and offsets in non-local propagation (the six cspn2d_*_nl*_g16 entry points, the six cspn_amd.functional.*_g16
functions, and NonLocal_Propagate under torch.autocast).

The float32 side of every comparison is code that exists without this feature: cspn2d_forward_nl, cspn2d_backward_nl_det, cspn2d_nl_sample and
cspn2d_nl_sample_backward_det on aff.float(), offset.float(), and test_nl's float64 statement on the same widened tensors.  A 16-bit value is
widened exactly where the kernels read it, so
    the forward, the history and the sampling operator        bitwise the float32 function on the widened tensors
    the deterministic backwards                               grad_x / grad_f bitwise; grad_aff / grad_offset bitwise the float32 result's .to(dtype)
    the scatter backwards                                     within test_backward._check of the float64 statement, plus one rounding of the
                                                              statement's value for the 16-bit gradients
That rounding (round to nearest): |fl(v) - v| <= 2^-11 |v| for fp16 normals and 2^-8 |v| for bf16 (11 and 8 significant bits), and <= 2^-25 for fp16
subnormals (their spacing is 2^-24).  It is derived from the formats, not from what the engine gives."""
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
import test_nl
import test_nl_det
from cspn_amd import _lib
from cspn_amd import functional as F
from cspn_amd import nlspn
from test_backward import GFLOOR, GTOL, _check
from test_kxk_norm import _cuda
from test_nl import B, CASES, KINDS, MODES, N_ITER, SHAPES, _inputs, _seed, nl_levels, sample_all

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_forward_nl_g16", "cspn2d_backward_nl_g16", "cspn2d_backward_nl_det_g16", "cspn2d_nl_sample_g16", "cspn2d_nl_sample_backward_g16",
       "cspn2d_nl_sample_backward_det_g16"]
TWINS = ["cspn2d_forward_nl", "cspn2d_backward_nl", "cspn2d_backward_nl_det", "cspn2d_nl_sample", "cspn2d_nl_sample_backward", "cspn2d_nl_sample_backward_det"]
DTYPES = [torch.float16, torch.bfloat16]
PAIRS = ["0T", "TT"]          # (float32 aff, T offset): what the module produces; (T, T): callers that normalise in 16 bits themselves
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
TINY = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0, torch.float32: 0.0}
NAMES = test_nl.NAMES
THIN = [CASES[3], CASES[12], CASES[21], CASES[30]]   # test_nl_det's thinning: every shape once


def _id(v):
    return {torch.float16: "fp16", torch.bfloat16: "bf16"}.get(v, None)


# =================================================================================================================================== CPU
def test_symbols_and_surface():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text)
        assert m, "not declared: " + s
        assert "int K" in m.group(1) and "int offset_dtype" in m.group(1), s
        assert ("int aff_dtype" in m.group(1)) == ("sample" not in s), s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert len(cspn_amd.__all__) == 36 and not any(n.endswith("_g16") and "nl" in n for n in cspn_amd.__all__)
    for new, twin in zip(NEW, TWINS):
        assert callable(getattr(F, new)) and not hasattr(cspn_amd, new)
        assert str(inspect.signature(getattr(F, new))) == str(inspect.signature(getattr(F, twin))), new
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    assert sig(nlspn.nl_propagate) == "aff offset x sparse_depth n_iter kernel_size deterministic".split()
    assert sig(nlspn.nl_sample) == "offset f kernel_size deterministic".split()
    assert sig(nlspn.NonLocal_Propagate.forward) == "self affinity offset feat confidence sparse_depth n_iter".split()
    assert sig(nlspn.NonLocal_Propagate.__init__) == "self prop_time prop_kernel affinity affinity_gamma preserve_input".split()
    assert sig(nlspn.NonLocal_Propagate.normalize) == "self affinity offset confidence".split()


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    fw, bw, bd, sm, sb, sd = (_lib.symbol(s) for s in NEW)
    a, o, x, s, out, h, w, go, ga, gd, gx, f, gf = (ctypes.c_void_p(i << 32) for i in range(1, 14))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    hb = 4 * 2 * 8 * 8 * 3
    shape = (2, 1, 8, 8)

    def fwd(a=a, o=o, x=x, s=s, out=out, h=None, hb=0, shape=shape, K=3, n=4, w=w, wb=M, adt=1, odt=1):
        return fw(a, adt, o, odt, x, s, out, h, hb, *shape, K, n, w, wb, None)

    def back(entry):
        def bwd(a=a, o=o, x=x, s=s, h=h, hb=hb, go=go, ga=ga, gd=gd, gx=gx, shape=shape, K=3, n=4, w=w, wb=M, adt=1, odt=1):
            return entry(a, adt, o, odt, x, s, h, hb, go, ga, gd, gx, *shape, K, n, w, wb, None)
        return bwd

    bwd, det = back(bw), back(bd)
    for call in (fwd, bwd, det):   # every rule of the twins, on fake pointers
        for kw in (dict(a=None), dict(o=None), dict(x=None)):
            assert call(**kw) == -1 and b"null" in err(), kw
        for bad in ((0, 1, 8, 8), (2, 0, 8, 8), (2, 1, 0, 8), (2, 1, 8, -1)):
            assert call(shape=bad) == -1 and b"shape" in err(), bad
        assert call(n=-1) == -1 and b"n_iter" in err()
        for K in (5, 7, 1, 4):
            assert call(K=K) == -3 and b"K" in err(), K
        for big in ((1, 1, 1 << 16, 1 << 15), (1, 40, 1 << 13, 1 << 13)):
            assert call(shape=big) == -3 and b"too large" in err(), big
        assert call(wb=64) == -2 and b"workspace" in err()
        assert call(w=None) == -2 and b"workspace" in err()
        assert call(w=ctypes.c_void_p((7 << 32) + 16)) == -2 and b"aligned" in err()
        # the dtype checks: a code outside {0, 1, 2}; the pairs that are not built; the three that are
        for kw in (dict(adt=3), dict(odt=3), dict(adt=-1), dict(odt=-1), dict(adt=3, odt=0)):
            assert call(**kw) == -1 and b"dtype" in err(), kw
        for pair in ((1, 0), (2, 0), (1, 2), (2, 1)):
            assert call(adt=pair[0], odt=pair[1]) == -3 and b"dtype" in err(), pair
        # ... and they come last: an earlier rule wins over a bad dtype
        assert call(adt=3, K=5) == -3 and b"K" in err()
        assert call(adt=1, odt=0, wb=64) == -2 and b"workspace" in err()
        assert call(adt=3, w=o) == -1 and b"alias" in err()
    assert fwd(out=None) == -1 and b"null" in err()
    assert bwd(go=None) == -1 and b"null" in err() and det(go=None) == -1 and b"null" in err()
    assert fwd(h=h, hb=hb - 4) == -2 and b"history" in err()
    for kw in (dict(out=x), dict(out=s), dict(h=a, hb=hb), dict(h=out, hb=hb), dict(w=o), dict(w=out)):
        assert fwd(**kw) == -1 and b"alias" in err(), kw
    for call in (bwd, det):
        assert call(h=None, hb=0) == -1 and b"history" in err()
        assert call(h=None, hb=0, ga=None) == -1 and b"history" in err()
        assert call(hb=hb - 4) == -1 and b"history" in err()
        for kw in (dict(ga=gx), dict(gd=ga), dict(gx=go), dict(ga=h), dict(w=ga)):
            assert call(**kw) == -1 and b"alias" in err(), kw
        # the pairs that are built pass every check (nothing asked for: nothing is launched)
        for pair in ((0, 0), (0, 1), (0, 2), (1, 1), (2, 2)):
            assert call(adt=pair[0], odt=pair[1], ga=None, gd=None, gx=None) == 0, pair
        # aliasing is counted in the stored element size: offset holds 2 * 16 * 8 * 8 elements
        n_off = 2 * 16 * 8 * 8
        # a grad_offset in the second half of what would be the float32 extent of offset is no alias of a 16-bit offset.  It is put at an odd
        # address there, so that the call ends at the last check of all (16-bit tensors at even addresses) instead of reaching the device
        half = ctypes.c_void_p(o.value + 2 * n_off + 1)
        inside = ctypes.c_void_p(o.value + 2 * n_off - 2)
        assert call(gd=half, adt=0, odt=1, ga=None, gx=None) == -1 and b"2-byte" in err()
        assert call(gd=half, adt=0, odt=0, ga=None, gx=None) == -1 and b"alias" in err()
        assert call(gd=inside, adt=0, odt=1, ga=None, gx=None) == -1 and b"alias" in err()
    # the same for the forward: out right behind a 16-bit aff is no alias, inside a float32 one it is
    n_aff = 2 * 8 * 8 * 8
    assert fwd(out=ctypes.c_void_p(a.value + 4 * n_aff - 256), adt=0, odt=1) == -1 and b"alias" in err()
    assert fwd(out=ctypes.c_void_p(a.value + 2 * n_aff - 2), adt=1, odt=1) == -1 and b"alias" in err()
    assert fwd(out=ctypes.c_void_p(a.value + 1), adt=1, odt=1) == -1 and b"alias" in err()
    # 16-bit tensors at odd addresses
    odd = ctypes.c_void_p(o.value + 1)
    assert bwd(o=odd, ga=None, gd=None, gx=None) == -1 and b"2-byte" in err()
    assert bwd(o=odd, adt=0, odt=0, ga=None, gd=None, gx=None) == 0   # (the float32 pair makes no such check, as its twin)

    # the sampling operator and its two backwards
    def smp(o=o, f=f, out=out, shape=(2, 8, 8), K=3, odt=1):
        return sm(o, odt, f, out, *shape, K, None)

    def sbk(o=o, f=f, go=go, gf=gf, gd=gd, shape=(2, 8, 8), K=3, odt=1):
        return sb(o, odt, f, go, gf, gd, *shape, K, None)

    def sdt(o=o, f=f, go=go, gf=gf, gd=gd, shape=(2, 8, 8), K=3, odt=1, w=w, wb=M):
        return sd(o, odt, f, go, gf, gd, *shape, K, w, wb, None)

    for call in (smp, sbk, sdt):
        for kw in (dict(o=None), dict(f=None)):
            assert call(**kw) == -1 and b"null" in err(), kw
        for bad in ((0, 8, 8), (2, 0, 8), (2, 8, -1)):
            assert call(shape=bad) == -1 and b"shape" in err(), bad
        for K in (5, 7, 1):
            assert call(K=K) == -3 and b"K" in err(), K
        assert call(shape=(1, 1 << 16, 1 << 15)) == -3 and b"too large" in err()
        for odt in (3, -1):
            assert call(odt=odt) == -1 and b"dtype" in err(), odt
        assert call(odt=3, K=5) == -3 and b"K" in err()
    assert smp(out=None) == -1 and b"null" in err()
    assert smp(out=f) == -1 and b"alias" in err()
    assert smp(out=ctypes.c_void_p(o.value + 2 * n_off - 2)) == -1 and b"alias" in err()
    for call in (sbk, sdt):
        assert call(go=None) == -1 and b"null" in err()
        for kw in (dict(gd=gf), dict(gf=f), dict(gd=go), dict(gd=inside)):
            assert call(**kw) == -1 and b"alias" in err(), kw
        assert call(gd=half, gf=None) == -1 and b"2-byte" in err()
        assert call(gd=half, gf=None, odt=0) == -1 and b"alias" in err()
        for odt in (0, 1, 2):
            assert call(gf=None, gd=None, odt=odt) == 0
    assert sdt(wb=64) == -2 and b"workspace" in err()
    assert sdt(w=None) == -2 and b"workspace" in err()
    assert sdt(w=gd) == -1 and b"alias" in err()
    need = _lib.symbol("cspn2d_nl_sample_backward_det_workspace_bytes")(2, 8, 8, 3)
    assert sdt(wb=need - 1) == -2 and b"workspace" in err()
    need = _lib.symbol("cspn2d_backward_nl_det_workspace_bytes")(*shape, 3, 4, 1)
    assert det(wb=need - 1) == -2 and b"workspace" in err()


def test_python_argument_errors_without_gpu():
    a, o, x, s, go = torch.rand(1, 8, 6, 9), torch.rand(1, 16, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9)
    f, gk = torch.rand(1, 1, 6, 9), torch.rand(1, 8, 6, 9)
    h, bf = torch.float16, torch.bfloat16
    calls = {
        "forward": lambda a=a, o=o, x=x, s=s, n=3, **k: F.cspn2d_forward_nl_g16(a, o, x, s, n, **k),
        "backward": lambda a=a, o=o, x=x, s=s, n=3, **k: F.cspn2d_backward_nl_g16(a, o, x, s, go, n, **k),
        "det": lambda a=a, o=o, x=x, s=s, n=3, **k: F.cspn2d_backward_nl_det_g16(a, o, x, s, go, n, **k),
    }
    for what, call in calls.items():
        for kw in (dict(a=torch.rand(1, 7, 6, 9)), dict(a=torch.rand(1, 24, 6, 9)), dict(o=torch.rand(1, 8, 6, 9)), dict(o=torch.rand(1, 18, 6, 9)),
                   dict(x=torch.rand(1, 2, 6, 8)), dict(x=torch.rand(2, 2, 6, 9)), dict(x=torch.rand(2, 6, 9)), dict(o=torch.rand(1, 18, 6, 9).half())):
            with pytest.raises(ValueError):
                call(**kw)
        for K in (5, 7, 4, "3", True):
            with pytest.raises(ValueError, match="kernel_size"):
                call(kernel_size=K)
        # the pairs that are not built, and float64 anywhere
        for da, do in ((h, torch.float32), (bf, torch.float32), (h, bf), (bf, h)):
            with pytest.raises(TypeError, match="not built"):
                call(a=a.to(da), o=o.to(do))
        for kw in (dict(a=a.double()), dict(o=o.double()), dict(a=a.double(), o=o.double())):
            with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
                call(**kw)
        for dt in (h, bf, torch.float64):   # everything but aff and offset is float32
            for name in ("x", "s"):
                with pytest.raises(TypeError, match="float32"):
                    call(**{name: dict(x=x, s=s)[name].to(dt)})
        for bad in (torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 8), torch.rand(1, 6, 9)):
            with pytest.raises(ValueError, match="sparse_depth"):
                call(s=bad)
        with pytest.raises(ValueError, match="n_iter"):
            call(n=-1)
        # a well-formed call on the CPU reaches the engine, which is GPU-only: every pair that is built
        for da, do in ((torch.float32, torch.float32), (torch.float32, h), (torch.float32, bf), (h, h), (bf, bf)):
            with pytest.raises(cspn_amd.CspnError):
                call(a=a.to(da), o=o.to(do))
        with pytest.raises(cspn_amd.CspnError):
            call(o=o.half(), s=None)
    for fn in (F.cspn2d_backward_nl_g16, F.cspn2d_backward_nl_det_g16):
        with pytest.raises(TypeError, match="float32"):
            fn(a, o.half(), x, s, go.half(), 3)
        with pytest.raises(ValueError, match="grad_out"):
            fn(a, o.half(), x, s, torch.rand(1, 3, 6, 9), 3)
    assert F.cspn2d_forward_nl_g16(a.half(), o.half(), x, s, 0) is x and F.cspn2d_forward_nl_g16(a, o.half(), x, None, 0, return_history=True) == (x, None)
    samplers = (lambda **k: F.cspn2d_nl_sample_g16(k.pop("o", o.half()), k.pop("f", f), **k),
                lambda **k: F.cspn2d_nl_sample_backward_g16(k.pop("o", o.half()), k.pop("f", f), gk, **k),
                lambda **k: F.cspn2d_nl_sample_backward_det_g16(k.pop("o", o.half()), k.pop("f", f), gk, **k))
    for call in samplers:
        with pytest.raises(ValueError):
            call(o=torch.rand(1, 8, 6, 9).half())
        with pytest.raises(ValueError, match="f "):
            call(f=torch.rand(1, 2, 6, 9))
        with pytest.raises(ValueError, match="kernel_size"):
            call(kernel_size=5)
        with pytest.raises(TypeError, match="float32"):
            call(f=f.half())
        with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
            call(o=o.double())
        for dt in (torch.float32, h, bf):
            with pytest.raises(cspn_amd.CspnError):
                call(o=o.to(dt))
    for fn in (F.cspn2d_nl_sample_backward_g16, F.cspn2d_nl_sample_backward_det_g16):
        with pytest.raises(ValueError, match="grad_out"):
            fn(o.half(), f, torch.rand(1, 16, 6, 9))
        with pytest.raises(TypeError, match="float32"):
            fn(o.half(), f, gk.half())
    # the float32 functions still take float32 and nothing else
    for dt in (h, bf):
        for fn in (F.cspn2d_forward_nl, lambda *t: F.cspn2d_backward_nl(*t[:4], go, 3), lambda *t: F.cspn2d_backward_nl_det(*t[:4], go, 3)):
            for i in range(4):
                args = [a, o, x, s]
                args[i] = args[i].to(dt)
                with pytest.raises(TypeError, match="float32"):
                    fn(*args, 3) if fn is F.cspn2d_forward_nl else fn(*args)
        for fn in (lambda o_, f_: F.cspn2d_nl_sample(o_, f_), lambda o_, f_: F.cspn2d_nl_sample_backward(o_, f_, gk),
                   lambda o_, f_: F.cspn2d_nl_sample_backward_det(o_, f_, gk)):
            with pytest.raises(TypeError, match="float32"):
                fn(o.to(dt), f)
            with pytest.raises(TypeError, match="float32"):
                fn(o, f.to(dt))
    # the module: 16-bit tensors are let through to the engine (which is GPU-only), float64 is not
    m = cspn_amd.NonLocal_Propagate(3)
    g = torch.rand(1, 8, 6, 9)
    for dt in (h, bf):
        with pytest.raises(cspn_amd.CspnError):
            m(g.to(dt), o.to(dt), x.to(dt), None, s.to(dt))
    with pytest.raises(TypeError):
        m(g, o.double(), x)
    with pytest.raises(TypeError, match="float32"):
        m(g, o.half(), x.double())


# ---- dispatch: 16-bit inputs reach the _g16 functions (the det ones where asked), float32 inputs the names they always reached ----
ALL_NAMES = TWINS + NEW


def _record(monkeypatch):
    seen = []

    def prop(name):
        def f(aff, offset, x, sparse_depth, grad_out, n_iter, kernel_size=3, history=None, need_aff=True, need_offset=True, need_x=True):
            seen.append(name)
            return (torch.zeros_like(aff) if need_aff else None, torch.zeros_like(offset) if need_offset else None, torch.zeros_like(x) if need_x else None)
        return f

    def samp(name):
        def f(offset, f_, grad_out, kernel_size=3, need_f=True, need_offset=True):
            seen.append(name)
            return torch.zeros_like(f_) if need_f else None, torch.zeros_like(offset) if need_offset else None
        return f

    def forward(name):
        def f(aff, offset, x, sparse_depth, n_iter, kernel_size=3, return_history=False):
            seen.append(name)
            return (x.clone(), torch.zeros(1)) if return_history else x.clone()
        return f

    def sample(name):
        def f(offset, f_, kernel_size=3):
            seen.append(name)
            return f_.expand(-1, 8, -1, -1).clone()
        return f
    for name in ALL_NAMES:
        make = (samp if "sample_backward" in name else sample if "sample" in name else prop if "backward" in name else forward)
        monkeypatch.setattr(F, name, make(name))
    return seen


def _leaves(da, do):
    return [torch.rand(*s).to(dt).requires_grad_(True) for s, dt in (((1, 8, 6, 9), da), ((1, 16, 6, 9), do), ((1, 2, 6, 9), torch.float32),
                                                                   ((1, 1, 6, 9), torch.float32))] + [torch.rand(1, 1, 6, 9)]


@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_dispatch_by_dtype(monkeypatch, dt):
    seen = _record(monkeypatch)

    def run(da, do, **kw):
        del seen[:]
        a, o, x, f, s = _leaves(da, do)
        nlspn.nl_propagate(a, o, x, s, 3, **kw).sum().backward()
        nlspn.nl_sample(o, f, **kw).sum().backward()
        with torch.no_grad():
            nlspn.nl_propagate(a, o, x, s, 3, **kw)
            nlspn.nl_sample(o, f, **kw)
        return list(seen)
    f32 = torch.float32
    fw, bw, bd, sm, sb, sd = TWINS
    assert run(f32, f32) == [fw, bw, sm, sb, fw, sm]
    assert run(f32, f32, deterministic=True) == [fw, bd, sm, sd, fw, sm]
    g = [n + "_g16" for n in TWINS]
    for da in (f32, dt):
        assert run(da, dt) == [g[0], g[1], g[3], g[4], g[0], g[3]], da
        assert run(da, dt, deterministic=True) == [g[0], g[2], g[3], g[5], g[0], g[3]], da
    try:
        torch.use_deterministic_algorithms(True)
        assert run(f32, dt) == [g[0], g[2], g[3], g[5], g[0], g[3]]
        assert run(f32, f32) == [fw, bd, sm, sd, fw, sm]
    finally:
        torch.use_deterministic_algorithms(False)
    # the module: a 16-bit affinity is normalised in float32, so the engine sees (float32, T); the confidence is sampled at 16-bit offsets
    for da, do, want in ((dt, dt, {g[0], g[2], g[3], g[5]}), (f32, dt, {g[0], g[2], g[3], g[5]}), (f32, f32, {fw, bd, sm, sd})):
        a, o, x, f, s = _leaves(da, do)
        m = cspn_amd.NonLocal_Propagate(3, 3, "TGASS")
        m.deterministic = True
        del seen[:]
        with torch.autocast("cpu", dtype=torch.bfloat16):
            y = m(a, o, x.to(dt), f.to(dt), s.to(dt))
        y.sum().backward()
        assert set(seen) == want and y.dtype == f32, (da, do, seen)
        assert a.grad.dtype == da and o.grad.dtype == do


# =================================================================================================================================== GPU
def _np64(t):
    return t.detach().double().cpu().numpy()


def _check16(got, ref, dt, what):
    """test_backward._check plus one rounding of the reference value to dt: element-wise
    |got - ref| <= GFLOOR max|ref| + (GTOL + EPS[dt]) |ref| + TINY[dt], and the max-norm within GTOL + EPS[dt] (+ TINY[dt] / max|ref|)"""
    a, b = _np64(got), _np64(ref)
    if dt == torch.float32:
        return _check(a, b, what)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)), what
    scale = max(np.abs(b).max(), 1e-30)
    d = np.abs(a - b)
    bound = GFLOOR * scale + (GTOL + EPS[dt]) * np.abs(b) + TINY[dt]
    worst, err = float((d / bound).max()), float(d.max() / scale)
    print("%s (%s): max-norm rel err %.3e, worst element at %.3f of its bound" % (what, _id(dt), err, worst))
    assert worst <= 1.0, "%s: element-wise bound exceeded %.3gx" % (what, worst)
    assert err <= GTOL + EPS[dt] + TINY[dt] / scale, "%s: max-norm relative error %.3g" % (what, err)
    return True


def _offsets16(off, kind, dt):
    """the offsets a 16-bit tensor can hold: fp16 'huge' uses +-60000 (exact in fp16, finite, outside every image) in place of +-1e9"""
    if kind == "huge" and dt == torch.float16:
        off = torch.where(off.abs() == 1e9, off.sign() * 60000.0, off)
    return off.to(dt)


@functools.lru_cache(maxsize=None)
def _case(H, W, C, sparse, kind, dt, pair, n=N_ITER):
    """16-bit inputs on the device, and the float32 engine's results on their widened copies: made once"""
    aff, off, x, s, go = _inputs(H, W, C, sparse, kind, _seed(H, W, C, sparse, kind))
    off16 = _offsets16(off, kind, dt)
    aff16 = aff.to(dt)
    a, o, xd, sd, god = _cuda(aff16 if pair == "TT" else aff16.float(), off16, x, s, go)
    aw, ow = a.float(), o.float()
    assert aw.data_ptr() != a.data_ptr() or pair == "0T"
    out, hist = F.cspn2d_forward_nl(aw, ow, xd, sd, n, return_history=True)
    det = F.cspn2d_backward_nl_det(aw, ow, xd, sd, god, n, history=hist)
    return dict(dev=(a, o, xd, sd, god), wide=(aw, ow), out=out, hist=hist, det=det, cpu=(aff16.float(), off16.float(), x, s, go))


@functools.lru_cache(maxsize=None)
def _statement(H, W, C, sparse, kind, dt, n):
    """the float64 statement's gradients on the widened tensors"""
    aff, off, x, s, go = _case(H, W, C, sparse, kind, dt, "TT", n)["cpu"]
    leaves = [t.double().requires_grad_(True) for t in (aff, off, x)]
    nl_levels(*leaves, None if s is None else s.double(), n)[-1].backward(go.double())
    return [t.grad for t in leaves]


def _grads_close16(got, want, dts, names=NAMES):
    for g, w, dt, what in zip(got, want, dts, names):
        assert g.dtype == dt, (what, g.dtype)
        _check16(g, w, dt, what)


def _same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        assert a is None or memguard.same_bits(a, b), "%s: output %d differs (%s vs %s)" % (what, i, a.dtype, b.dtype)


def _det_want(c):
    """the float32 det result as the 16-bit entry point must return it: grad_aff / grad_offset cast once to the stored dtypes"""
    a, o = c["dev"][:2]
    ga, gd, gx = c["det"]
    return ga.to(a.dtype), gd.to(o.dtype), gx


GRID = [c + (dt, pair) for c in CASES for dt in DTYPES for pair in PAIRS]
GRID_IDS = ["%dx%d-C%d-%s-%s-%s-%s" % (c[0], c[1], c[2], "masked" if c[3] else "plain", c[4], _id(c[5]), c[6]) for c in GRID]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,sparse,kind,dt,pair", GRID, ids=GRID_IDS)
def test_forward_bitwise_and_det_backward_bitwise(H, W, C, sparse, kind, dt, pair):
    c = _case(H, W, C, sparse, kind, dt, pair)
    a, o, xd, sd, god = c["dev"]
    assert o.dtype == dt and a.dtype == (dt if pair == "TT" else torch.float32)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(c["out"]).all())
    out, hist = F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER, return_history=True)
    assert out.dtype == torch.float32 and hist.dtype == torch.float32
    assert memguard.same_bits(out, c["out"]) and memguard.same_bits(hist, c["hist"])
    assert memguard.same_bits(F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER), c["out"])   # through the ping-pong levels
    got = F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER, history=hist)
    assert [g.dtype for g in got] == [a.dtype, o.dtype, torch.float32]
    _same(got, _det_want(c), "det backward")
    if (H, W, C, sparse, kind) in THIN:
        _same(F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER, history=hist), got, "second call")
        _same(F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER), got, "without a kept history")
        # the (0, 0) pair through the new entry point: bitwise the float32 entry point
        aw, ow = c["wide"]
        _same((F.cspn2d_forward_nl_g16(aw, ow, xd, sd, N_ITER),) + F.cspn2d_backward_nl_det_g16(aw, ow, xd, sd, god, N_ITER, history=hist),
              (c["out"],) + tuple(c["det"]), "the float32 pair")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", PAIRS)
def test_scatter_backward_every_gradient_subset(n, sparse, dt, pair):
    H, W, C, kind = 17, 65, 3, "normal"
    c = _case(H, W, C, sparse, kind, dt, pair, n)
    a, o, xd, sd, god = c["dev"]
    ref = _statement(H, W, C, sparse, kind, dt, n)
    dts = (a.dtype, o.dtype, torch.float32)
    for need in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)):
        for history in (None, c["hist"]):
            got = F.cspn2d_backward_nl_g16(a, o, xd, sd, god, n, 3, history, *map(bool, need))
            assert [g is not None for g in got] == list(map(bool, need))
            keep = [i for i in range(3) if need[i]]
            _grads_close16([got[i] for i in keep], [ref[i] for i in keep], [dts[i] for i in keep], [NAMES[i] for i in keep])
    assert F.cspn2d_backward_nl_g16(a, o, xd, sd, god, n, 3, None, False, False, False) == (None, None, None)
    if sparse:
        assert bool((got[2].cpu()[(c["cpu"][3] > 0).expand(B, C, H, W)] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("pair", PAIRS)
def test_fp16_subnormal_gradients_are_rounded_once(pair):
    """grad_out scaled by 2^-20 (exact): grad_aff falls below 2^-14, where fp16 is subnormal with a spacing of 2^-24.  Rounding the float32 sum once
    gives the float32 result's .to(float16); rounding through a normalised intermediate would not"""
    H, W, C, sparse, kind = 17, 65, 3, True, "normal"
    c = _case(H, W, C, sparse, kind, torch.float16, pair)
    a, o, xd, sd, god = c["dev"]
    small = god * 2.0 ** -20
    aw, ow = c["wide"]
    want = F.cspn2d_backward_nl_det(aw, ow, xd, sd, small, N_ITER, history=c["hist"])
    got = F.cspn2d_backward_nl_det_g16(a, o, xd, sd, small, N_ITER, history=c["hist"])
    _same(got, (want[0].to(a.dtype), want[1].to(o.dtype), want[2]), "subnormal gradients")
    for g in (got[0],) if pair == "TT" else () + (got[1],):
        mag = g.float().abs()
        sub = (mag > 0) & (mag < 2.0 ** -14)
        print("%d of %d elements are non-zero fp16 subnormals" % (int(sub.sum()), g.numel()))
        assert int(sub.sum()) >= 100


def _shifted(t, k):
    """a view k elements behind a 256-byte boundary"""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 256 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + k * t.element_size()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,sparse", [(16, 64, True), (18, 68, False), (17, 65, True)])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", PAIRS)
def test_alignment(H, W, sparse, dt, pair):
    """aff / offset 1, 2 and 4 elements off a 16-byte boundary (a 16-bit tensor is then 2-, 4- and 8-byte aligned: only the last takes the quad
    loads; a float32 aff is 4-, 8- and 16-byte aligned), each tensor alone and all together: the aligned call's bits"""
    C, kind = 3, "normal"
    c = _case(H, W, C, sparse, kind, dt, pair)
    dev = c["dev"]
    ref = _statement(H, W, C, sparse, kind, dt, N_ITER)
    dts = (dev[0].dtype, dev[1].dtype, torch.float32)
    variants = [[_shifted(t, k) if j == i else t for j, t in enumerate(dev)] for i in (0, 1) for k in (1, 2, 4)]
    variants += [[_shifted(t, 1) if j == i else t for j, t in enumerate(dev)] for i in (2, 3, 4) if dev[i] is not None]
    variants += [[_shifted(t, k) for t in dev] for k in (1, 2, 4)]
    assert dev[0].data_ptr() % 16 == 0 and dev[1].data_ptr() % 16 == 0
    for v in variants:
        a, o, xd, sd, god = v
        out, hist = F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER, return_history=True)
        _same((out, hist, F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER)), (c["out"], c["hist"], c["out"]), "forward, shifted")
        _same(F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER, history=hist), _det_want(c), "det backward, shifted")
        _grads_close16(F.cspn2d_backward_nl_g16(a, o, xd, sd, god, N_ITER, history=hist), ref, dts)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(16, 64), (17, 65)])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("pair", PAIRS)
def test_nan_affinities_and_infinite_offsets_stay_inside(H, W, dt, pair):
    """a NaN affinity, a NaN offset and offsets of +-inf (fp16: 1e9 cast to fp16) at a few pixels: out has the bits of the float32 engine on the widened
    tensors (NaNs canonicalised), and the call runs between guard bands"""
    C, sparse = 3, True
    aff, off, x, s, go = _inputs(H, W, C, sparse, "normal", 8100 + W)
    aff16, off16 = aff.to(dt), off.to(dt)
    big = torch.tensor([1e9, -1e9]).to(dt) if dt == torch.float16 else torch.tensor([float("inf"), float("-inf")]).to(dt)
    assert bool(torch.isinf(big).all())
    aff16[0, 3, 2, 5] = float("nan")
    aff16[1, 0, H - 1, W - 1] = float("nan")
    off16[0, 4, 1, 1], off16[0, 5, 1, 1] = big[0], big[1]
    off16[1, 0, H - 1, 0], off16[1, 15, 0, W - 1] = big[1], big[0]
    off16[0, 7, H // 2, W // 2] = float("nan")
    a, o, xd, sd, god = _cuda(aff16 if pair == "TT" else aff16.float(), off16, x, s, go)
    want, want_hist = F.cspn2d_forward_nl(a.float(), o.float(), xd, sd, N_ITER, return_history=True)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want).any())

    def call(a, o, xd, sd, god):
        out, hist = F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER, return_history=True)
        grads = F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER, history=hist) + F.cspn2d_backward_nl_g16(a, o, xd, sd, god, N_ITER, history=hist)
        return (out, hist, F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER)) + grads
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, "ones", call, (a, o, xd, sd, god), "cuda", 4 * B * 16 * H * W)
    assert len(session.workspaces) >= 4
    _same(outs[:3], (want, want_hist, want), "NaN / inf")


# ---- the sampling operator ----
@functools.lru_cache(maxsize=None)
def _sample_case(H, W, kind, dt):
    gen = torch.Generator().manual_seed(300 + W + KINDS.index(kind))
    off = _offsets16(test_nl._offsets(kind, H, W, gen), kind, dt)
    f = torch.rand(B, 1, H, W, generator=gen) * 2 - 0.5
    go = torch.randn(B, 8, H, W, generator=gen)
    leaves = [t.double().requires_grad_(True) for t in (off.float(), f)]
    sample_all(*leaves).backward(go.double())
    return _cuda(off, f, go), [t.grad for t in leaves]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_sampling_operator_and_its_backwards(H, W, kind, dt):
    (od, fd, god), (rgo, rgf) = _sample_case(H, W, kind, dt)
    ow = od.float()
    out = F.cspn2d_nl_sample_g16(od, fd)
    assert out.dtype == torch.float32 and memguard.same_bits(out, F.cspn2d_nl_sample(ow, fd))
    assert memguard.same_bits(F.cspn2d_nl_sample_g16(ow, fd), out)   # the float32 code through the new entry point
    wf, wd = F.cspn2d_nl_sample_backward_det(ow, fd, god)
    got = F.cspn2d_nl_sample_backward_det_g16(od, fd, god)
    assert got[0].dtype == torch.float32 and got[1].dtype == dt
    _same(got, (wf, wd.to(dt)), "det sampling backward")
    _same(F.cspn2d_nl_sample_backward_det_g16(od, fd, god), got, "second call")
    gf2, none = F.cspn2d_nl_sample_backward_det_g16(od, fd, god, need_offset=False)
    none2, gd2 = F.cspn2d_nl_sample_backward_det_g16(od, fd, god, need_f=False)
    assert none is None and none2 is None
    _same((gf2, gd2), got, "one gradient at a time")
    gf, gd = F.cspn2d_nl_sample_backward_g16(od, fd, god)
    _grads_close16((gf, gd), (rgf, rgo), (torch.float32, dt), ("grad_f", "grad_offset"))
    assert memguard.same_bits(gd, got[1])   # grad_offset is written once by the same kernel
    for k in (1, 2, 4):   # the offset 2-, 4- and 8-byte aligned: one pixel per lane, the same bits
        o2 = _shifted(od, k)
        assert memguard.same_bits(F.cspn2d_nl_sample_g16(o2, fd), out)
        _same(F.cspn2d_nl_sample_backward_det_g16(o2, fd, god), got, "shifted")


# ---- the module under torch.autocast ----
class _Head(torch.nn.Module):
    """a 3 x 3 conv that emits 8 affinity and 16 offset planes, as an NLSPN head does"""

    def __init__(self, cin=6):
        super().__init__()
        self.conv = torch.nn.Conv2d(cin, 24, 3, padding=1)

    def forward(self, feat):
        y = self.conv(feat)
        return y[:, :8] * 0.5, y[:, 8:] * 4.0


@functools.lru_cache(maxsize=None)
def _head_case(H, W, dt):
    torch.manual_seed(1234 + W)
    head = _Head().cuda()
    gen = torch.Generator().manual_seed(77 + W)
    feat_in = torch.randn(B, 6, H, W, generator=gen).cuda()
    _, _, x, conf, s, go = test_nl._module_inputs(H, W, 2, 60 + W)
    return head, feat_in, _cuda(x, conf, s, go)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_conf", [False, True])
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_module_under_autocast(mode, use_conf, dt):
    """A 3 x 3 conv head under torch.autocast feeds NonLocal_Propagate inside the autocast region (deterministic=True): the output is float32 and
    bitwise the module's on .float() copies outside autocast, the conv's weights receive a gradient, and every gradient is held to the scatter
    test's bound: test_backward._check of test_nl's float64 _module_ref on the widened tensors plus ONE rounding of the reference value.

    With a confidence the offset is used twice, by the confidence sampling and by the steps.  Two gradients each rounded to the offset's dtype and
    added in it are three roundings, and where the two nearly cancel they miss this bound (the float64 statement's own two contributions, treated so,
    miss it 7 - 72 x); so the module adds the two float32 gradients and rounds once, which is what is held to the bound here."""
    H, W = ((17, 65), (16, 64))[MODES.index(mode) % 2 ^ int(use_conf)]
    head, feat_in, (x, conf, s, go) = _head_case(H, W, dt)
    head.zero_grad()
    m = cspn_amd.NonLocal_Propagate(N_ITER, 3, mode, test_nl.GAMMA, True).cuda()
    m.deterministic = True
    xl, cl = x.detach().requires_grad_(True), conf.detach().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt):
        g, off = head(feat_in)
        g.retain_grad()
        off.retain_grad()
        y = m(g, off, xl, cl if use_conf else None, s)
    assert g.dtype == dt and off.dtype == dt and y.dtype == torch.float32
    y.backward(go)
    assert g.grad.dtype == dt and off.grad.dtype == dt and xl.grad.dtype == torch.float32
    w = head.conv.weight.grad
    assert w is not None and bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
    # the same module on float32 copies, outside autocast: the same bits
    with torch.no_grad():
        m32 = cspn_amd.NonLocal_Propagate(N_ITER, 3, mode, test_nl.GAMMA, True).cuda()
        want = m32(g.detach().float(), off.detach().float(), x, conf if use_conf else None, s)
    assert memguard.same_bits(y.detach(), want)
    # the gradients against the float64 statement on the widened tensors
    cpu = [t.detach().float().cpu() for t in (g, off, x, conf, s, go)]
    ref, ref_grads = test_nl._module_ref(mode, *cpu, use_conf, True, N_ITER)
    assert test_nl.rel_err(y.detach().cpu().numpy(), ref.numpy()) <= test_nl.RTOL
    grads = [g.grad, off.grad, xl.grad] + ([cl.grad] if use_conf else []) + ([m.scale.grad] if mode == "TGASS" else [])
    dts = [dt, dt, torch.float32] + [torch.float32] * (len(grads) - 3)
    assert len(grads) == len(ref_grads) and all(t is not None for t in grads)
    missed = []
    for got, want, d, what in zip(grads, ref_grads, dts, test_nl.MODULE_NAMES):   # every figure is printed before anything is asserted
        assert got.dtype == d, what
        try:
            _check16(got, want, d, what)
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, missed


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_module_dispatch_on_the_gpu(dt, monkeypatch):
    """16-bit inputs reach the _g16 functions (the det ones under deterministic=True), float32 inputs the names they always reached"""
    calls = []
    for name in ALL_NAMES:
        monkeypatch.setattr(F, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(F, name), name))
    H, W = 17, 65
    g, off, x, conf, s, go = _cuda(*test_nl._module_inputs(H, W, 2, 91))
    for det in (True, False):
        for da, do in ((dt, dt), (torch.float32, dt), (torch.float32, torch.float32)):
            m = cspn_amd.NonLocal_Propagate(N_ITER, 3, "TGASS", test_nl.GAMMA, True).cuda()
            m.deterministic = det
            del calls[:]
            leaves = [t.detach().to(d).requires_grad_(True) for t, d in ((g, da), (off, do), (x, torch.float32), (conf, torch.float32))]
            m(*leaves, s).backward(go)
            tail = "_g16" if do == dt else ""
            want = {"cspn2d_forward_nl", "cspn2d_nl_sample", "cspn2d_backward_nl" + ("_det" if det else ""), "cspn2d_nl_sample_backward" + ("_det" if det else "")}
            assert set(calls) == {n + tail for n in want}, (det, da, do, calls)
            assert leaves[0].grad.dtype == da and leaves[1].grad.dtype == do


# ---- memory hygiene: every _g16 function and the module on 16-bit inputs between guard bands on NaN and on finite poison, and in a stale arena.
# The guarded buffers are laid out in bytes of the tensors' own element size (memguard.guarded), so the bands around a 16-bit gradient start right
# behind its last 2-byte element.  Forward and det outputs are compared bitwise with the clean run, the scatter's with the float64 statement ----
N_BITWISE = 13   # out, out (with a history), the history, the sample, det (3), det alone, det one step (3), sampling det (2); then the scatters


def _hygiene_inputs(H, W, C, sparse, kind, dt, pair):
    c = _case(H, W, C, sparse, kind, dt, pair)
    gen = torch.Generator().manual_seed(990 + W)
    f = torch.rand(B, 1, H, W, generator=gen).cuda()
    gk = torch.randn(B, 8, H, W, generator=gen).cuda()
    return tuple(c["dev"]) + (f, gk)


def _hygiene_call(a, o, x, s, go, f, gk):
    n = N_ITER
    out = F.cspn2d_forward_nl_g16(a, o, x, s, n)
    out2, hist = F.cspn2d_forward_nl_g16(a, o, x, s, n, return_history=True)
    smp = F.cspn2d_nl_sample_g16(o, f)
    det = F.cspn2d_backward_nl_det_g16(a, o, x, s, go, n, history=hist)
    alone = F.cspn2d_backward_nl_det_g16(a, o, x, s, go, n, 3, None, False, True, False)[1:2]   # its own forward; no grad_x
    one = F.cspn2d_backward_nl_det_g16(a, o, x, s, go, 1)
    sdet = F.cspn2d_nl_sample_backward_det_g16(o, f, gk)
    scatter = F.cspn2d_backward_nl_g16(a, o, x, s, go, n, history=hist)
    ssc = F.cspn2d_nl_sample_backward_g16(o, f, gk)
    return (out, out2, hist, smp) + tuple(det) + tuple(alone) + tuple(one) + tuple(sdet) + tuple(scatter) + tuple(ssc)


def _module_hygiene_inputs(H, W, dt):
    g, off, x, conf, s, go = test_nl._module_inputs(H, W, 2, 77 + W)
    return tuple(_cuda(g.to(dt), off.to(dt), x.to(dt), conf.to(dt), s.to(dt), go))


def _module_hygiene_call(g, off, x, conf, s, go):
    outs = []
    for mode in ("TGASS", "AS"):
        m = cspn_amd.NonLocal_Propagate(N_ITER, 3, mode, test_nl.GAMMA, True).cuda()
        m.deterministic = True
        leaves = [t.detach().requires_grad_(True) for t in (g, off, x, conf)]
        y = m(*leaves, s)
        y.backward(go)
        outs += [y.detach()] + [t.grad for t in leaves] + ([m.scale.grad] if mode == "TGASS" else [])
    return tuple(outs)


HYGIENE = {}
for _H, _W, _C, _sp, _kind, _dt, _pair in ((17, 65, 3, True, "normal", torch.float16, "0T"), (33, 132, 1, False, "hot", torch.bfloat16, "TT"),
                                           (16, 64, 1, True, "huge", torch.float16, "TT"), (5, 8, 3, True, "integer", torch.bfloat16, "0T")):
    _name = "nl-g16-%dx%d-C%d-%s-%s-%s-%s" % (_H, _W, _C, "masked" if _sp else "plain", _kind, _id(_dt), _pair)
    HYGIENE[_name] = (tuple(NEW), functools.partial(_hygiene_inputs, _H, _W, _C, _sp, _kind, _dt, _pair), _hygiene_call, 4 * B * max(_C, 16) * _H * _W,
                      (_H, _W, _C, _sp, _kind, _dt, _pair), (_H, _W))
for _H, _W, _dt in ((17, 65, torch.float16), (16, 64, torch.bfloat16)):
    _name = "nl-g16-module-%dx%d-%s" % (_H, _W, _id(_dt))
    HYGIENE[_name] = (("NonLocal_Propagate",), functools.lru_cache(maxsize=None)(functools.partial(_module_hygiene_inputs, _H, _W, _dt)), _module_hygiene_call,
                      4 * B * 16 * _H * _W, None, (_H, _W))
_CLEAN = {}


def test_the_hygiene_table_covers_every_new_function_and_both_dtypes_and_pairs():
    assert {n for c in HYGIENE.values() for n in c[0]} == set(NEW) | {"NonLocal_Propagate"}
    keys = [c[4] for c in HYGIENE.values() if c[4]]
    assert {k[5] for k in keys} == set(DTYPES) and {k[6] for k in keys} == set(PAIRS)
    assert not set(HYGIENE) & set(test_nl.HYGIENE)


def _clean(name):
    if name not in _CLEAN:
        build, call = HYGIENE[name][1:3]
        a, b = call(*build()), call(*build())
        torch.cuda.synchronize()
        nb = N_BITWISE if "module" not in name else len(a)
        memguard.assert_same_outputs(b[:nb], a[:nb], "second clean run")
        _CLEAN[name] = a
    return _CLEAN[name]


def _assert_hygiene(name, outs, what):
    clean = _clean(name)
    for t in outs:
        assert t is None or bool(torch.isfinite(t.float()).all()), "%s: poison reached an output" % what
    if "module" in name:
        return memguard.assert_same_outputs(outs, clean, what)   # forward and det backward throughout
    nb = N_BITWISE
    memguard.assert_same_outputs(outs[:nb], clean[:nb], what)
    H, W, C, sp, kind, dt, pair = HYGIENE[name][4]
    ref = _statement(H, W, C, sp, kind, dt, N_ITER)
    _grads_close16(outs[nb:nb + 3], ref, (outs[4].dtype, outs[5].dtype, torch.float32))   # the scatter: the statement's, in the det call's dtypes
    # the sampling scatter: grad_f against the float64 statement, grad_offset written once by the kernel the det call uses
    off, f, gk = (t.detach().float().cpu().double() for t in (HYGIENE[name][1]()[i] for i in (1, 5, 6)))
    leaf = f.clone().requires_grad_(True)
    sample_all(off, leaf).backward(gk)
    _check16(outs[nb + 3], leaf.grad, torch.float32, "sampling scatter grad_f")
    assert memguard.same_bits(outs[nb + 4], clean[nb - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(HYGIENE))
@pytest.mark.parametrize("poison", ["ones", "big"])
def test_every_call_between_guard_bands(name, poison):
    _, build, call, plane, _, (H, W) = HYGIENE[name]
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, call, build(), "cuda", plane)
    assert len(session.workspaces) >= 3 and len(session.guards) > len(session.workspaces)
    # a 16-bit grad_offset lies in a payload of 2 bytes an element: its back guard starts right behind the last of them
    assert any(g.nbytes == 2 * B * 16 * H * W for g in session.guards)
    _assert_hygiene(name, outs, "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    order = list(HYGIENE) + [list(HYGIENE)[0]]
    plane = 4 * B * 16 * 33 * 132
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "zero", plane_bytes=plane)
        for name in order:
            HYGIENE[name][2](*HYGIENE[name][1]())
            session.check()
        sizes = [n for _, n in session.workspaces]
    assert sizes and max(sizes) > 0
    arena = memguard.Arena(max(sizes), "cuda", plane)
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "stale", arena=arena, plane_bytes=plane)
        for i, name in enumerate(order):
            inputs = HYGIENE[name][1]()
            snap = memguard.snapshot(*inputs)
            outs = HYGIENE[name][2](*inputs)
            session.check()
            snap.assert_unchanged()
            _assert_hygiene(name, outs, "step %d (%s) in the stale arena" % (i + 1, name))
    assert arena.taken > 0


# ---- streams and a captured graph ----
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
def test_side_stream_and_captured_graph_give_the_eager_bits(dt):
    H, W, C, sparse, kind, pair = 33, 132, 3, True, "normal", "0T"
    c = _case(H, W, C, sparse, kind, dt, pair)
    a, o, xd, sd, god = c["dev"]

    def run():
        out, hist = F.cspn2d_forward_nl_g16(a, o, xd, sd, N_ITER, return_history=True)
        return (out,) + F.cspn2d_backward_nl_det_g16(a, o, xd, sd, god, N_ITER, history=hist)
    eager = run()
    _same(eager, (c["out"],) + _det_want(c), "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = run()
    side.synchronize()
    _same(got, eager, "side stream")
    # a captured graph: the workspaces (the det one included) are sized by host arithmetic and allocated from the graph's pool during capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        run()
    torch.cuda.current_stream().wait_stream(warm)
    assert _lib.symbol("cspn2d_backward_nl_det_workspace_bytes")(B, C, H, W, 3, N_ITER, 1) > 0
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _same(captured, eager, "graph replay")
