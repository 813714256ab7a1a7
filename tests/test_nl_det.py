"""The run-to-run bitwise backward of non-local propagation (cspn2d_backward_nl_det_f32, cspn2d_nl_sample_backward_det_f32; cspn_amd/csrc/
cspn2d_nl_det.hip): the adjoint gathers through an inverted index of the operator and sums each destination's terms in an order-independent way.

The statement, the inputs and the bounds are tests/test_nl.py's: every gradient lies within test_backward._check of the float64 statement, the bound
the scatter is held to.  What is new here is asserted bit for bit: two calls give the same gradients, and a mirrored problem -- the same multiset of
terms at every destination, met in another order -- gives the mirrored grad_x."""
import contextlib
import ctypes
import functools
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
import memguard
import test_nl
from cspn_amd import _lib
from cspn_amd import functional as F
from cspn_amd import nlspn
from test_backward import _check
from test_kxk_norm import _cuda, _misaligned
from test_nl import B, CASES, KINDS, MODES, N_ITER, SHAPES, _case, _inputs, _seed, bases, nl_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cspn2d_backward_nl_det_workspace_bytes", "cspn2d_backward_nl_det_f32", "cspn2d_nl_sample_backward_det_workspace_bytes",
       "cspn2d_nl_sample_backward_det_f32"]
NAMES = test_nl.NAMES


# =================================================================================================================================== CPU
def test_new_symbols_are_exported_declared_and_nothing_else_moved():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % s, text)
        assert m, "not declared: " + s
        assert "int K" in m.group(1), s
        assert hasattr(lib, s), "not exported: " + s
        assert _lib.symbol(s) is not None
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION
    assert len(cspn_amd.__all__) == 36
    sig = lambda f: list(inspect.signature(f).parameters)   # noqa: E731
    for twin in ("cspn2d_backward_nl", "cspn2d_nl_sample_backward"):
        det = getattr(F, twin + "_det")
        assert callable(det) and not hasattr(cspn_amd, twin + "_det") and twin + "_det" not in cspn_amd.__all__
        assert str(inspect.signature(det)) == str(inspect.signature(getattr(F, twin))), twin
    assert sig(nlspn.nl_propagate) == "aff offset x sparse_depth n_iter kernel_size deterministic".split()
    assert sig(nlspn.nl_sample) == "offset f kernel_size deterministic".split()
    assert inspect.signature(nlspn.nl_propagate).parameters["deterministic"].default is None
    assert inspect.signature(nlspn.nl_sample).parameters["deterministic"].default is None
    assert nlspn.NonLocal_Propagate.deterministic is None and "deterministic" in vars(nlspn.NonLocal_Propagate)
    m = cspn_amd.NonLocal_Propagate(3)
    m.deterministic = True
    assert m.deterministic is True and nlspn.NonLocal_Propagate.deterministic is None and "deterministic" not in m.state_dict()
    assert sig(nlspn.NonLocal_Propagate.forward) == "self affinity offset feat confidence sparse_depth n_iter".split()
    assert sig(nlspn.NonLocal_Propagate.__init__) == "self prop_time prop_kernel affinity affinity_gamma preserve_input".split()


def _r(b):
    return (b + 255) // 256 * 256


def _index_bytes(P, c):
    """include/cspn_amd.h: the worklist counter, the starts, the cursors, the plane c, the worklist, the scan's partials, the entries"""
    return 256 + _r(4 * (P + 1)) + _r(4 * P) + c * _r(4 * P) + _r(4 * (P // 4 + 1)) + _r(4 * ((P + 2047) // 2048)) + 256 * P


def test_byte_queries_are_the_headers_closed_forms():
    det, smp, bws = (_lib.symbol(s) for s in (NEW[0], NEW[2], "cspn2d_backward_nl_workspace_bytes"))
    for Bq, C, H, W in ((2, 3, 17, 65), (1, 1, 1, 1), (2, 1, 33, 132), (8, 1, 352, 1216), (1, 2, 64, 32)):
        P = Bq * H * W
        level = 4 * ((Bq * C * H * W + 63) // 64 * 64)
        for n in (1, 2, 3, 18):
            for sp in (0, 1):
                assert bws(Bq, C, H, W, 3, n, sp) == (n - 1 + sp) * level
                assert det(Bq, C, H, W, 3, n, sp) == (n - 1 + sp) * level + _index_bytes(P, 1), (Bq, C, H, W, n, sp)
        assert det(Bq, C, H, W, 3, 0, 0) == 0 == det(Bq, C, H, W, 3, 0, 1)   # the identity: no adjoint step, no index
        assert smp(Bq, H, W, 3) == _index_bytes(P, 0)
        assert _index_bytes(P, 1) % 256 == 0 and 264 * P < _index_bytes(P, 1) <= 270 * P + 6 * 256   # about 270 bytes a pixel
    Bq, C, H, W = 2, 3, 17, 65
    for bad in ((0, C, H, W, 3, 4), (Bq, 0, H, W, 3, 4), (Bq, C, 0, W, 3, 4), (Bq, C, H, 0, 3, 4), (Bq, C, H, W, 5, 4), (Bq, C, H, W, 7, 4), (Bq, C, H, W, 3, -1),
                (1, 1, 1 << 16, 1 << 15, 3, 4)):   # the list of test_nl.test_byte_queries
        assert det(*bad, 1) == 0 and bws(*bad, 1) == 0, bad
    for bad in ((0, H, W, 3), (Bq, 0, W, 3), (Bq, H, 0, 3), (Bq, H, W, 5), (Bq, H, W, 7), (1, 1 << 16, 1 << 15, 3)):
        assert smp(*bad) == 0, bad


def test_abi_argument_errors_without_gpu():
    lib = cspn_amd.load()
    bw, sb = _lib.symbol(NEW[1]), _lib.symbol(NEW[3])
    a, o, x, s, out, h, w, go, ga, gd, gx, f, gf = (ctypes.c_void_p(i << 32) for i in range(1, 14))
    err = lambda: lib.cspn_last_error()   # noqa: E731
    M = 1 << 24
    hb = 4 * 2 * 8 * 8 * 3
    shape = (2, 1, 8, 8)

    def bwd(a=a, o=o, x=x, s=s, h=h, hb=hb, go=go, ga=ga, gd=gd, gx=gx, shape=shape, K=3, n=4, w=w, wb=M):
        return bw(a, o, x, s, h, hb, go, ga, gd, gx, *shape, K, n, w, wb, None)

    def smp(o=o, f=f, go=go, gf=gf, gd=gd, shape=shape, K=3, w=w, wb=M):
        return sb(o, f, go, gf, gd, shape[0], shape[2], shape[3], K, w, wb, None)

    for kw in (dict(a=None), dict(o=None), dict(x=None), dict(go=None)):
        assert bwd(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(o=None), dict(f=None), dict(go=None)):
        assert smp(**kw) == -1 and b"null" in err(), kw
    for call in (bwd, smp):
        for bad in ((0, 1, 8, 8), (2, 1, 0, 8), (2, 1, 8, -1)):
            assert call(shape=bad) == -1 and b"shape" in err(), bad
        for K in (5, 7, 1, 4):
            assert call(K=K) == -3 and b"K" in err(), K
        assert call(shape=(1, 1, 1 << 16, 1 << 15)) == -3 and b"too large" in err()
        assert call(wb=64) == -2 and b"workspace" in err()
        assert call(w=None) == -2 and b"workspace" in err()
        assert call(w=ctypes.c_void_p((7 << 32) + 16)) == -2 and b"aligned" in err()
        for t in (o, go):   # the workspace on an input
            assert call(w=t) == -1 and b"alias" in err()
    assert bwd(shape=(2, 0, 8, 8)) == -1 and b"shape" in err()
    assert bwd(n=-1) == -1 and b"n_iter" in err()
    assert bwd(shape=(1, 40, 1 << 13, 1 << 13)) == -3 and b"too large" in err()
    # the workspace a byte short of the query
    need = _lib.symbol(NEW[0])(*shape, 3, 4, 1)
    assert need > 0 and bwd(wb=need - 1) == -2 and b"workspace" in err()
    need = _lib.symbol(NEW[2])(2, 8, 8, 3)
    assert need > 0 and smp(wb=need - 1) == -2 and b"workspace" in err()
    # grad_aff and grad_offset need the history where n_iter >= 2; grad_x does not
    assert bwd(h=None, hb=0) == -1 and b"history" in err()
    assert bwd(h=None, hb=0, ga=None) == -1 and b"history" in err()
    assert bwd(hb=hb - 4) == -1 and b"history" in err()
    for kw in (dict(ga=gx), dict(gd=ga), dict(gx=go), dict(ga=h), dict(w=ga), dict(w=gx), dict(w=a), dict(w=x), dict(w=s), dict(w=h)):
        assert bwd(**kw) == -1 and b"alias" in err(), kw
    assert bwd(ga=None, gd=None, gx=None) == 0   # nothing asked for: nothing to do
    for kw in (dict(gd=gf), dict(gf=f), dict(gd=go), dict(w=gf), dict(w=gd), dict(w=f)):
        assert smp(**kw) == -1 and b"alias" in err(), kw
    assert smp(gf=None, gd=None) == 0


def test_python_argument_errors_without_gpu():
    a, o, x, s, go = torch.rand(1, 8, 6, 9), torch.rand(1, 16, 6, 9), torch.rand(1, 2, 6, 9), torch.rand(1, 1, 6, 9), torch.rand(1, 2, 6, 9)
    f, gk = torch.rand(1, 1, 6, 9), torch.rand(1, 8, 6, 9)

    def call(a=a, o=o, x=x, s=s, n=3, **k):
        return F.cspn2d_backward_nl_det(a, o, x, s, go, n, **k)
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
        F.cspn2d_backward_nl_det(a, o, x, s, go.double(), 3)
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_backward_nl_det(a, o, x, s, torch.rand(1, 3, 6, 9), 3)

    def smp(**k):
        return F.cspn2d_nl_sample_backward_det(k.pop("o", o), k.pop("f", f), gk, **k)
    with pytest.raises(ValueError):
        smp(o=torch.rand(1, 8, 6, 9))
    with pytest.raises(ValueError, match="f "):
        smp(f=torch.rand(1, 2, 6, 9))
    with pytest.raises(ValueError, match="kernel_size"):
        smp(kernel_size=5)
    with pytest.raises(TypeError, match="float32"):
        smp(f=f.half())
    with pytest.raises(TypeError, match="float32"):
        smp(o=o.double())
    with pytest.raises(cspn_amd.CspnError):
        smp()
    with pytest.raises(ValueError, match="grad_out"):
        F.cspn2d_nl_sample_backward_det(o, f, torch.rand(1, 16, 6, 9))


# ---- dispatch: which backward an autograd pass reaches ----
BACKWARDS = ("cspn2d_backward_nl", "cspn2d_backward_nl_det", "cspn2d_nl_sample_backward", "cspn2d_nl_sample_backward_det")


def _record(monkeypatch):
    """the four backward functions replaced by recorders, the two forwards by stand-ins (the engine is GPU-only; the dispatch is not)"""
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
    for name in BACKWARDS:
        monkeypatch.setattr(F, name, (samp if "sample" in name else prop)(name))

    def forward(aff, offset, x, sparse_depth, n_iter, kernel_size=3, return_history=False):
        return (x.clone(), torch.zeros(1)) if return_history else x.clone()
    monkeypatch.setattr(F, "cspn2d_forward_nl", forward)
    monkeypatch.setattr(F, "cspn2d_nl_sample", lambda offset, f, kernel_size=3: f.expand(-1, 8, -1, -1).clone())
    return seen


def _leaves():
    return [torch.rand(*s).requires_grad_(True) for s in ((1, 8, 6, 9), (1, 16, 6, 9), (1, 2, 6, 9), (1, 1, 6, 9))] + [torch.rand(1, 1, 6, 9)]


def _dispatch(seen, **kw):
    """-> the backward functions one nl_propagate and one nl_sample reach, in call order"""
    del seen[:]
    a, o, x, f, s = _leaves()
    nlspn.nl_propagate(a, o, x, s, 3, **kw).sum().backward()
    nlspn.nl_sample(o, f, **kw).sum().backward()
    return list(seen)


def test_dispatch_follows_torchs_flag_unless_forced(monkeypatch):
    seen = _record(monkeypatch)
    scatter, det = [BACKWARDS[0], BACKWARDS[2]], [BACKWARDS[1], BACKWARDS[3]]
    assert not torch.are_deterministic_algorithms_enabled()
    assert _dispatch(seen) == scatter
    assert _dispatch(seen, deterministic=None) == scatter
    assert _dispatch(seen, deterministic=True) == det
    assert _dispatch(seen, deterministic=False) == scatter
    try:
        torch.use_deterministic_algorithms(True)
        assert _dispatch(seen) == det
        assert _dispatch(seen, deterministic=False) == scatter
        assert _dispatch(seen, deterministic=True) == det
        # the flag is read when the backward runs, not when the graph is made
        a, o, x, f, s = _leaves()
        y = nlspn.nl_propagate(a, o, x, s, 3)
        torch.use_deterministic_algorithms(False)
        del seen[:]
        y.sum().backward()
        assert seen == scatter[:1]
    finally:
        torch.use_deterministic_algorithms(False)
    # the module: its attribute, on the class None, set on an instance
    for forced, flag, want in ((None, False, scatter), (True, False, det), (False, True, scatter), (None, True, det)):
        a, o, x, f, s = _leaves()
        m = cspn_amd.NonLocal_Propagate(3, 3, "TC")
        if forced is not None:
            m.deterministic = forced
        del seen[:]
        try:
            torch.use_deterministic_algorithms(flag)
            m(a, o, x, f, s).sum().backward()
        finally:
            torch.use_deterministic_algorithms(False)
        assert sorted(seen) == sorted(want), (forced, flag, seen)


# ---- the documented sum, as a model in numpy and Python integers ----
def _int_to_f32_scaled(S, s):
    """ldexpf(__ll2float_rn(S), -s): the integer rounded to 24 bits, ties to even, then scaled (exact in the normal range)"""
    a = abs(S)
    shift = a.bit_length() - 24
    if shift > 0:
        q, r = divmod(a, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and q & 1):
            q += 1
        a = q << shift
    return np.float32(math.copysign(math.ldexp(float(a), -s), S))


def model_sum(terms):
    t = np.asarray(terms, np.float32)
    if np.isnan(t).any() or (np.isposinf(t).any() and np.isneginf(t).any()):
        return np.float32("nan")
    if np.isinf(t).any():
        return t[np.isinf(t)][0]
    mx = float(np.abs(t).max())
    if mx == 0.0:
        return np.float32(0.0)
    e = math.frexp(mx)[1] - 1
    L = (len(t) - 1).bit_length()          # ceil(log2 m)
    s = 61 - e - L
    q = [int(v) for v in np.rint(np.ldexp(t.astype(np.float64), s))]   # exact scaling, round to nearest even
    assert max(abs(v) for v in q) <= 1 << (62 - L)
    S = sum(q)
    assert abs(S) <= 1 << 62
    return _int_to_f32_scaled(S, s)


@pytest.mark.parametrize("m", [1, 2, 33, 5000])
def test_the_documented_sum_ignores_order_and_is_within_an_ulp_of_the_exact_sum(m):
    rng = np.random.RandomState(m)
    ex = rng.randint(-20, 20, m)
    ex[:2] = (-20, 19)[:m]   # both ends of the 40 binades are drawn
    t = (rng.uniform(1, 2, m) * np.exp2(ex) * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    assert m == 1 or np.frexp(np.abs(t))[1].max() - np.frexp(np.abs(t))[1].min() == 39
    want = model_sum(t)
    for _ in range(100):
        assert model_sum(rng.permutation(t)).tobytes() == want.tobytes()
    exact = math.fsum(float(v) for v in t)
    ulp = float(np.spacing(np.float32(abs(exact))))
    print("m = %d: model %.9g, exact %.17g, |model - exact| = %.3g ulp" % (m, want, exact, abs(float(want) - exact) / ulp))
    assert abs(float(want) - exact) <= ulp
    # the special cases
    assert model_sum(np.zeros(m, np.float32)).tobytes() == np.float32(0.0).tobytes()
    assert model_sum(-np.zeros(m, np.float32)).tobytes() == np.float32(0.0).tobytes()
    if m >= 2:
        u = t.copy()
        u[0] = np.inf
        assert model_sum(u) == np.inf
        u[1] = -np.inf
        assert np.isnan(model_sum(u))
        u[1] = np.nan
        assert np.isnan(model_sum(u))


# =================================================================================================================================== GPU
def _equal(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (what, i)
        assert a is None or torch.equal(a, b), "%s: output %d differs" % (what, i)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,sparse,kind", CASES)
def test_every_gradient_vs_fp64_statement(H, W, C, sparse, kind):
    """the bound the scatter is held to.  'hot' puts 8 H W taps on each of four addresses per image: the long-list kernel runs in these cases"""
    c = _case(H, W, C, sparse, kind)
    ad, od, xd, sd, god = c["dev"]
    got = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, N_ITER, history=c["hist"])
    test_nl._grads_close(got, c["ref_grads"])
    if sparse:   # a pinned pixel passes no gradient to x
        assert bool((got[2].cpu()[(c["sparse"] > 0).expand(B, C, H, W)] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,sparse,kind", [CASES[3], CASES[12], CASES[21], CASES[30]])
def test_the_backward_twice_gives_identical_bits(H, W, C, sparse, kind):
    c = _case(H, W, C, sparse, kind)
    ad, od, xd, sd, god = c["dev"]
    first = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, N_ITER, history=c["hist"])
    _equal(F.cspn2d_backward_nl_det(ad, od, xd, sd, god, N_ITER, history=c["hist"]), first, "second call")
    _equal(F.cspn2d_backward_nl_det(ad, od, xd, sd, god, N_ITER), first, "without a kept history")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_sampling_backward_vs_bil_and_twice_bitwise(H, W, kind):
    (od, fd, god), _, (rgo, rgf) = test_nl._sample_case(H, W, kind)
    gf, gd = F.cspn2d_nl_sample_backward_det(od, fd, god)
    test_nl._grads_close((gf, gd), (rgf, rgo), ("grad_f", "grad_offset"))
    _equal(F.cspn2d_nl_sample_backward_det(od, fd, god), (gf, gd), "second call")
    gf2, none = F.cspn2d_nl_sample_backward_det(od, fd, god, need_offset=False)
    none2, gd2 = F.cspn2d_nl_sample_backward_det(od, fd, god, need_f=False)
    assert none is None and none2 is None and torch.equal(gf2, gf) and torch.equal(gd2, gd)
    assert torch.equal(gd, F.cspn2d_nl_sample_backward(od, fd, god, need_f=False)[1])   # grad_offset: the scatter form's kernel, written once
    for t in (od, fd, god):   # a view one element off its boundary
        args = [_misaligned(u) if u is t else u for u in (od, fd, god)]
        _equal(F.cspn2d_nl_sample_backward_det(*args), (gf, gd), "misaligned")


# ---- order independence by construction: a mirrored problem sums the same multiset of terms at every destination, in another order ----
def _exact_problem(H, W, C, sparse, seed):
    """aff multiples of 1/64 in [-1/4, 1/4], offsets multiples of 1/4 in [-3, 3]: every weight, coefficient and c is exact in float32"""
    gen = torch.Generator().manual_seed(seed)
    aff = torch.randint(-16, 17, (B, 8, H, W), generator=gen).float() / 64
    off = torch.randint(-12, 13, (B, 16, H, W), generator=gen).float() / 4
    x = torch.rand(B, C, H, W, generator=gen)
    s = (torch.rand(B, 1, H, W, generator=gen) < 0.1).float() * (torch.rand(B, 1, H, W, generator=gen) * 5 + 0.1) if sparse else None
    go = torch.randn(B, C, H, W, generator=gen) * torch.exp2(torch.randint(-8, 9, (B, C, H, W), generator=gen).float())
    return aff, off, x, s, go


def _mirror(aff, off, x, s, go, axis):
    """axis 3: left-right (planes flipped, dx -> -dx, neighbour (by, bx) <-> (by, -bx)); axis 2: up-down"""
    bs = bases(3)
    perm = [bs.index((by, -bx) if axis == 3 else (-by, bx)) for by, bx in bs]
    fl = lambda t: None if t is None else t.flip(axis).contiguous()   # noqa: E731
    aff2 = fl(aff[:, perm])
    off2 = fl(torch.stack([off[:, 2 * k + j] * (-1.0 if j == (1 if axis == 3 else 0) else 1.0) for k in perm for j in (0, 1)], 1))
    return aff2, off2, fl(x), fl(s), fl(go)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_a_mirrored_problem_gives_the_mirrored_grad_x_bit_for_bit(sparse):
    H, W, C, n = 33, 132, 2, 3
    cpu = _exact_problem(H, W, C, sparse, 4100 + int(sparse))
    assert torch.equal(cpu[0] * 64, (cpu[0] * 64).round()) and torch.equal(cpu[1] * 4, (cpu[1] * 4).round())
    ad, od, xd, sd, god = _cuda(*cpu)
    gx = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, n, 3, None, False, False, True)[2]
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    # the statement on these inputs, for good measure: the mirror of a wrong result would pass the comparison below
    leaf = cpu[2].double().requires_grad_(True)
    nl_levels(cpu[0].double(), cpu[1].double(), leaf, None if cpu[3] is None else cpu[3].double(), n)[-1].backward(cpu[4].double())
    test_nl._grads_close((gx,), (leaf.grad,), ("grad_x",))
    for axis in (3, 2):
        m = _mirror(*cpu, axis)
        # the mirrored problem is the same function: its float64 statement is the mirror
        leaf2 = m[2].double().requires_grad_(True)
        nl_levels(m[0].double(), m[1].double(), leaf2, None if m[3] is None else m[3].double(), n)[-1].backward(m[4].double())
        assert float((leaf2.grad.flip(axis) - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max()), axis
        gm = F.cspn2d_backward_nl_det(*_cuda(*m), n, 3, None, False, False, True)[2]
        assert torch.equal(gm.flip(axis), gx), "axis %d: %d of %d elements differ" % (axis, int((gm.flip(axis) != gx).sum()), gx.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_all_taps_on_one_point(sparse):
    """every tap of every pixel lands at one interior point with fractions (0.25, 0.5): four lists of 8 H W entries per image (32 H W in all), each
    summed by one wave"""
    H, W, C, n = 33, 132, 2, 3
    aff, off, x, s, go = _inputs(H, W, C, sparse, "hot", 5200 + int(sparse))
    leaves = [t.double().requires_grad_(True) for t in (aff, off, x)]
    nl_levels(*leaves, None if s is None else s.double(), n)[-1].backward(go.double())
    ad, od, xd, sd, god = _cuda(aff, off, x, s, go)
    got = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, n)
    test_nl._grads_close(got, [t.grad for t in leaves])
    _equal(F.cspn2d_backward_nl_det(ad, od, xd, sd, god, n), got, "second call")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2])
@pytest.mark.parametrize("sparse", [False, True])
def test_the_edges_of_n_iter_every_gradient_subset_and_no_history(n, sparse):
    H, W, C, kind = 17, 65, 3, "normal"
    c = _case(H, W, C, sparse, kind, n)
    ad, od, xd, sd, god = c["dev"]
    full = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, n, history=c["hist"])
    if n == 0:
        ga, gd, gx = full
        assert torch.equal(gx, god) and not bool(ga.any()) and not bool(gd.any())
        return
    test_nl._grads_close(full, c["ref_grads"])
    for need in itertools.product((False, True), repeat=3):
        for history in (None, c["hist"]):
            got = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, n, 3, history, *need)
            _equal(got, [g if k else None for g, k in zip(full, need)], "need %s" % (need,))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(16, 64), (33, 132), (17, 65)])
@pytest.mark.parametrize("sparse", [False, True])
def test_misaligned_views_and_an_odd_width(H, W, sparse):
    C = 3
    c = _case(H, W, C, sparse, "normal")
    ad, od, xd, sd, god = c["dev"]
    want = F.cspn2d_backward_nl_det(ad, od, xd, sd, god, N_ITER, history=c["hist"])
    test_nl._grads_close(want, c["ref_grads"])
    tensors = [t.cpu() if t is not None else None for t in c["dev"]]
    off = [None if t is None else _misaligned(t.cuda()) for t in tensors]
    variants = [off] + [[(_misaligned(t.cuda()) if j == i else t.cuda()) if t is not None else None for j, t in enumerate(tensors)] for i in range(5)]
    for v in variants:   # all five off their boundary, then each alone: the same bits (the forward's are the aligned call's, test_nl.py)
        _equal(F.cspn2d_backward_nl_det(*v, N_ITER), want, "misaligned")


# ---- the module under torch.use_deterministic_algorithms(True) ----
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_conf", [False, True])
@pytest.mark.parametrize("preserve", [False, True])
def test_module_under_torchs_flag_twice_bitwise_and_vs_fp64_autograd(mode, use_conf, preserve, monkeypatch):
    H, W, C = ((17, 65), (33, 132))[MODES.index(mode) % 2 ^ int(use_conf)] + (2,)
    cpu = test_nl._module_inputs(H, W, C, 40 + MODES.index(mode))
    _, ref_grads = test_nl._module_ref(mode, *cpu, use_conf, preserve, N_ITER)
    calls = []
    for name in BACKWARDS:   # count the calls on their way through
        monkeypatch.setattr(F, name, (lambda f, name: lambda *a, **k: (calls.append(name), f(*a, **k))[1])(getattr(F, name), name))
    dev = _cuda(*cpu)
    try:
        torch.use_deterministic_algorithms(True)
        y1, g1 = test_nl._module_run(mode, *dev, use_conf, preserve, N_ITER)
        y2, g2 = test_nl._module_run(mode, *dev, use_conf, preserve, N_ITER)
    finally:
        torch.use_deterministic_algorithms(False)
    assert set(calls) == ({BACKWARDS[1], BACKWARDS[3]} if use_conf else {BACKWARDS[1]}), calls
    assert len(g1) == len(ref_grads) == 3 + int(use_conf) + int(mode == "TGASS") and all(g is not None for g in g1)
    _equal([y2] + g2, [y1] + g1, "second run")
    test_nl._grads_close(g1, ref_grads, test_nl.MODULE_NAMES)


# ---- memory hygiene: both entry points between guard bands on poisoned workspaces, and in a stale arena ----
def _hygiene_inputs(H, W, C, sparse, kind, seed):
    aff, off, x, s, go = _inputs(H, W, C, sparse, kind, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    f = torch.rand(B, 1, H, W, generator=gen)
    gk = torch.randn(B, 8, H, W, generator=gen)
    return tuple(_cuda(aff, off, x, s, go, f, gk))


def _hygiene_call(aff, off, x, s, go, f, gk):
    n = N_ITER
    _, hist = F.cspn2d_forward_nl(aff, off, x, s, n, return_history=True)
    grads = F.cspn2d_backward_nl_det(aff, off, x, s, go, n, history=hist)
    alone = F.cspn2d_backward_nl_det(aff, off, x, s, go, n, 3, None, False, True, False)[1:2]   # its own forward; no grad_x: the sweep stops at A_1
    only_x = F.cspn2d_backward_nl_det(aff, off, x, s, go, n, 3, None, False, False, True)[2:]
    one = F.cspn2d_backward_nl_det(aff, off, x, s, go, 1)
    sg = F.cspn2d_nl_sample_backward_det(off, f, gk)
    return tuple(grads) + tuple(alone) + tuple(only_x) + tuple(one) + tuple(sg)


HYGIENE = [(33, 132, 3, True, "normal"), (33, 132, 1, False, "hot"), (17, 65, 3, True, "huge"), (5, 8, 1, True, "integer")]


@functools.lru_cache(maxsize=None)
def _hygiene(i):
    """the inputs and the outputs of a clean (unpatched) run, made once"""
    H, W, C, sp, kind = HYGIENE[i]
    inputs = _hygiene_inputs(H, W, C, sp, kind, 950 + W + C)
    clean = _hygiene_call(*inputs)
    torch.cuda.synchronize()
    for t in clean:
        assert bool(torch.isfinite(t).all())
    return inputs, clean


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(HYGIENE)))
@pytest.mark.parametrize("poison", ["ones", "big"])   # NaN poison, finite poison
def test_both_entry_points_between_guard_bands(i, poison):
    """every output, history and workspace lies between guard bands and is poisoned before the call: intact bands, unchanged inputs, outputs bitwise
    the unguarded run's -- so the counts, the cursors and the worklist counter are set by the call, and no level or entry is read before it is
    written"""
    inputs, clean = _hygiene(i)
    H, W, C = HYGIENE[i][:3]
    with contextlib.ExitStack() as stack:
        outs, session = memguard.run_guarded(stack, poison, _hygiene_call, inputs, "cuda", 4 * B * max(C, 16) * H * W)
    assert len(session.workspaces) >= 5 and len(session.guards) > len(session.workspaces)
    memguard.assert_same_outputs(outs, clean, "poison %r" % poison)


@pytest.mark.gpu
def test_stale_arena():
    """a large case, then smaller ones, then the large one again through ONE workspace arena that is never refilled: each call finds the index the
    calls before it left, and still returns the clean bits"""
    order = [0, 1, 2, 3, 0]
    plane = 4 * B * 16 * 33 * 132
    with contextlib.ExitStack() as stack:   # guarded first: this pass has the sizes
        session = memguard.patched(stack, "zero", plane_bytes=plane)
        for i in order:
            _hygiene_call(*_hygiene(i)[0])
            session.check()
        sizes = [n for _, n in session.workspaces]
    assert sizes and max(sizes) > 0
    arena = memguard.Arena(max(sizes), "cuda", plane)
    with contextlib.ExitStack() as stack:
        session = memguard.patched(stack, "stale", arena=arena, plane_bytes=plane)
        for step, i in enumerate(order):
            inputs, clean = _hygiene(i)
            snap = memguard.snapshot(*inputs)
            outs = _hygiene_call(*inputs)
            session.check()
            snap.assert_unchanged()
            memguard.assert_same_outputs(outs, clean, "step %d (case %d) in the stale arena" % (step + 1, i))
    assert arena.taken > 0
