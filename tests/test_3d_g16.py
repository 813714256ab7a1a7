"""fp16 / bf16 gates and guides in the 3D engine (the Paddle contract: norm_type 'none', no mask; the demo module on a raw guide).
The contract is exact widening: a 16-bit gate is widened to float32 where it is read and every operation after that is the float32
kernel's, so outputs and grad_feat are BITWISE the float32 engine's on gate.float() (same shape, alignments, path and algo), and a gate
gradient is the float32 one rounded once to the gate's dtype.
CPU: exports, header, binding table, ABI version, argument errors.  GPU: bitwise against the float32 engine on every path (persistent,
per-step vector and scalar, folding for misaligned views, fused and per-step backward), against float64 torch statements, through the
modules, and the peak memory of a call (no float32 copy of the gates)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from oracle.backward import OFF3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
NEW = ["cspn3d_forward_g16_algo", "cspn3d_forward_multi_g16", "cspn3d_forward_absnorm_g16", "cspn3d_backward_g16_workspace_bytes",
       "cspn3d_backward_g16", "cspn3d_backward_multi_g16_workspace_bytes", "cspn3d_backward_multi_g16", "cspn_gate_absnorm_g16",
       "cspn_gate_absnorm_backward_g16"]
# (B, D, H, W, n): where tests/test_absnorm.py exercises the persistent kernel
PERSISTENT = [(1, 8, 16, 128, 4),    # two tiles in x
              (2, 6, 10, 64, 12),    # two volumes, 12 steps
              (1, 9, 17, 72, 5),     # partial tiles in z, y and x
              (2, 5, 9, 68, 2)]      # the volume seam off a multiple of 8; the minimal n
# where it does not apply
STEPWISE_ONLY = [(1, 6, 10, 66, 4),  # W % 4 != 0
                 (1, 8, 16, 128, 1),  # n = 1
                 (2, 3, 5, 7, 3)]     # small and odd
GFLOOR, GTOL = 5e-6, 2e-4            # the gradient bound of tests/test_backward3d.py and tests/test_absnorm.py on the float32 engine
EPS = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}   # one rounding to nearest, relative to the value


# ---- CPU ----
def test_new_symbols_are_exported_declared_bound_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert s in _lib._SYMBOLS and _lib.symbol(s) is not None, "not in the binding's table: " + s
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION


def test_abi_argument_errors_are_the_float32_twins_without_gpu():
    lib = cspn_amd.load()
    sym = _lib.symbol
    a, b, c, d, e = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))
    ws = ctypes.c_void_p(1 << 30)
    big = 1 << 40
    # forward: every failing argument set gives the twin's code, for both gate types
    f32, g16 = sym("cspn3d_forward_f32_algo"), sym("cspn3d_forward_g16_algo")
    cases = [((a, b, None, c), (0, 2, 4, 8, 3, 2, 0), (ws, big)),      # B = 0: nothing to do
             ((a, b, None, c), (1, 0, 4, 8, 3, 2, 0), (ws, big)),      # bad shape
             ((a, b, None, c), (1, 2, 4, 8, -1, 2, 0), (ws, big)),     # n_iter < 0
             ((a, b, None, c), (1, 2, 4, 8, 3, 2, 7), (ws, big)),      # unknown algo
             ((None, b, None, c), (1, 2, 4, 8, 3, 2, 0), (ws, big)),   # null gate
             ((a, None, None, c), (1, 2, 4, 8, 3, 2, 0), (ws, big)),   # null feat
             ((a, b, None, c), (1, 2, 4, 8, 3, 2, 0), (None, 0)),      # no workspace
             ((a, b, None, c), (1, 2, 4, 8, 3, 2, 0), (ctypes.c_void_p((1 << 30) + 16), big)),   # misaligned workspace
             ((a, b, None, c), (1, 2, 4, 8, 3, 2, 2), (ws, big)),      # persistent requested where it cannot run
             ((a, b, None, c), (1 << 12, 1 << 7, 1 << 7, 1 << 7, 3, 2, 0), (ws, big))]   # beyond 32-bit plane indexing
    for ptrs, ints, tail in cases:
        want = f32(*ptrs, *ints, *tail, None)
        for dt in (1, 2):
            assert g16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want, (ints, tail)
    assert {f32(*p, *i, *t, None) for p, i, t in cases} >= {0, -1, -2, -3}   # (the list does cover the codes)
    ok = ((a, b, None, c), (1, 2, 4, 8, 3, 2, 0), (None, 0))   # fails only at the workspace: every check in front of it passes
    for dt in (0, 3, -1, 16):
        assert g16(a, dt, b, None, c, *ok[1], *ok[2], None) == -1 and b"gate_dtype" in lib.cspn_last_error()
    assert g16(ctypes.c_void_p((1 << 24) + 1), 1, b, None, c, *ok[1], *ok[2], None) == -1 and b"2-byte" in lib.cspn_last_error()
    # the normalising and the masked modes stay float32-only
    for norm in (0, 1):
        assert g16(a, 1, b, None, c, 1, 2, 4, 8, 3, norm, 0, ws, big, None) == -1 and b"Paddle contract" in lib.cspn_last_error()
    assert g16(a, 2, b, d, c, 1, 2, 4, 8, 3, 2, 0, ws, big, None) == -1 and b"Paddle contract" in lib.cspn_last_error()
    # multi-channel forward
    m32, m16 = sym("cspn3d_forward_multi_f32"), sym("cspn3d_forward_multi_g16")
    for ptrs, ints, tail in [((a, b, c), (1, 0, 2, 4, 8, 3), (ws, big)), ((None, b, c), (1, 2, 2, 4, 8, 3), (ws, big)),
                             ((a, b, c), (1, 2, 2, 4, 8, 3), (None, 0)), ((a, b, c), (1, 2, 2, 4, 8, 3), (ws, big))]:
        want = m32(*ptrs, *ints, *tail, None)
        assert want != 0
        for dt in (1, 2):
            assert m16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want
    assert m16(a, 0, b, c, 1, 2, 2, 4, 8, 3, ws, big, None) == -1 and m16(a, 3, b, c, 1, 2, 2, 4, 8, 3, ws, big, None) == -1
    # the demo module
    n32, n16 = sym("cspn3d_forward_absnorm_f32"), sym("cspn3d_forward_absnorm_g16")
    for ptrs, ints, tail in [((None, b, c), (1, 2, 4, 4, 3, 0), (None, 0)), ((a, b, b), (1, 2, 4, 4, 3, 0), (None, 0)),
                             ((a, b, c), (1, 2, 4, 4, 3, 7), (None, 0)), ((a, b, c), (1, 2, 4, 4, 3, 0), (None, 0)),
                             ((a, b, c), (1, 2, 4, 4, -1, 0), (None, 0))]:
        want = n32(*ptrs, *ints, *tail, None)
        assert want != 0
        for dt in (1, 2):
            assert n16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want
    assert n16(a, 0, b, c, 1, 2, 4, 4, 3, 0, None, 0, None) == -1 and n16(a, 3, b, c, 1, 2, 4, 4, 3, 0, None, 0, None) == -1
    # the guide's range is counted in 2-byte elements: out right behind a 16-bit guide does not alias it (behind a float32 one it does)
    V = 2 * 4 * 4
    behind = ctypes.c_void_p((1 << 24) + 26 * V * 2)
    assert n32(a, b, behind, 1, 2, 4, 4, 3, 0, None, 0, None) == -1 and b"alias" in lib.cspn_last_error()
    assert n16(a, 1, b, behind, 1, 2, 4, 4, 3, 0, None, 0, None) == -2
    # backward
    b32, b16 = sym("cspn3d_backward_f32"), sym("cspn3d_backward_g16")
    for ptrs, ints, tail in [((a, b, c, d, e), (1, 2, 4, 8, 3, 0), (ws, big)),     # a normalising mode
                             ((a, b, c, d, e), (1, 2, 0, 8, 3, 2), (ws, big)), ((None, b, c, d, e), (1, 2, 4, 8, 3, 2), (ws, big)),
                             ((a, b, c, d, e), (1, 2, 4, 8, 3, 2), (None, 0)), ((a, b, c, d, e), (1, 2, 4, 8, -2, 2), (ws, big))]:
        want = b32(*ptrs, *ints, *tail, None)
        assert want != 0
        for dt in (1, 2):
            assert b16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want
    assert b16(a, 0, b, c, d, e, 1, 2, 4, 8, 3, 2, ws, big, None) == -1 and b16(a, 3, b, c, d, e, 1, 2, 4, 8, 3, 2, ws, big, None) == -1
    assert b16(a, 1, b, c, ctypes.c_void_p((4 << 24) + 1), e, 1, 2, 4, 8, 3, 2, ws, big, None) == -1   # an odd grad_gate address
    bm32, bm16 = sym("cspn3d_backward_multi_f32"), sym("cspn3d_backward_multi_g16")
    assert bm16(a, 2, b, c, d, e, 1, 0, 2, 4, 8, 3, ws, big, None) == bm32(a, b, c, d, e, 1, 0, 2, 4, 8, 3, ws, big, None) == -1
    assert bm16(a, 0, b, c, d, e, 1, 2, 2, 4, 8, 3, ws, big, None) == -1
    # workspace queries: never smaller than the float32 twins'; where the fused sweeps can run, the float32 copy of the gates on top
    w32, w16 = lib.cspn3d_backward_workspace_bytes, sym("cspn3d_backward_g16_workspace_bytes")
    wm32, wm16 = sym("cspn3d_backward_multi_workspace_bytes"), sym("cspn3d_backward_multi_g16_workspace_bytes")
    w32.restype = ctypes.c_size_t
    assert w16(0, 4, 8, 16, 3) == 0 and w16(1, 4, 8, 16, 0) == 0 and wm16(1, 0, 4, 8, 16, 3) == 0
    assert w16(2, 4, 8, 16, 1) == w32(2, 4, 8, 16, 1) and w16(2, 3, 5, 7, 3) == w32(2, 3, 5, 7, 3)   # n = 1; W % 4 != 0: no fused sweeps
    assert w16(2, 4, 8, 16, 3) >= w32(2, 4, 8, 16, 3) and wm16(2, 3, 4, 8, 16, 3) >= wm32(2, 3, 4, 8, 16, 3)
    # the normaliser's 16-bit forms: K = 26 only, the twins' checks
    g32, g16n = sym("cspn_gate_absnorm_f32"), sym("cspn_gate_absnorm_g16")
    gb32, gb16 = sym("cspn_gate_absnorm_backward_f32"), sym("cspn_gate_absnorm_backward_g16")
    assert g16n(a, 1, b, 2, 8, 64, None) == -1 and b"K must be 26" in lib.cspn_last_error()
    assert g16n(a, 0, b, 2, 26, 64, None) == -1 and g16n(a, 3, b, 2, 26, 64, None) == -1
    assert g16n(None, 1, b, 2, 26, 64, None) == g32(None, b, 2, 26, 64, None) == -1
    assert g16n(a, 2, a, 2, 26, 64, None) == g32(a, a, 2, 26, 64, None) == -1 and b"alias" in lib.cspn_last_error()
    assert g16n(a, 2, b, 0, 26, 64, None) == g32(a, b, 0, 26, 64, None) == -1
    assert gb16(a, 1, b, a, 1, 26, 16, None) == gb32(a, b, a, 1, 26, 16, None) == -1
    assert gb16(a, 1, None, c, 1, 26, 16, None) == gb32(a, None, c, 1, 26, 16, None) == -1
    assert gb16(a, 0, b, c, 1, 26, 16, None) == -1 and gb16(a, 1, b, c, 1, 24, 16, None) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_entry_points_exist_and_raise_without_gpu(dtype):
    """what the K x K 16-bit paths raise for a CPU tensor: shape errors first, then "GPU-only" """
    g, x = torch.rand(1, 26, 2, 4, 8).to(dtype), torch.rand(1, 1, 2, 4, 8)
    for f in (F.cspn3d_forward, F.cspn3d_forward_multi, F.cspn3d_backward, F.cspn3d_backward_multi, F.cspn3d_forward_absnorm):
        assert callable(f)
    with pytest.raises(ValueError, match="gate must be"):
        F.cspn3d_forward(g[:, :25], x, None, 3, "none")
    with pytest.raises(ValueError, match="gate must be"):
        F.cspn3d_backward(g[:, :25], x, x, 3)
    with pytest.raises(ValueError, match="guide must be"):
        F.cspn3d_forward_absnorm(g[:, :25], x, 3)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_forward(g, x, None, 3, "none")
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_forward_multi(g, x.repeat(1, 2, 1, 1, 1), 3)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_backward(g, x, x, 3)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_backward_multi(g, x.repeat(1, 2, 1, 1, 1), x.repeat(1, 2, 1, 1, 1), 3)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_forward_absnorm(g, x, 3)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        cspn_amd.affinity_propagate(x, g, 3, 2)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        cspn_amd.CSPN(3, 1, 3, 2)(g, x.to(dtype))


@pytest.mark.gpu
def test_float64_and_the_normalising_modes_still_raise_typeerror_on_the_device():
    """(on a CPU tensor the engine reports the device first, so the dtype errors can only be seen with device tensors)"""
    g, x = torch.rand(1, 26, 2, 4, 8, device="cuda"), torch.rand(1, 1, 2, 4, 8, device="cuda")
    for f in (lambda t: F.cspn3d_forward(t, x, None, 3, "none"), lambda t: F.cspn3d_forward_multi(t, x, 3), lambda t: F.cspn3d_backward(t, x, x, 3),
              lambda t: F.cspn3d_backward_multi(t, x, x, 3), lambda t: F.cspn3d_forward_absnorm(t, x, 3), lambda t: cspn_amd.affinity_propagate(x, t, 3, 2)):
        with pytest.raises(TypeError, match="float32"):
            f(g.double())
    with pytest.raises(TypeError, match="float32"):
        F.cspn3d_forward(g.half(), x.double(), None, 3, "none")
    for dtype in DTYPES:
        for norm in ("8sum", "8sum_abs"):
            with pytest.raises(TypeError, match="float32"):
                F.cspn3d_forward(g.to(dtype), x, None, 3, norm)
        with pytest.raises(TypeError, match="float32"):
            F.cspn3d_forward(g.to(dtype), x, (x > 0.5).float(), 3, "none")
        with pytest.raises(TypeError, match="float32"):
            cspn_amd.gate_absnorm(g.to(dtype), 26)   # the public tensor op stays float32-only (tests/test_absnorm.py)


# ---- GPU: inputs (made once per shape on the CPU generator, shared, never modified) ----
@functools.lru_cache(maxsize=None)
def _inputs(B, D, H, W, dtype, C=1, zero_voxel=True):
    """gates: randn, normalised by their abs-sum (so: negative ones too), one plane scaled by 2^-20 (float16 subnormals), exact zeros,
    and -- where the test does not normalise -- one all-zero voxel; rounded to dtype.  feat, grad_out float32"""
    gen = torch.Generator().manual_seed(1000 * B + 100 * D + 10 * H + W)
    g = torch.randn(B, 26, D, H, W, generator=gen)
    g = g / g.abs().sum(1, keepdim=True)
    g[:, 5] *= 2.0 ** -20
    g.view(-1)[::97] = 0.0
    if zero_voxel:
        g[0, :, D // 2, H // 2, W // 2] = 0.0
    h = torch.rand(B, C, D, H, W, generator=gen)
    go = torch.randn(B, C, D, H, W, generator=gen)
    g16 = g.to(dtype).cuda()
    if dtype == torch.float16:
        sub = g16[:, 5].float().abs()
        assert bool(((sub > 0) & (sub < 2.0 ** -14)).any()), "no float16 subnormal among the gates"
    return g16, h.cuda(), go.cuda()


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(torch.nan_to_num(a.float(), nan=123.0), torch.nan_to_num(b.float(), nan=123.0))


def _offset_view(t):
    """the same values one element off the allocation's alignment (2 bytes for a 16-bit tensor, 4 for float32)"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


# ---- GPU forward, NONE op ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["persistent", "stepwise"])
@pytest.mark.parametrize("shape", PERSISTENT)
def test_none_forward_is_bitwise_the_float32_engine(dtype, algo, shape):
    B, D, H, W, n = shape
    g, h, _ = _inputs(B, D, H, W, dtype)
    out = F.cspn3d_forward(g, h, None, n, "none", algo)
    F.cspn3d_check_status()
    ref = F.cspn3d_forward(g.float(), h, None, n, "none", algo)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STEPWISE_ONLY)
def test_none_forward_auto_where_the_persistent_kernel_does_not_apply(dtype, shape):
    B, D, H, W, n = shape
    g, h, _ = _inputs(B, D, H, W, dtype)
    out = F.cspn3d_forward(g, h, None, n, "none")
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and torch.equal(out, F.cspn3d_forward(g.float(), h, None, n, "none"))
    with pytest.raises(_lib.CspnError):
        F.cspn3d_forward(g, h, None, n, "none", "persistent")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_none_forward_on_a_view_two_bytes_off(dtype):
    B, D, H, W, n = PERSISTENT[0]
    g, h, _ = _inputs(B, D, H, W, dtype)
    out = F.cspn3d_forward(_offset_view(g), h, None, n, "none")
    F.cspn3d_check_status()
    ref = F.cspn3d_forward(_offset_view(g.float()), h, None, n, "none")
    F.cspn3d_check_status()
    assert torch.equal(out, ref)
    assert torch.equal(out, F.cspn3d_forward(g, h, None, n, "none"))   # (the folding path computes the same sums in the same order)
    F.cspn3d_check_status()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_multi_channel_forward_is_bitwise_the_float32_engine(dtype):
    B, D, H, W, n = PERSISTENT[1]
    g, h, _ = _inputs(B, D, H, W, dtype, C=3)
    out = F.cspn3d_forward_multi(g, h, n)
    F.cspn3d_check_status()
    ref = F.cspn3d_forward_multi(g.float(), h, n)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    # a 16-bit value tensor is widened with one cast
    assert torch.equal(F.cspn3d_forward_multi(g, h.to(dtype), n), F.cspn3d_forward_multi(g.float(), h.to(dtype).float(), n))
    F.cspn3d_check_status()


# ---- GPU forward, the demo module ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("algo", ["persistent", "stepwise"])
@pytest.mark.parametrize("shape", PERSISTENT)
def test_demo_module_forward_is_bitwise_the_float32_engine(dtype, algo, shape):
    B, D, H, W, n = shape
    g, h, _ = _inputs(B, D, H, W, dtype, zero_voxel=False)
    out = F.cspn3d_forward_absnorm(g, h, n, algo)
    F.cspn3d_check_status()
    ref = F.cspn3d_forward_absnorm(g.float(), h, n, algo)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and _same(out, ref)
    assert bool(torch.isfinite(out).any())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_demo_module_forward_auto_off_the_persistent_kernel_and_on_an_offset_view(dtype):
    B, D, H, W, n = STEPWISE_ONLY[0]
    g, h, _ = _inputs(B, D, H, W, dtype, zero_voxel=False)
    assert _same(F.cspn3d_forward_absnorm(g, h, n), F.cspn3d_forward_absnorm(g.float(), h, n))
    B, D, H, W, n = PERSISTENT[0]
    g, h, _ = _inputs(B, D, H, W, dtype, zero_voxel=False)
    out = F.cspn3d_forward_absnorm(_offset_view(g), h, n)
    F.cspn3d_check_status()
    ref = F.cspn3d_forward_absnorm(_offset_view(g.float()), h, n)
    F.cspn3d_check_status()
    assert _same(out, ref)


# ---- GPU backward ----
def _backward_pair(dtype, B, D, H, W, n, C=1, **kw):
    g, h, go = _inputs(B, D, H, W, dtype, C=C)
    fn = F.cspn3d_backward if C == 1 else F.cspn3d_backward_multi
    gg, gf = fn(g, h, go, n, **kw)
    F.cspn3d_check_status()
    rg, rf = fn(g.float(), h, go, n, **kw)
    F.cspn3d_check_status()
    return gg, gf, rg, rf


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 8, 16, 128, 1), (1, 8, 16, 128, 2), (1, 8, 16, 128, 4),
                                   (2, 6, 10, 64, 12),      # the fused sweeps: level-keeping 16-bit forward, widened transposed sweep
                                   (2, 3, 5, 7, 3), (1, 6, 10, 66, 4)])
def test_backward_is_the_float32_engine_rounded_once(dtype, shape):
    gg, gf, rg, rf = _backward_pair(dtype, *shape)
    assert gg.dtype == dtype and gf.dtype == torch.float32
    assert torch.equal(gf, rf)
    assert _same(gg, rg.to(dtype))
    assert float(gg.float().abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_multi_and_either_output_alone(dtype):
    gg, gf, rg, rf = _backward_pair(dtype, 2, 6, 10, 64, 4, C=2)
    assert gg.dtype == dtype and torch.equal(gf, rf) and _same(gg, rg.to(dtype))
    gg1, none, rg1, _ = _backward_pair(dtype, 2, 6, 10, 64, 4, need_feat=False)
    assert none is None and _same(gg1, rg1.to(dtype))
    none, gf1, _, rf1 = _backward_pair(dtype, 2, 6, 10, 64, 4, need_gate=False)
    assert none is None and torch.equal(gf1, rf1)
    # a 16-bit grad_out / feat is widened with one cast
    g, h, go = _inputs(2, 6, 10, 64, dtype)
    a = F.cspn3d_backward(g, h.to(dtype), go.to(dtype), 4)
    b = F.cspn3d_backward(g.float(), h.to(dtype).float(), go.to(dtype).float(), 4)
    assert torch.equal(a[1], b[1]) and _same(a[0], b[0].to(dtype))


# ---- GPU: against truth, not only against itself ----
def _torch_none3d(w, h, n_iter):
    """H_{t+1}(p) = sum_k w_k(p) H_t(p + off_k), zero outside (tests/test_backward3d.py::_torch_forward, tests/test_absnorm.py)"""
    B, _, D, H, W = w.shape
    x = h[:, 0]
    for _ in range(n_iter):
        pad = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))
        acc = 0
        for k, (dz, dy, dx) in enumerate(OFF3):
            acc = acc + w[:, k] * pad[:, 1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        x = acc
    return x[:, None]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(1, 9, 17, 72, 5), (1, 6, 10, 66, 4)])
def test_against_the_float64_statements(dtype, shape):
    """The float64 recurrence on the WIDENED gates.  Forward and grad_feat: the float32 engine's bounds (1e-6 max-norm; GFLOOR / GTOL
    element-wise).  Gate gradient: the same bound plus one rounding to the dtype, |r(v) - ref| <= |v - ref| + eps |v| with
    |v| <= |ref| + |v - ref|, i.e. (1 + eps) bound32 + eps |ref|, eps = 2^-11 (float16) or 2^-8 (bfloat16).
    Gates, feat and grad_out are positive and away from 0, so every gradient is 0 (a neighbour outside the volume) or far above the
    float16 subnormal range, where the rounding is no longer relative."""
    from helpers import assert_close
    B, D, H, W, n = shape
    gen = torch.Generator().manual_seed(77 + W)
    g = torch.rand(B, 26, D, H, W, generator=gen) + 0.1
    g = (g / g.sum(1, keepdim=True)).to(dtype)
    h = torch.rand(B, 1, D, H, W, generator=gen) + 0.5
    go = 16.0 * (torch.rand(B, 1, D, H, W, generator=gen) + 0.5)
    gt, ht = g.double().requires_grad_(True), h.double().requires_grad_(True)
    ref = _torch_none3d(gt, ht, n)
    ref.backward(go.double())
    out = F.cspn3d_forward(g.cuda(), h.cuda(), None, n, "none")
    gg, gf = F.cspn3d_backward(g.cuda(), h.cuda(), go.cuda(), n)
    F.cspn3d_check_status()
    e_out = _rel(out.cpu().numpy(), ref.detach().numpy())
    print("forward rel err %.3g" % e_out)
    assert e_out <= 1e-6
    assert_close(gf.cpu().numpy(), ht.grad.numpy(), "grad_feat", rtol=GTOL, atol_frac=GFLOOR)
    a, b = gg.float().cpu().double().numpy(), gt.grad.numpy()
    nz = np.abs(b[b != 0])
    assert nz.min() > 2.0 ** -13, "a gradient near the float16 subnormal range: the test's inputs are wrong"
    eps = EPS[dtype]
    scale = np.abs(b).max()
    bound = (1 + eps) * (GFLOOR * scale + GTOL * np.abs(b)) + eps * np.abs(b)
    worst = float((np.abs(a - b) / bound).max())
    print("grad_gate worst excess %.3g, max-norm %.3g" % (worst, _rel(a, b)))
    assert worst <= 1.0 and _rel(a, b) <= (1 + eps) * GTOL + eps
    assert gg.dtype == dtype


# ---- GPU: the modules ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_demo_module_trains_on_a_16_bit_guide(dtype):
    B, D, H, W = 2, 6, 10, 64
    gen = torch.Generator().manual_seed(5)
    guide = torch.randn(B, 52, D, H, W, generator=gen).to(dtype).cuda()
    feat = torch.rand(B, 2, D, H, W, generator=gen).cuda()
    go = torch.randn(B, 2, D, H, W, generator=gen).cuda()
    m = cspn_amd.CSPN(3, 2, 3, 4)
    g16, f16 = guide.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    g32, f32 = guide.float().detach().requires_grad_(True), feat.clone().requires_grad_(True)
    out = m(g16, f16)
    out.backward(go)
    ref = m(g32, f32)
    ref.backward(go)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    assert g16.grad.dtype == dtype and _same(g16.grad, g32.grad.to(dtype)) and torch.equal(f16.grad, f32.grad)
    assert bool(torch.isfinite(g16.grad.float()).all()) and float(g16.grad.float().abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 2])
def test_affinity_propagate_trains_on_16_bit_gates(dtype, C):
    B, D, H, W, n = 2, 6, 10, 64, 4
    g, h, go = _inputs(B, D, H, W, dtype, C=C)
    g16, x16 = g.clone().requires_grad_(True), h.clone().requires_grad_(True)
    g32, x32 = g.float().detach().requires_grad_(True), h.clone().requires_grad_(True)
    out = cspn_amd.affinity_propagate(x16, g16, 3, n)
    out.backward(go)
    ref = cspn_amd.affinity_propagate(x32, g32, 3, n)
    ref.backward(go)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and torch.equal(out, ref)
    assert g16.grad.dtype == dtype and _same(g16.grad, g32.grad.to(dtype)) and torch.equal(x16.grad, x32.grad)
    with torch.no_grad():
        assert torch.equal(cspn_amd.affinity_propagate(h, g, 3, n), ref)


# ---- GPU: no float32 copy of the gates ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_float32_copy_of_the_gates_is_made(dtype):
    """the peak of a call on 16-bit gates is the float32 call's on pre-widened gates (+ 4 MiB: two 2-MiB allocator blocks); widening
    the gates first would add their 13.6 MB"""
    gen = torch.Generator(device="cuda").manual_seed(9)
    g = torch.rand(2, 26, 16, 32, 128, device="cuda", generator=gen)
    g16 = (g / g.sum(1, keepdim=True)).to(dtype)
    g32 = g16.float()
    x = torch.rand(2, 1, 16, 32, 128, device="cuda", generator=gen)
    del g
    assert g32.numel() * 4 > 13e6

    def rise(gates):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = cspn_amd.affinity_propagate(x, gates, 3, 4)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, out

    with torch.no_grad():
        rise(g32), rise(g16)   # (first calls: the library's own one-time allocations)
        r32, o32 = rise(g32)
        r16, o16 = rise(g16)
    F.cspn3d_check_status()
    print("peak rise: float32 %d B, 16-bit %d B" % (r32, r16))
    assert torch.equal(o16, o32)
    assert r16 <= r32 + (4 << 20)
