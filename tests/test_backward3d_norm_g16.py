"""fp16 / bf16 guidance in the 3D normalising and masked modes (cspn3d_forward_norm_g16, cspn3d_backward_norm_g16,
cspn_amd.cspn3d_forward_norm, cspn_amd.cspn3d_backward_norm, cspn_amd.Affinity_Propagate3d).
The contract is the exact widening of every other *_g16 path: a 16-bit gate is widened where a kernel reads it and everything after that is
the float32 kernel's, so out and grad_feat are BITWISE the float32 engine's on guidance.float() (same algo, same alignment class) and
grad_guidance is the float32 one rounded once to the guidance's dtype; NaNs are matched position for position.
CPU: exports, header, bindings, the argument errors of the float32 twins, the workspace query, what CPU tensors raise.
GPU: the comparisons above on every kernel variant, alignment class, special values, partial calls and through the module."""
import ctypes
import functools
import os
import re

import pytest
import torch

import cspn_amd
from cspn_amd import _lib
from cspn_amd import functional as F
from oracle.backward import OFF3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
NEW = ["cspn3d_forward_norm_g16", "cspn3d_backward_norm_g16_workspace_bytes", "cspn3d_backward_norm_g16"]
# mode = (norm_type, mask): the normalising modes with the three mask settings of tests/test_backward3d_norm.py, 'none' with a mask
MODES = [(norm, mask) for norm in ("8sum", "8sum_abs") for mask in ("nomask", "mask", "mask_neg")] + [("none", "mask"), ("none", "mask_neg")]
# (B, D, H, W), n_iter
CASES = [((2, 4, 5, 7), 1),      # odd W: the VEC = 1 kernels; B = 2: the batch stride in 2-byte elements
         ((1, 3, 6, 8), 4),      # VEC = 4; every quad touches a row edge (guarded path); shifted 8-byte loads at 2-byte alignment
         ((2, 6, 10, 36), 12),   # VEC = 4, interior quads, several workgroups, many levels
         ((1, 1, 3, 4), 2)]      # D = 1, W = 4: every z neighbour and both x edges out of range in the same quad
FUSED_CASES = [((1, 8, 8, 64), 3),    # algo 'auto' runs the adjoint sweep in the persistent kernel's transposed instance: one tile
               ((1, 9, 17, 72), 5)]   # partial tiles


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_new_symbols_are_exported_declared_bound_and_the_abi_stays_5():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cspn_amd.h")).read(), flags=re.S)
    lib = cspn_amd.load()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, text), "not declared: " + s
        assert hasattr(lib, s), "not exported: " + s
        assert s in _lib._SYMBOLS and _lib.symbol(s) is not None, "not in the binding's table: " + s
    assert lib.cspn_abi_version() == 5 == _lib.ABI_VERSION and "#define CSPN_ABI_VERSION 5" in text
    assert "cspn3d_forward_norm" in cspn_amd.__all__ and callable(cspn_amd.cspn3d_forward_norm)


def test_abi_argument_errors_are_the_float32_twins_without_gpu():
    """every call below returns before a launch: the pointers are never dereferenced"""
    lib = cspn_amd.load()
    sym = _lib.symbol
    a, b, c, d, e, f = (ctypes.c_void_p((k + 1) << 32) for k in range(6))   # far apart: no range overlaps another
    ws = ctypes.c_void_p(7 << 32)
    big = 1 << 40
    # ---- forward: (gate, feat, sparse, out), (B, D, H, W, n_iter, norm, algo), (ws, bytes)
    f32, g16 = sym("cspn3d_forward_f32_algo"), sym("cspn3d_forward_norm_g16")
    cases = [((a, b, c, d), (0, 2, 4, 8, 3, 1, 0), (ws, big)),       # B = 0: nothing to do
             ((a, b, c, d), (1, 0, 4, 8, 3, 1, 0), (ws, big)),       # bad shape
             ((a, b, None, d), (1, 2, 4, 8, -1, 0, 0), (ws, big)),   # n_iter < 0
             ((a, b, c, d), (1, 2, 4, 8, 3, 1, 7), (ws, big)),       # unknown algo
             ((a, b, c, d), (1, 2, 4, 8, 3, 7, 0), (ws, big)),       # unknown norm
             ((a, b, c, d), (1, 2, 4, 8, 3, 3, 0), (ws, big)),       # PRENORM: the 2D entry points' only
             ((None, b, c, d), (1, 2, 4, 8, 3, 1, 0), (ws, big)),    # null guidance
             ((a, None, c, d), (1, 2, 4, 8, 3, 0, 0), (ws, big)),    # null feat
             ((a, b, c, None), (1, 2, 4, 8, 3, 2, 0), (ws, big)),    # null out
             ((a, b, c, d), (1, 2, 4, 8, 3, 1, 0), (None, 0)),       # no workspace
             ((a, b, None, d), (1, 2, 4, 8, 3, 0, 0), (ws, 1024)),   # workspace too small
             ((a, b, c, d), (1, 2, 4, 8, 3, 1, 0), (ctypes.c_void_p((7 << 32) + 16), big)),   # misaligned workspace
             ((a, b, None, d), (1, 2, 4, 8, 3, 2, 2), (ws, big)),    # persistent requested where it cannot run (the Paddle contract: before any launch)
             ((a, b, c, d), (1 << 12, 1 << 7, 1 << 7, 1 << 7, 3, 1, 0), (ws, big))]   # beyond 32-bit plane indexing
    for ptrs, ints, tail in cases:
        want = f32(*ptrs, *ints, *tail, None)
        for dt in (1, 2):
            assert g16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want, (ints, tail)
    assert {f32(*p, *i, *t, None) for p, i, t in cases} == {0, -1, -2, -3}   # (the list does cover the codes, and nothing was launched)
    ok = ((1, 2, 4, 8, 3, 1, 0), (None, 0))   # fails only at the workspace: every check in front of it passes
    assert g16(a, 1, b, c, d, *ok[0], *ok[1], None) == -2
    for dt in (0, 3, -1):
        assert g16(a, dt, b, c, d, *ok[0], *ok[1], None) == -1 and b"gate_dtype" in lib.cspn_last_error()
    assert g16(ctypes.c_void_p((1 << 32) + 1), 1, b, c, d, *ok[0], *ok[1], None) == -1 and b"2-byte" in lib.cspn_last_error()
    # cspn3d_forward_g16_algo keeps refusing these modes (tests/test_3d_g16.py)
    assert sym("cspn3d_forward_g16_algo")(a, 1, b, None, d, 1, 2, 4, 8, 3, 1, 0, ws, big, None) == -1 and b"Paddle contract" in lib.cspn_last_error()

    # ---- backward: (guidance, feat, sparse, grad_out, grad_guidance, grad_feat), (B, D, H, W, n_iter, norm, algo), (ws, bytes)
    b32, b16 = sym("cspn3d_backward_norm_f32"), sym("cspn3d_backward_norm_g16")
    cases = [((a, b, c, d, e, f), (0, 2, 2, 4, 2, 1, 0), (ws, big)),       # B = 0
             ((a, b, c, d, e, f), (1, 0, 2, 4, 2, 1, 0), (ws, big)),       # bad shape
             ((a, b, c, d, e, f), (1, 2, 2, -3, 2, 0, 0), (ws, big)),
             ((a, b, c, d, e, f), (1, 2, 2, 4, -1, 1, 0), (ws, big)),      # n_iter < 0
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 1, 5), (ws, big)),       # unknown algo
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 7, 0), (ws, big)),       # unknown norm
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 3, 0), (ws, big)),       # PRENORM
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, -1, 0), (ws, big)),
             ((None, b, c, d, e, f), (1, 2, 2, 4, 2, 1, 0), (ws, big)),    # null guidance
             ((a, None, c, d, e, f), (1, 2, 2, 4, 2, 0, 0), (ws, big)),    # null feat
             ((a, b, c, None, e, f), (1, 2, 2, 4, 2, 2, 0), (ws, big)),    # null grad_out
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 1, 0), (None, 0)),       # no workspace
             ((a, b, None, d, e, f), (1, 2, 2, 4, 2, 0, 0), (ws, 1024)),   # workspace too small
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 1, 0), (ctypes.c_void_p((7 << 32) + 64), big)),   # misaligned workspace
             ((a, b, c, d, a, f), (1, 2, 2, 4, 2, 1, 0), (ws, big)),       # grad_guidance on the guidance
             ((a, b, c, d, e, b), (1, 2, 2, 4, 2, 1, 0), (ws, big)),       # grad_feat on feat
             ((a, b, c, d, e, ws), (1, 2, 2, 4, 2, 1, 0), (ws, big)),      # grad_feat on the workspace
             ((a, b, c, d, None, None), (1, 2, 2, 4, 2, 1, 0), (ws, big)),  # nothing asked for: nothing launched
             ((a, b, c, d, None, None), (1, 2, 2, 4, 0, 1, 0), (ws, big)),
             ((a, b, c, d, e, f), (1, 2, 2, 4, 2, 1, 2), (ws, big)),       # persistent where 'auto' would not fuse the sweep (n_iter < 3)
             ((a, b, None, d, e, f), (1, 2, 2, 4, 2, 2, 2), (ws, big)),    # the same for the Paddle contract
             ((a, b, c, d, e, f), (1 << 12, 1 << 7, 1 << 7, 1 << 7, 3, 1, 0), (ws, big))]   # beyond 32-bit plane indexing
    for ptrs, ints, tail in cases:
        want = b32(*ptrs, *ints, *tail, None)
        for dt in (1, 2):
            assert b16(ptrs[0], dt, *ptrs[1:], *ints, *tail, None) == want, (ints, tail)
    assert {b32(*p, *i, *t, None) for p, i, t in cases} == {0, -1, -2, -3}
    ok = ((1, 2, 2, 4, 2, 1, 0), (None, 0))
    assert b16(a, 2, b, c, d, e, f, *ok[0], *ok[1], None) == -2
    for dt in (0, 3, -1):
        assert b16(a, dt, b, c, d, e, f, *ok[0], *ok[1], None) == -1 and b"gate_dtype" in lib.cspn_last_error()
    assert b16(ctypes.c_void_p((1 << 32) + 1), 1, b, c, d, e, f, *ok[0], *ok[1], None) == -1 and b"2-byte" in lib.cspn_last_error()
    assert b16(a, 1, b, c, d, ctypes.c_void_p((5 << 32) + 1), f, *ok[0], *ok[1], None) == -1 and b"2-byte" in lib.cspn_last_error()
    # the guidance's range is counted in 2-byte elements: an output right behind a 16-bit guidance does not alias it (the call gets as far as
    # the refusal of algo 'persistent' for n_iter = 2), behind a float32 guidance it does
    V = 2 * 2 * 4
    behind = ctypes.c_void_p((1 << 32) + 26 * V * 2)
    for outs in ((e, behind), (behind, f)):
        assert b32(a, b, c, d, *outs, 1, 2, 2, 4, 2, 1, 2, ws, big, None) == -1 and b"overlap" in lib.cspn_last_error()
        for dt in (1, 2):
            assert b16(a, dt, b, c, d, *outs, 1, 2, 2, 4, 2, 1, 2, ws, big, None) == -3 and b"persistent" in lib.cspn_last_error()
    # ... and the gradient's own range too: grad_feat right behind a 16-bit grad_guidance
    behind_gg = ctypes.c_void_p((5 << 32) + 26 * V * 2)
    assert b32(a, b, c, d, e, behind_gg, 1, 2, 2, 4, 2, 1, 2, ws, big, None) == -1
    assert b16(a, 1, b, c, d, e, behind_gg, 1, 2, 2, 4, 2, 1, 2, ws, big, None) == -3
    assert b16(a, 1, b, c, d, e, ctypes.c_void_p((5 << 32) + 26 * V * 2 - 4), 1, 2, 2, 4, 2, 1, 2, ws, big, None) == -1


def test_workspace_query_is_the_float32_one():
    """everything in the workspace of the normalising and masked modes is float32, so the 16-bit call needs exactly the float32 call's bytes.
    'none' without a mask is forwarded to cspn3d_backward_g16, whose workspace keeps the widened gates of its transposed sweep"""
    q32, q16 = _lib.symbol("cspn3d_backward_norm_workspace_bytes"), _lib.symbol("cspn3d_backward_norm_g16_workspace_bytes")
    paddle16 = _lib.symbol("cspn3d_backward_g16_workspace_bytes")
    for dims in ((2, 4, 5, 7), (1, 3, 6, 8), (2, 6, 10, 36), (1, 1, 3, 4), (1, 8, 8, 64), (1, 9, 17, 72), (4, 32, 160, 608)):
        for n in (1, 2, 3, 12):
            for norm, has_sparse in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1)):
                assert q16(*dims, n, norm, has_sparse) == q32(*dims, n, norm, has_sparse) > 0
            assert q16(*dims, n, 2, 0) == paddle16(*dims, n) >= q32(*dims, n, 2, 0)
    assert q16(0, 4, 8, 16, 3, 1, 0) == 0 and q16(1, 4, 8, 16, 0, 1, 0) == 0 and q16(1, 4, 8, 16, 3, 3, 0) == 0 and q16(1, 4, 8, 16, 3, -1, 1) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_tensors_raise_shape_errors_first_then_gpu_only(dtype):
    g, x = torch.rand(1, 26, 2, 4, 8).to(dtype), torch.rand(1, 1, 2, 4, 8)
    with pytest.raises(ValueError, match="guidance must be"):
        F.cspn3d_forward_norm(g[:, :25], x, None, 3, "8sum")
    with pytest.raises(ValueError, match="guidance must be"):
        F.cspn3d_backward_norm(g[:, :25], x, None, x, 3, "8sum")
    with pytest.raises(ValueError, match="guidance must be"):
        cspn_amd.Affinity_Propagate3d(3)(g[:, :25], x)
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_forward_norm(g, x, None, 3, "8sum_abs")
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_forward_norm(g, x, x, 3, "none")
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        F.cspn3d_backward_norm(g, x, None, x, 3, "8sum_abs")
    with pytest.raises(_lib.CspnError, match="GPU-only"):
        cspn_amd.Affinity_Propagate3d(3)(g, x, x)
    assert cspn_amd.Affinity_Propagate3d(3)(g, x, None, n_iter=0) is x


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _make(shape, seed, mask, dtype):
    """the inputs of tests/test_backward3d_norm.py, made on the CPU generator: guidance (rand - 0.3) cast to dtype (both signs)"""
    B, D, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    g = (torch.rand(B, 26, D, H, W, generator=gen) - 0.3).to(dtype)
    feat = torch.rand(B, 1, D, H, W, generator=gen)
    go = torch.randn(B, 1, D, H, W, generator=gen)
    sparse = None
    if mask != "nomask":
        sparse = (torch.rand(B, 1, D, H, W, generator=gen) < 0.2).float() * (feat + 0.1)
        sparse.view(-1)[0] = 1.5   # at least one pinned voxel at every size
        if mask == "mask_neg":
            sparse.view(-1)[-1] = -2.0   # m = -1, u = 2
    return g, feat, sparse, go


@functools.lru_cache(maxsize=None)
def _inputs(shape, n_iter, mask, dtype):
    """on the device, shared and never modified: (guidance in dtype, feat, sparse or None, grad_out)"""
    return tuple(None if t is None else t.cuda() for t in _make(shape, 31 + n_iter, mask, dtype))


@functools.lru_cache(maxsize=None)
def _reference(shape, n_iter, norm, mask, dtype, algo):
    """the float32 engine on guidance.float(): (out, grad_guidance, grad_feat), computed once per case"""
    g, feat, sparse, go = _inputs(shape, n_iter, mask, dtype)
    g32 = g.float()
    out = F.cspn3d_forward(g32, feat, sparse, n_iter, norm, algo)
    gg, gf = F.cspn3d_backward_norm(g32, feat, sparse, go, n_iter, norm, algo)
    F.cspn3d_check_status()
    return out, gg, gf


def _bitwise(a, b):
    """same dtype, same bits wherever neither is NaN, NaN exactly where the other has one"""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    ints = torch.int32 if a.dtype == torch.float32 else torch.int16
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and ((a.contiguous().view(ints) == b.contiguous().view(ints)) | na).all())


def _assert_case(shape, n_iter, norm, mask, dtype, algo):
    g, feat, sparse, go = _inputs(shape, n_iter, mask, dtype)
    ref_out, ref_gg, ref_gf = _reference(shape, n_iter, norm, mask, dtype, algo)
    out = F.cspn3d_forward_norm(g, feat, sparse, n_iter, norm, algo)
    gg, gf = F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm, algo)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and gf.dtype == torch.float32 and gg.dtype == dtype
    assert _bitwise(out, ref_out), "out"
    assert _bitwise(gf, ref_gf), "grad_feat"
    assert _bitwise(gg, ref_gg.to(dtype)), "grad_guidance"
    assert bool(torch.isfinite(out).all()) and float(gg.float().abs().max()) > 0 and float(gf.abs().max()) > 0
    return gg


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,mask", MODES)
@pytest.mark.parametrize("shape,n_iter", CASES + FUSED_CASES)
def test_forward_and_backward_are_the_float32_engine_on_the_widened_guidance(shape, n_iter, norm, mask, dtype):
    gg = _assert_case(shape, n_iter, norm, mask, dtype, "auto")
    if (shape, n_iter) in FUSED_CASES:   # 'auto' took the persistent transposed instance; one launch per step against the float32 stepwise call
        _assert_case(shape, n_iter, norm, mask, dtype, "stepwise")
        _assert_case(shape, n_iter, norm, mask, dtype, "persistent")
    if mask != "nomask":
        # exact zeros wherever the gate's consumer voxel q - off_k is pinned (m = 1, u = 0)
        sparse = _inputs(shape, n_iter, mask, dtype)[2]
        pinned = (torch.sign(sparse[:, 0]) == 1).float()
        pad = torch.nn.functional.pad(pinned, (1, 1, 1, 1, 1, 1))
        D, H, W = shape[1:]
        at_consumer = torch.stack([pad[:, 1 - dz:1 - dz + D, 1 - dy:1 - dy + H, 1 - dx:1 - dx + W] for dz, dy, dx in OFF3], 1).bool()
        if norm == "none":   # gates used as given: the consumer of g_k(p) is p itself
            at_consumer = pinned[:, None].bool().expand(-1, 26, -1, -1, -1)
        assert bool(at_consumer.any()) and not bool(gg[at_consumer].any())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_persistent_is_refused_where_the_float32_call_refuses_it(dtype):
    g, feat, sparse, go = _inputs((1, 3, 6, 8), 4, "mask", dtype)
    for guidance in (g, g.float()):
        with pytest.raises(_lib.CspnError, match="persistent 3D kernel does not take this backward"):
            F.cspn3d_backward_norm(guidance, feat, sparse, go, 2, "8sum_abs", algo="persistent")


def _view_at(t, offset_bytes):
    """the same values in a contiguous view whose pointer is offset_bytes behind a 256-byte boundary"""
    assert offset_bytes % t.element_size() == 0
    k = offset_bytes // t.element_size()
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 256 == offset_bytes
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm,mask", [("8sum", "nomask"), ("8sum_abs", "mask"), ("none", "mask_neg")])
def test_alignment_classes(norm, mask, dtype):
    """a guidance 2 bytes off an 8-byte boundary takes the scalar kernels, as a float32 guidance 4 bytes off a 16-byte boundary does; one 8
    bytes off a 16-byte boundary still takes the vector kernels, as an aligned float32 guidance does"""
    shape, n = (1, 3, 6, 8), 4
    g, feat, sparse, go = _inputs(shape, n, mask, dtype)
    for off16, off32 in ((2, 4), (8, 0)):
        gv, rv = _view_at(g, off16), _view_at(g.float(), off32)
        out = F.cspn3d_forward_norm(gv, feat, sparse, n, norm)
        gg, gf = F.cspn3d_backward_norm(gv, feat, sparse, go, n, norm)
        ref_out = F.cspn3d_forward(rv, feat, sparse, n, norm)
        ref_gg, ref_gf = F.cspn3d_backward_norm(rv, feat, sparse, go, n, norm)
        F.cspn3d_check_status()
        assert _bitwise(out, ref_out) and _bitwise(gf, ref_gf) and _bitwise(gg, ref_gg.to(dtype)), (off16, off32)
        assert float(gg.float().abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("shape", [(1, 3, 6, 8), (1, 3, 5, 7)])
def test_subnormals_are_kept_and_the_sign_of_minus_zero_is_zero(shape, norm, dtype):
    g, feat, _, go = _make(shape, 9, "nomask", dtype)
    g[:, :, 1:, 2:5, 1:6] = (g[:, :, 1:, 2:5, 1:6].float() * 2.0 ** -20).to(dtype)   # a block of float16 subnormals (tiny normals in bfloat16)
    g.view(-1)[::53] = -0.0
    if dtype == torch.float16:
        mag = g.float().abs()
        assert bool(((mag > 0) & (mag < 2.0 ** -14)).any()), "no float16 subnormal in the guidance"
    minus_zero = (g.view(torch.int16) == -32768)
    assert bool(minus_zero.any())
    g, feat, go = g.cuda(), feat.cuda(), go.cuda()
    out = F.cspn3d_forward_norm(g, feat, None, 3, norm)
    gg, gf = F.cspn3d_backward_norm(g, feat, None, go, 3, norm)
    ref_out = F.cspn3d_forward(g.float(), feat, None, 3, norm)
    ref_gg, ref_gf = F.cspn3d_backward_norm(g.float(), feat, None, go, 3, norm)
    assert _bitwise(out, ref_out) and _bitwise(gf, ref_gf) and _bitwise(gg, ref_gg.to(dtype))
    assert bool(torch.isfinite(out).all())
    # flushing the block to zero would change the sums: the same call on the flushed guidance differs
    flushed = torch.where(g.float().abs() < 2.0 ** -14, torch.zeros_like(g), g) if dtype == torch.float16 else None
    if flushed is not None:
        assert not torch.equal(F.cspn3d_forward_norm(flushed, feat, None, 3, norm), out)
    if norm == "8sum_abs":   # d|g| / dg = sign(g), sign(-0) = 0
        assert not bool(gg[minus_zero.cuda()].any())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
def test_all_zero_neighbourhood_gives_the_float32_engines_nan_pattern(norm, dtype):
    """a zeroed 3 x 3 x 3 block of every gate plane: S = 0 at its centre voxel only; the NaN spreads one voxel per step, both ways"""
    shape, n = (1, 5, 6, 8), 2
    g, feat, sparse, go = _make(shape, 2, "mask", dtype)
    g[:, :, 1:4, 2:5, 3:6] = 0
    sparse[0, 0, 2, 3, 4] = 0
    g, feat, sparse, go = g.cuda(), feat.cuda(), sparse.cuda(), go.cuda()
    for sp in (None, sparse):
        out = F.cspn3d_forward_norm(g, feat, sp, n, norm)
        gg, gf = F.cspn3d_backward_norm(g, feat, sp, go, n, norm)
        ref_out = F.cspn3d_forward(g.float(), feat, sp, n, norm)
        ref_gg, ref_gf = F.cspn3d_backward_norm(g.float(), feat, sp, go, n, norm)
        for got, ref in ((out, ref_out), (gf, ref_gf), (gg, ref_gg.to(dtype))):
            assert bool(torch.isnan(ref).any()) and not bool(torch.isnan(ref).all())
            assert torch.equal(torch.isnan(got), torch.isnan(ref)) and _bitwise(got, ref)
    # a single voxel has no neighbour in range: out and grad_feat NaN, its own gates read by nobody: gradient 0
    g, feat, _, go = (t if t is None else t.cuda() for t in _make((1, 1, 1, 1), 1, "nomask", dtype))
    gg, gf = F.cspn3d_backward_norm(g, feat, None, go, 2, norm)
    assert bool(torch.isnan(F.cspn3d_forward_norm(g, feat, None, 2, norm)).all()) and bool(torch.isnan(gf).all()) and not bool(gg.any())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,n_iter", [((1, 3, 6, 8), 4), ((1, 8, 8, 64), 3), ((2, 4, 5, 7), 1)])
def test_either_output_alone_and_a_second_call(shape, n_iter, dtype):
    for norm, mask in (("8sum_abs", "mask"), ("none", "mask")):
        g, feat, sparse, go = _inputs(shape, n_iter, mask, dtype)
        gg, gf = F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm)
        gg1, none = F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm, need_feat=False)
        none2, gf1 = F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm, need_guidance=False)
        gg2, gf2 = F.cspn3d_backward_norm(g, feat, sparse, go, n_iter, norm)
        F.cspn3d_check_status()
        assert none is None and none2 is None
        assert gg1.dtype == dtype and _bitwise(gg1, gg) and _bitwise(gg2, gg) and _bitwise(gf1, gf) and _bitwise(gf2, gf)
        assert _bitwise(F.cspn3d_forward_norm(g, feat, sparse, n_iter, norm), F.cspn3d_forward_norm(g, feat, sparse, n_iter, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,n_iter", [((1, 3, 6, 8), 4), ((2, 6, 10, 64), 12), ((2, 4, 5, 7), 3)])
def test_none_without_a_mask_is_the_paddle_contracts_16_bit_calls(shape, n_iter, dtype):
    g, feat, _, go = _inputs(shape, n_iter, "nomask", dtype)
    want_gg, want_gf = F.cspn3d_backward(g, feat, go, n_iter)
    got_gg, got_gf = F.cspn3d_backward_norm(g, feat, None, go, n_iter, "none")
    F.cspn3d_check_status()
    assert got_gg.dtype == dtype and _bitwise(got_gg, want_gg) and _bitwise(got_gf, want_gf)
    assert _bitwise(F.cspn3d_forward_norm(g, feat, None, n_iter, "none"), F.cspn3d_forward(g, feat, None, n_iter, "none"))
    F.cspn3d_check_status()
    # float32 guidance: cspn3d_forward_norm is cspn3d_forward
    g32 = g.float()
    assert torch.equal(F.cspn3d_forward_norm(g32, feat, None, n_iter, "8sum"), F.cspn3d_forward(g32, feat, None, n_iter, "8sum"))


@pytest.mark.gpu
def test_cspn3d_forward_keeps_its_typeerror_for_16_bit_guidance_in_these_modes():
    g, x = torch.rand(1, 26, 2, 4, 8, device="cuda").half(), torch.rand(1, 1, 2, 4, 8, device="cuda")
    with pytest.raises(TypeError, match="float32"):
        F.cspn3d_forward(g, x, None, 3, "8sum")
    with pytest.raises(TypeError, match="float32"):
        F.cspn3d_forward_norm(g, x.double(), None, 3, "8sum")
    with pytest.raises(TypeError, match="float32"):
        F.cspn3d_forward_norm(g.double(), x, None, 3, "8sum")
    assert F.cspn3d_forward_norm(g, x, None, 3, "8sum").dtype == torch.float32


# ---- the module ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("norm", ["8sum", "8sum_abs"])
@pytest.mark.parametrize("shape,n_iter", [((2, 6, 10, 36), 12), ((1, 8, 8, 64), 3)])
def test_module_trains_on_a_16_bit_leaf_guidance(shape, n_iter, norm, dtype):
    g, feat, sparse, go = _inputs(shape, n_iter, "mask", dtype)
    m = cspn_amd.Affinity_Propagate3d(n_iter, 3, norm)
    g16, f16 = g.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    g32, f32 = g.float().requires_grad_(True), feat.clone().requires_grad_(True)
    out = m(g16, f16, sparse)
    # the autograd node is the module's own Function, fed by the leaf itself, and what it saved IS the 16-bit tensor: no cast, no copy
    node = out.grad_fn
    assert type(node).__name__ == "_CSPN3dNormFunctionBackward"
    saved = node.saved_tensors[0]
    assert saved.dtype == dtype and saved.data_ptr() == g16.data_ptr()
    producer = node.next_functions[0][0]
    assert type(producer).__name__ == "AccumulateGrad" and producer.variable is g16
    out.backward(go)
    ref = m(g32, f32, sparse)
    ref.backward(go)
    F.cspn3d_check_status()
    assert out.dtype == torch.float32 and _bitwise(out, ref)
    assert g16.grad.dtype == dtype and _bitwise(g16.grad, g32.grad.to(dtype)) and _bitwise(f16.grad, f32.grad)
    assert float(g16.grad.float().abs().max()) > 0
    assert m(g16, f16, sparse, n_iter=0) is f16


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_still_widens_16_bit_values_and_differentiates_through_the_cast(dtype):
    shape, n_iter = (1, 3, 6, 8), 4
    g, feat, sparse, go = _inputs(shape, n_iter, "mask", dtype)
    m = cspn_amd.Affinity_Propagate3d(n_iter, 3, "8sum_abs")
    b16 = feat.to(dtype).requires_grad_(True)
    b32 = feat.to(dtype).float().requires_grad_(True)
    s16 = sparse.to(dtype)
    g16 = g.clone().requires_grad_(True)
    g32 = g.float().requires_grad_(True)
    out = m(g16, b16, s16)
    out.backward(go)
    ref = m(g32, b32, s16.float())
    ref.backward(go)
    assert out.dtype == torch.float32 and _bitwise(out, ref)
    assert b16.grad.dtype == dtype and _bitwise(b16.grad, b32.grad.to(dtype))
    assert g16.grad.dtype == dtype and _bitwise(g16.grad, g32.grad.to(dtype))
    assert type(out.grad_fn.next_functions[1][0]).__name__ == "ToCopyBackward0"   # blur_depth reaches the Function through its cast


# ---- no float32 copy of the guidance or of its gradient ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_float32_copy_of_the_guidance_or_its_gradient_is_made(dtype):
    """the workspace is the float32 call's, so the peak of a backward call on 16-bit guidance is the float32 call's on the pre-widened
    guidance minus half the float32 gradient (6.8 MB here; + 4 MiB: two 2-MiB allocator blocks).  A float32 copy of the guidance would add
    13.6 MB, a float32 gradient 6.8 MB"""
    B, D, H, W, n = 2, 16, 32, 128, 3
    gen = torch.Generator(device="cuda").manual_seed(9)
    g16 = (torch.rand(B, 26, D, H, W, device="cuda", generator=gen) - 0.3).to(dtype)
    g32 = g16.float()
    x = torch.rand(B, 1, D, H, W, device="cuda", generator=gen)
    go = torch.randn(B, 1, D, H, W, device="cuda", generator=gen)
    half_gradient = 26 * B * D * H * W * 2
    assert half_gradient > 6e6

    def rise(guidance):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = F.cspn3d_backward_norm(guidance, x, None, go, n, "8sum_abs")
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, res

    rise(g32), rise(g16)   # (first calls: the library's own one-time allocations)
    r32, res32 = rise(g32)
    r16, res16 = rise(g16)
    F.cspn3d_check_status()
    print("peak rise: float32 %d B, 16-bit %d B" % (r32, r16))
    assert _bitwise(res16[1], res32[1]) and _bitwise(res16[0], res32[0].to(dtype))
    assert r16 <= r32 - half_gradient + (4 << 20)
